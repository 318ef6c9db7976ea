# Builds tests/devfn/libenvlight_devfn.so: the TEST-ONLY device harness of pt_envlight.h (envlight_devfn.hip), with the product's own
# HIPFLAGS read from gpuspectral_amd/csrc/Makefile, as tests/devfn/Makefile builds libpt_devfn.so.
#   make -C tests/devfn -f envlight.mk
HIPCC ?= hipcc
ARCH ?= gfx950
CSRC := ../../gpuspectral_amd/csrc
HIPFLAGS := $(subst $$(ARCH),$(ARCH),$(shell sed -n 's/^HIPFLAGS ?= //p' $(CSRC)/Makefile))
OUT ?= libenvlight_devfn.so
SRCS := envlight_devfn.hip envlight_bodies.h devfn_bodies.h
HDRS := $(CSRC)/pt_envlight.h $(CSRC)/pt_deltalight.h $(CSRC)/pt_medium.h $(CSRC)/pt_math.h $(CSRC)/pt_shading.h $(CSRC)/pt_trace.h $(CSRC)/pt_stages.h ../../include/gpuspectral_pt.h
# digest of the harness sources and the product headers they include (in this order), as tests/envlight_util.py recomputes it
DIGEST := $(shell cat $(SRCS) $(HDRS) | sha256sum | cut -c1-16)
BUILDINFO := arch=$(ARCH) digest=$(DIGEST) flags=$(filter-out --offload-arch=%,$(HIPFLAGS))

all: $(OUT)

# (one hipcc call, source to library: no object file that would have to be rebuilt where only the library travels)
$(OUT): $(SRCS) $(HDRS) envlight.mk $(CSRC)/Makefile
	$(HIPCC) $(HIPFLAGS) -DDEVFN_BUILD_INFO='"$(BUILDINFO)"' -shared -o $@ envlight_devfn.hip

.PHONY: all
