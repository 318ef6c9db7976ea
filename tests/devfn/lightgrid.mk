# Builds tests/devfn/liblightgrid_devfn.so: the TEST-ONLY device harness of pt_lightgrid.h (lightgrid_devfn.hip), with the product's own
# HIPFLAGS read from gpuspectral_amd/csrc/Makefile, as tests/devfn/Makefile builds libpt_devfn.so.
#   make -C tests/devfn -f lightgrid.mk
HIPCC ?= hipcc
ARCH ?= gfx950
CSRC := ../../gpuspectral_amd/csrc
HIPFLAGS := $(subst $$(ARCH),$(ARCH),$(shell sed -n 's/^HIPFLAGS ?= //p' $(CSRC)/Makefile))
OUT ?= liblightgrid_devfn.so
SRCS := lightgrid_devfn.hip lightgrid_bodies.h devfn_bodies.h
HDRS := $(CSRC)/pt_lightgrid.h $(CSRC)/pt_lightpick.h $(CSRC)/pt_envlight.h $(CSRC)/pt_deltalight.h $(CSRC)/pt_medium.h $(CSRC)/pt_math.h $(CSRC)/pt_shading.h $(CSRC)/pt_trace.h $(CSRC)/pt_stages.h ../../include/gpuspectral_pt.h
# digest of the harness sources and the product headers they include (in this order), as tests/lightgrid_util.py recomputes it
DIGEST := $(shell cat $(SRCS) $(HDRS) | sha256sum | cut -c1-16)
BUILDINFO := arch=$(ARCH) digest=$(DIGEST) flags=$(filter-out --offload-arch=%,$(HIPFLAGS))

all: $(OUT)

# (one hipcc call, source to library: no object file that would have to be rebuilt where only the library travels)
$(OUT): $(SRCS) $(HDRS) lightgrid.mk $(CSRC)/Makefile
	$(HIPCC) $(HIPFLAGS) -DDEVFN_BUILD_INFO='"$(BUILDINFO)"' -shared -o $@ lightgrid_devfn.hip

.PHONY: all
