// tests/emu/trace_work_ref.cpp -- TEST REFERENCE, NOT A PRODUCT PATH.
//
// The work a ray OUGHT to cost on a given wide tree, in double, for tests/trace_work.py.  Stand-alone: it includes nothing of the
// product and nothing of oracle/.  The 64-byte node record is decoded from the layout comment at the top of
// gpuspectral_amd/csrc/pt_trace.h ("HBM layout"), not from node_test, and the order words are never read:
//   words 0..2  origin.xyz (float)            word 3       scale.x (float)
//   words 4..6  qlo.x / qlo.y / qlo.z         word 7       qhi.x            one byte per child, child k = byte k
//   words 8..9  qhi.y / qhi.z                 word 10      child_base       word 11  tri_base - ni
//   word 12     bits 28..31: mask of the inner positions (ni = its popcount)          words 14..15 scale.y, scale.z (float)
//   plane = origin + q * scale; a position with qlo > qhi on an axis is unused; positions < ni are the nodes child_base + p, the
//   others the triangle slots (tri_base - ni) + p.
// Triangle packets: 12 floats per slot, vertices at floats 0..2, 4..6, 8..10; float 3 carries (global id << 3 | type) as bits.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

struct Child {
  double lo[3], hi[3];
  bool used;
};
struct Node {
  Child c[4];
  int ni;
  uint32_t child_base, tri_base_minus_ni;
};

float as_float(uint32_t w) {
  float f;
  std::memcpy(&f, &w, 4);
  return f;
}

Node decode(const uint32_t* w) {
  Node n;
  const double origin[3] = {as_float(w[0]), as_float(w[1]), as_float(w[2])};
  const double scale[3] = {as_float(w[3]), as_float(w[14]), as_float(w[15])};
  const uint32_t qlo[3] = {w[4], w[5], w[6]}, qhi[3] = {w[7], w[8], w[9]};
  n.child_base = w[10];
  n.tri_base_minus_ni = w[11];
  n.ni = __builtin_popcount(w[12] >> 28);
  for (int k = 0; k < 4; ++k) {
    n.c[k].used = true;
    for (int a = 0; a < 3; ++a) {
      const uint32_t l = (qlo[a] >> (8 * k)) & 255u, h = (qhi[a] >> (8 * k)) & 255u;
      if (l > h) n.c[k].used = false;
      n.c[k].lo[a] = origin[a] + (double)l * scale[a];
      n.c[k].hi[a] = origin[a] + (double)h * scale[a];
    }
  }
  return n;
}

struct Ray {
  double o[3], d[3], tmin, tmax;
};

// exact slab test: does the segment [t0, t1] of the ray meet the closed box?  entry = the parameter at which it does
bool enters(const Ray& r, const Child& b, double t0, double t1, double& entry) {
  double tn = t0, tf = t1;
  for (int a = 0; a < 3; ++a) {
    if (r.d[a] == 0.0) {
      if (r.o[a] < b.lo[a] || r.o[a] > b.hi[a]) return false;
      continue;
    }
    double x = (b.lo[a] - r.o[a]) / r.d[a], y = (b.hi[a] - r.o[a]) / r.d[a];
    if (x > y) std::swap(x, y);
    tn = std::max(tn, x);
    tf = std::min(tf, y);
  }
  entry = tn;
  return tn <= tf;
}

// Moeller-Trumbore in double; u, v = weights of v1, v2
bool moller_trumbore(const float* p, const Ray& r, double& t) {
  const double v0[3] = {p[0], p[1], p[2]}, e1[3] = {p[4] - v0[0], p[5] - v0[1], p[6] - v0[2]},
               e2[3] = {p[8] - v0[0], p[9] - v0[1], p[10] - v0[2]};
  const double pv[3] = {r.d[1] * e2[2] - r.d[2] * e2[1], r.d[2] * e2[0] - r.d[0] * e2[2], r.d[0] * e2[1] - r.d[1] * e2[0]};
  const double det = e1[0] * pv[0] + e1[1] * pv[1] + e1[2] * pv[2];
  if (det == 0.0) return false;
  const double s[3] = {r.o[0] - v0[0], r.o[1] - v0[1], r.o[2] - v0[2]};
  const double u = (s[0] * pv[0] + s[1] * pv[1] + s[2] * pv[2]) / det;
  const double q[3] = {s[1] * e1[2] - s[2] * e1[1], s[2] * e1[0] - s[0] * e1[2], s[0] * e1[1] - s[1] * e1[0]};
  const double v = (r.d[0] * q[0] + r.d[1] * q[1] + r.d[2] * q[2]) / det;
  t = (e2[0] * q[0] + e2[1] * q[1] + e2[2] * q[2]) / det;
  return u >= 0.0 && v >= 0.0 && u + v <= 1.0 && t > r.tmin && t < r.tmax;
}

uint32_t global_id(const float* p) {
  uint32_t w;
  std::memcpy(&w, p + 3, 4);
  return w >> 3;
}

}  // namespace

extern "C" {

// lo, hi: num_nodes x 4 x 3 doubles; used: num_nodes x 4; ni, child_base, tri_base_minus_ni: num_nodes
void twr_decode(const uint32_t* nodes, uint64_t num_nodes, double* lo, double* hi, uint8_t* used, int32_t* ni, uint32_t* child_base,
                uint32_t* tri_base_minus_ni) {
  for (uint64_t i = 0; i < num_nodes; ++i) {
    const Node n = decode(nodes + 16 * i);
    ni[i] = n.ni;
    child_base[i] = n.child_base;
    tri_base_minus_ni[i] = n.tri_base_minus_ni;
    for (int k = 0; k < 4; ++k) {
      used[4 * i + k] = n.c[k].used;
      for (int a = 0; a < 3; ++a) lo[12 * i + 3 * k + a] = n.c[k].lo[a], hi[12 * i + 3 * k + a] = n.c[k].hi[a];
    }
  }
}

// rays: n x {o.xyz, tmin, d.xyz, tmax} (float).  Per ray:
//   t_hit / slot_hit  the closest hit of the brute force over the slots [0, num_real_slots) (ties: the smaller global id); a miss
//                     gives t_hit = tmax, slot_hit = -1
//   w_min             node records a traversal that knew t_hit would read: the root, and every record reached from it through
//                     inner-child boxes that the segment [tmin, t_hit] enters
//   w_sorted          node records the textbook ordered traversal fetches: depth first, a record's hit inner children by ascending
//                     entry distance, a stacked record whose entry lies beyond the best t so far is dropped unfetched
//   tris_sorted       triangle tests of that traversal;  slot_sorted: its hit (must equal slot_hit)
void twr_work(const uint32_t* nodes, uint64_t num_nodes, const float* packets, uint64_t num_real_slots, const float* rays, uint64_t n,
              double* t_hit, int64_t* slot_hit, uint32_t* w_min, uint32_t* w_sorted, uint32_t* tris_sorted, int64_t* slot_sorted) {
  std::vector<Node> tree(num_nodes);
  for (uint64_t i = 0; i < num_nodes; ++i) tree[i] = decode(nodes + 16 * i);
  for (uint64_t i = 0; i < n; ++i) {
    const float* f = rays + 8 * i;
    Ray r;
    for (int a = 0; a < 3; ++a) r.o[a] = f[a], r.d[a] = f[4 + a];
    r.tmin = f[3];
    r.tmax = f[7];
    // ---- brute force ----
    double best = r.tmax;
    int64_t best_slot = -1;
    for (uint64_t s = 0; s < num_real_slots; ++s) {
      double t;
      if (!moller_trumbore(packets + 12 * s, r, t)) continue;
      if (t < best || (t == best && best_slot >= 0 && global_id(packets + 12 * s) < global_id(packets + 12 * best_slot))) best = t, best_slot = (int64_t)s;
    }
    t_hit[i] = best;
    slot_hit[i] = best_slot;
    // ---- the ideal ----
    uint32_t count = 0;
    std::vector<uint32_t> todo;
    if (num_nodes) todo.push_back(0);
    while (!todo.empty()) {
      const Node& nd = tree[todo.back()];
      todo.pop_back();
      ++count;
      for (int k = 0; k < nd.ni; ++k) {
        double entry;
        if (nd.c[k].used && enters(r, nd.c[k], r.tmin, best, entry)) todo.push_back(nd.child_base + (uint32_t)k);
      }
    }
    w_min[i] = count;
    // ---- the exact sort ----
    struct Entry {
      uint32_t node;
      double entry;
    };
    std::vector<Entry> stack;
    if (num_nodes) stack.push_back(Entry{0u, r.tmin});
    double cur = r.tmax;
    int64_t cur_slot = -1;
    uint32_t fetched = 0, tested = 0;
    while (!stack.empty()) {
      const Entry e = stack.back();
      stack.pop_back();
      if (e.entry > cur) continue;  // beyond the best hit so far: never fetched
      const Node& nd = tree[e.node];
      ++fetched;
      for (int k = nd.ni; k < 4; ++k) {
        double entry;
        if (!nd.c[k].used || !enters(r, nd.c[k], r.tmin, cur, entry)) continue;
        const uint64_t s = (uint64_t)nd.tri_base_minus_ni + (uint64_t)k;
        ++tested;
        double t;
        if (s >= num_real_slots || !moller_trumbore(packets + 12 * s, r, t)) continue;
        if (t < cur || (t == cur && cur_slot >= 0 && global_id(packets + 12 * s) < global_id(packets + 12 * cur_slot))) cur = t, cur_slot = (int64_t)s;
      }
      Entry hit[4];
      int nh = 0;
      for (int k = 0; k < nd.ni; ++k) {
        double entry;
        if (nd.c[k].used && enters(r, nd.c[k], r.tmin, cur, entry)) hit[nh++] = Entry{nd.child_base + (uint32_t)k, entry};
      }
      std::stable_sort(hit, hit + nh, [](const Entry& a, const Entry& b) { return a.entry > b.entry; });  // farthest first: popped last
      for (int k = 0; k < nh; ++k) stack.push_back(hit[k]);
    }
    w_sorted[i] = fetched;
    tris_sorted[i] = tested;
    slot_sorted[i] = cur_slot;
  }
}
}
