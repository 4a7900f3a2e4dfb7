// bvh_cover_main.hip -- what the binary-tree walk of odw_kernels.hip (nearest<BVH = true>) and the mesh kernel take for
// granted in the tables build_accel (csrc/odw_build.h) hands them, checked by brute force, under AddressSanitizer +
// UndefinedBehaviorSanitizer.
//
// A program of its own (tests/test_native_bvh_cover.py compiles and runs it; no GPU, no Python, nothing preloaded).
// Layouts: those of grid_cover_main.hip (the random ones from a generator of its own), the lattice moved to
// (3000, -7000, 11000), 80 and 1000 coincident boxes (every SAH cost ties: one primitive peeled per level), a geometric
// chain of spheres (ratio 1.5), 5000 random boxes (the binned route), 2000 boxes whose centroids coincide on two axes,
// a single primitive and a scene of dead primitives only (the wrapper root), cubes of 12 triangles (the eight-wide tree
// too), 200 boxes with extents of 1e200 (every SAH cost infinite).  Held on each:
//   coverage  every live primitive in exactly one leaf, the leaves partition `order`, entries and children in range, no
//             node reachable twice, every node reached from node 0;
//   boxes     each child box (float32) contains the enlarged float64 boxes of everything below it, and the un-enlarged
//             boxes grown by the float32 ulp of |lo| and |hi|; the absent child of a wrapper root is the far point, which
//             the walk's slab test accepts for no ray;
//   depth     max_depth is the true height, max_depth + 2 <= ODW_BVH_STACK; the coincident layouts reach 20 levels or more;
//   leaves    count <= kBvhLeaf, first + count <= 1 << 24, the leaf word decodes back with the kernel's expressions;
//   wide      each slot's decoded box contains everything below the slot, every facet in exactly one leaf record,
//             depth <= kWideMaxDepth, at most 15 facets per slot, the solid words agree with prim_solid.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "odw_kernels.hip"
#include "odw_grid.hip"
#include "odw_mesh.hip"
#include "odw_build.h"

namespace {

constexpr double kTol = 1e-6;

// splitmix64 -> uniform doubles
struct Rng {
  uint64_t s;
  double next(double lo, double hi) {
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    z ^= z >> 31;
    return lo + (hi - lo) * ((double)(z >> 11) * (1.0 / 9007199254740992.0));
  }
};

struct Layout {
  std::string name;
  std::vector<int32_t> type, group, solid, flags, cond_off{0};
  std::vector<double> xform, params;
  std::vector<Box> boxes;          // not empty: these boxes in place of compute_boxes' (one per primitive)
  bool all_dead = false;           // no live primitive: build_accel hangs primitive 0 under a wrapper root
  bool force_tree = false;         // (scenes the flat loop would take, and those no grid need be built for)
  bool wrapper = false;            // expected: one leaf under a wrapper root
  bool may_refuse = false;         // a refusal with a message is an answer too
  int min_depth = 0;               // levels the tree has to reach
  int wide = 0;                    // expected: the eight-wide tree is built

  // centre and half-widths (a sphere: h[0] the radius)
  void solid_at(int t, const double* c, const double* h) {
    const int p = (int)type.size();
    type.push_back(t); group.push_back(p % 2); solid.push_back(p);
    flags.push_back(ODW_FLAG_CONVEX | ((t == ODW_PRIM_BOX ? 0x3f : 1) << ODW_FACEMASK_SHIFT));
    for (int r = 0; r < 3; ++r) {
      for (int k = 0; k < 3; ++k) xform.push_back(r == k ? 1.0 : 0.0);
      xform.push_back(-(t == ODW_PRIM_BOX ? c[r] - h[r] : c[r]));
    }
    if (t == ODW_PRIM_BOX) for (double v : {2 * h[0], 2 * h[1], 2 * h[2], 0.0}) params.push_back(v);
    else if (t == ODW_PRIM_SPHERE) for (double v : {h[0], 0.0, 0.0, 0.0}) params.push_back(v);
    else for (double v : {h[0], h[1], h[2], 0.0}) params.push_back(v);
    cond_off.push_back(0);
  }
  void sphere(double x, double y, double z, double r) {
    const double c[3] = {x, y, z}, h[3] = {r, r, r};
    solid_at(ODW_PRIM_SPHERE, c, h);
  }
  void facet(int s, const double* v0, const double* v1, const double* v2) {
    for (const double* v : {v0, v1, v2}) xform.insert(xform.end(), v, v + 3);
    xform.insert(xform.end(), 3, 0.0);
    type.push_back(ODW_PRIM_TRIANGLE); group.push_back(0); solid.push_back(s);
    flags.push_back(ODW_FLAG_CONVEX | (1 << ODW_FACEMASK_SHIFT));
    params.insert(params.end(), 4, 0.0);
    cond_off.push_back(0);
  }
  // the cube [c - h, c + h] as 12 triangles, counter-clockwise from outside
  void cube(int s, double x, double y, double z, double h) {
    const double c[3] = {x, y, z};
    for (int a = 0; a < 3; ++a)
      for (int side = 0; side < 2; ++side) {
        const int b = (a + 1) % 3, e = (a + 2) % 3;
        double v[4][3];
        for (int k = 0; k < 4; ++k) {
          const double sb = (k == 1 || k == 2) ? h : -h, se = (k >= 2) ? h : -h;
          v[k][a] = c[a] + (side ? h : -h); v[k][b] = c[b] + sb; v[k][e] = c[e] + se;
        }
        if (side) { facet(s, v[0], v[1], v[2]); facet(s, v[0], v[2], v[3]); }
        else { facet(s, v[0], v[2], v[1]); facet(s, v[0], v[3], v[2]); }
      }
  }
};

Layout lattice(bool mixed, const double* T, const char* name) {
  Layout l;
  l.name = name;
  int i = 0;
  for (int x = 0; x < 5; ++x)
    for (int y = 0; y < 4; ++y)
      for (int z = 0; z < 4; ++z, ++i) {
        const double c[3] = {10.0 * x + T[0], 10.0 * y + T[1], 10.0 * z + T[2]}, h[3] = {2.0, 2.0, 2.0};
        l.solid_at(mixed && i % 3 == 1 ? ODW_PRIM_BOX : ODW_PRIM_SPHERE, c, h);
      }
  return l;
}

Layout cloud() {
  Layout l;
  l.name = "cloud";
  Rng g{3};
  for (int i = 0; i < 90; ++i) {
    const double x = g.next(-30, 30), y = g.next(-30, 30), z = g.next(-30, 30);
    l.sphere(x, y, z, g.next(1, 9));
  }
  return l;
}

Layout staggered() {
  Layout l;
  l.name = "staggered";
  for (int i = 0; i < 5; ++i)
    for (int j = 0; j < 4; ++j)
      for (int k = 0; k < 4; ++k) l.sphere(6.0 * i + 3 * (j % 2), 6.0 * j + 3 * (k % 2), 6.0 * k + 3 * (i % 2), 2.5);
  return l;
}

Layout big() {
  Layout l;
  l.name = "13^3 lattice";
  for (int i = 0; i < 13; ++i)
    for (int j = 0; j < 13; ++j)
      for (int k = 0; k < 13; ++k) l.sphere(10.0 * i, 10.0 * j, 10.0 * k, 2 + 0.001 * (i % 7));
  return l;
}

Layout seventy() {
  Layout l;
  l.name = "seventy";
  Rng g{5};
  const int kinds[3] = {ODW_PRIM_SPHERE, ODW_PRIM_BOX, ODW_PRIM_ELLIPSOID};
  for (int i = 0; i < 70; ++i) {
    const double c[3] = {g.next(-200, 200), g.next(-200, 200), g.next(-200, 200)};
    double h[3] = {g.next(1, 3), g.next(1, 3), g.next(1, 3)};
    if (kinds[i % 3] == ODW_PRIM_SPHERE) h[1] = h[2] = h[0];
    l.solid_at(kinds[i % 3], c, h);
  }
  return l;
}

Layout line() {
  Layout l;
  l.name = "line of 300";
  for (int i = 0; i < 300; ++i) l.sphere(1.0 * i, 0.0, 0.0, 0.25);
  return l;
}

// m unit spheres whose boxes are replaced by `box(i)`
Layout of_boxes(const char* name, int m, const std::function<Box(int)>& box) {
  Layout l;
  l.name = name;
  l.force_tree = true;
  for (int i = 0; i < m; ++i) { l.sphere(0.0, 0.0, 0.0, 1.0); l.boxes.push_back(box(i)); }
  return l;
}

Layout coincident(const char* name, int m) {
  Layout l = of_boxes(name, m, [](int) { return Box{{-1.5, 2.0, -3.0}, {2.5, 4.25, 1.0}}; });
  l.min_depth = 20;
  return l;
}

Layout chain() {
  Layout l;
  l.name = "geometric chain";
  l.force_tree = true;
  double x = 0.0, r = 1e-3;
  for (int i = 0; i < 40; ++i, r *= 1.5) { x += 2.5 * r; l.sphere(x, 0.1 * r, -0.2 * r, r); }
  return l;
}

Layout random_boxes() {
  Rng g{17};
  return of_boxes("5000 random boxes", 5000, [&](int) {
    Box b;
    for (int a = 0; a < 3; ++a) { const double c = g.next(-500, 500), h = g.next(0.01, 20); b.lo[a] = c - h; b.hi[a] = c + h; }
    return b;
  });
}

Layout two_axes() {
  Rng g{23};
  return of_boxes("2000 on a line", 2000, [&](int) {
    Box b;
    const double c[3] = {7.0, g.next(-300, 300), -4.0};
    for (int a = 0; a < 3; ++a) { const double h = a == 1 ? g.next(0.1, 2) : 3.0; b.lo[a] = c[a] - h; b.hi[a] = c[a] + h; }
    return b;
  });
}

Layout single() {
  Layout l;
  l.name = "single primitive";
  l.force_tree = l.wrapper = true;
  l.sphere(3.0, -2.0, 8.0, 1.5);
  return l;
}

Layout none_alive() {
  Layout l;
  l.name = "no live primitive";
  l.force_tree = l.wrapper = l.all_dead = true;
  for (int i = 0; i < 6; ++i) l.sphere(4.0 * i, 0.0, 0.0, 1.0);
  return l;
}

Layout cubes() {
  Layout l;
  l.name = "12-triangle cubes";
  l.wide = 1;
  int i = 0;
  for (int x = 0; x < 5; ++x)
    for (int y = 0; y < 4; ++y)
      for (int z = 0; z < 4; ++z, ++i)
        if (i % 3 == 1) l.cube(i / 3, 10.0 * x, 10.0 * y, 10.0 * z, 2.0);
  return l;
}

Layout huge_extents() {
  Rng g{29};
  Layout l = of_boxes("200 boxes of 1e200", 200, [&](int) {
    Box b;
    for (int a = 0; a < 3; ++a) { const double c = g.next(-10, 10); b.lo[a] = c - 0.5e200; b.hi[a] = c + 0.5e200; }
    return b;
  });
  l.may_refuse = true;
  return l;
}

int bad = 0;
#define HOLD(cond, ...) do { if (!(cond)) { if (++bad < 40) { fprintf(stderr, "%s: ", l.name.c_str()); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } } while (0)

// the slab test of the walk (odw_kernels.hip, nearest<BVH = true>), in float32 as it stands there
bool walk_accepts(const float* lo, const float* hi, const float* o, const float* iv, float cutf) {
  const float x0 = (lo[0] - o[0]) * iv[0], x1 = (hi[0] - o[0]) * iv[0];
  const float y0 = (lo[1] - o[1]) * iv[1], y1 = (hi[1] - o[1]) * iv[1];
  const float z0 = (lo[2] - o[2]) * iv[2], z1 = (hi[2] - o[2]) * iv[2];
  const float tn = fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fminf(z0, z1));
  const float tf = fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fmaxf(z0, z1));
  return tf * 1.00001f + 1e-3f >= fmaxf(tn, 0.f) * 0.99999f - 1e-3f && tn * 0.99999f - 1e-3f < cutf;
}

double ulp32(double v) {
  const float f = std::fabs((float)v);
  if (!(f < FLT_MAX)) return 0.0;
  return (double)std::nextafterf(f, INFINITY) - (double)f;
}

struct Walk {
  const Layout& l;
  const SceneAccel& A;
  const std::vector<Box>& plain;         // as compute_boxes (or the layout) gave them
  std::vector<Box> grown;                // as build_accel enlarges them
  std::vector<int> node_seen, entry_seen, prim_seen;
  int height = 0, largest_leaf = 0, leaves = 0;

  Walk(const Layout& l_, const SceneAccel& A_, const std::vector<Box>& b) : l(l_), A(A_), plain(b), grown(b) {
    for (Box& g : grown)
      for (int a = 0; a < 3; ++a) {
        const double s = 1e-4 + 4e-7 * (std::fabs(g.lo[a]) + std::fabs(g.hi[a]));
        g.lo[a] -= s;
        g.hi[a] += s;
      }
    node_seen.assign(A.nodes.size(), 0);
    entry_seen.assign(A.order.size(), 0);
    prim_seen.assign(plain.size(), 0);
  }

  // everything below one child of node n, met at `depth`: -> the float64 box of what lies below it
  Box child(int n, int which, int depth) {
    const BvhNode& nd = A.nodes[n];
    const float* lo = which ? nd.lo1 : nd.lo0;
    const float* hi = which ? nd.hi1 : nd.hi0;
    const int32_t link = which ? nd.child1 : nd.child0, count = which ? nd.count1 : nd.count0;
    Box below;
    below.reset();
    height = std::max(height, depth);
    if (count > 0) {
      ++leaves;
      largest_leaf = std::max(largest_leaf, (int)count);
      HOLD(count <= kBvhLeaf, "node %d: a leaf of %d primitives, kBvhLeaf is %d", n, count, kBvhLeaf);
      HOLD(link >= 0 && (size_t)link + (size_t)count <= A.order.size() && (size_t)link + (size_t)count <= ((size_t)1 << 24),
           "node %d: leaf [%d, %d + %d) of %zu entries", n, link, link, count, A.order.size());
      if (count <= 127 && link >= 0 && link < (1 << 24)) {
        // the kernel's expressions, both ways
        const int r = -2 - (link | (count << 24));
        const int code = -2 - r;
        HOLD(r < -1 && (code & 0xffffff) == link && (code >> 24) == count, "node %d: leaf word %d decodes to (%d, %d), not (%d, %d)", n, r,
             code & 0xffffff, code >> 24, link, count);
      }
      for (int k = 0; k < count; ++k) {
        const size_t e = (size_t)link + k;
        if (link < 0 || e >= A.order.size()) break;
        ++entry_seen[e];
        const int p = A.order[e];
        HOLD(p >= 0 && p < (int)plain.size(), "order[%zu] = %d of %zu primitives", e, p, plain.size());
        if (p < 0 || p >= (int)plain.size()) continue;
        ++prim_seen[p];
        below.grow(grown[p]);
        for (int a = 0; a < 3; ++a)
          HOLD((double)lo[a] <= plain[p].lo[a] - ulp32(plain[p].lo[a]) && (double)hi[a] >= plain[p].hi[a] + ulp32(plain[p].hi[a]),
               "node %d child %d axis %d: [%.9g, %.9g] does not hold primitive %d grown by an ulp: [%.17g, %.17g]", n, which, a, lo[a], hi[a], p,
               plain[p].lo[a], plain[p].hi[a]);
      }
    } else {
      HOLD(link > 0 && link < (int)A.nodes.size(), "node %d: child %d of %zu nodes", n, link, A.nodes.size());
      if (link <= 0 || link >= (int)A.nodes.size()) return below;
      below = node(link, depth);
    }
    for (int a = 0; a < 3; ++a)
      HOLD((double)lo[a] <= below.lo[a] && (double)hi[a] >= below.hi[a], "node %d child %d axis %d: [%.9g, %.9g] does not hold [%.17g, %.17g] below it", n,
           which, a, lo[a], hi[a], below.lo[a], below.hi[a]);
    return below;
  }

  Box node(int n, int depth) {
    Box below;
    below.reset();
    if (++node_seen[n] > 1) { HOLD(false, "node %d is reachable twice", n); return below; }
    below.grow(child(n, 0, depth + 1));
    below.grow(child(n, 1, depth + 1));
    return below;
  }
};

// the absent child of a wrapper root: the far point, which the slab test accepts for no ray
void check_far_child(const Layout& l, const BvhNode& nd) {
  for (int a = 0; a < 3; ++a) HOLD(nd.lo1[a] == 3.0e38f && nd.hi1[a] == 3.0e38f, "absent child, axis %d: [%g, %g]", a, nd.lo1[a], nd.hi1[a]);
  HOLD(nd.child1 == 0 && nd.count1 == 0, "absent child: link %d, count %d", nd.child1, nd.count1);
  const double comps[] = {1.0, -1.0, 0.0, -0.0, 1e-40, -1e-40, 1e-30, -1e-30, 1e-17, 0.3, -0.7};
  const float origins[] = {0.0f, -1e4f, 1e4f, 1e30f};
  // (cut: the walk's (float)min(tmax, t + 2 tol) * 1.00001f + 1e-3f; coordinates and ray lengths up to 1e30 mm -- a ray
  //  that starts at the far point itself, or may run 3e38 mm, does reach it)
  int accepted = 0, tried = 0;
  for (double dx : comps)
    for (double dy : comps)
      for (double dz : comps)
        for (float ox : origins)
          for (float cut : {1000.0f, 1.0e30f}) {
            const float o[3] = {ox, -ox, 0.5f * ox};
            const float iv[3] = {(float)(1.0 / dx), (float)(1.0 / dy), (float)(1.0 / dz)};
            accepted += walk_accepts(nd.lo1, nd.hi1, o, iv, cut * 1.00001f + 1e-3f);
            ++tried;
          }
  HOLD(accepted == 0, "the slab test accepts the absent child for %d of %d rays", accepted, tried);
}

// ---- the eight-wide tree: slot boxes, leaf records, depth, solid words
struct WideWalk {
  const Layout& l;
  const SceneAccel& A;
  const std::vector<Box>& grown;
  const std::vector<int>& prim_solid;
  std::vector<int> rec_seen, prim_seen, node_seen;
  int depth = 0, most = 0;

  // -> the primitives below node `index`
  std::vector<int> node(size_t index, int d) {
    std::vector<int> all;
    depth = std::max(depth, d);
    if ((index + 1) * kWideWords > A.wide_nodes.size()) { HOLD(false, "wide node %zu of %zu", index, A.wide_nodes.size() / kWideWords); return all; }
    if (++node_seen[index] > 1 || d > 64) { HOLD(false, "wide node %zu is reachable twice", index); return all; }
    const uint32_t* w = &A.wide_nodes[index * kWideWords];
    double corner[3], unit[3];
    for (int a = 0; a < 3; ++a) {
      float c, u;
      const uint32_t eb = ((w[3] >> (8 * a)) & 0xffu) << 23;
      std::memcpy(&c, &w[a], 4);
      std::memcpy(&u, &eb, 4);
      corner[a] = c; unit[a] = u;
    }
    const uint32_t imask = w[6] & 0xffu, lmask = (w[6] >> 8) & 0xffu;
    HOLD((imask & lmask) == 0, "wide node %zu: slots both inner and leaf (%02x, %02x)", index, imask, lmask);
    size_t rec = w[5];
    int rank = 0;
    for (int sl = 0; sl < 8; ++sl) {
      const int count = (int)((w[7] >> (4 * sl)) & 15u);
      std::vector<int> below;
      if (imask & (1u << sl)) {
        HOLD(count == 0, "wide node %zu slot %d: an inner slot with %d facets", index, sl, count);
        below = node((size_t)w[4] + rank, d + 1);
        ++rank;
      } else if (lmask & (1u << sl)) {
        HOLD(count >= 1 && count <= 15, "wide node %zu slot %d: %d facets", index, sl, count);
        most = std::max(most, count);
        for (int k = 0; k < count; ++k, ++rec) {
          if ((rec + 1) * ODW_LEAF_WORDS > A.leaf_recs.size()) { HOLD(false, "leaf record %zu of %zu", rec, A.leaf_recs.size() / ODW_LEAF_WORDS); break; }
          ++rec_seen[rec];
          int p;
          std::memcpy(&p, &A.leaf_recs[rec * ODW_LEAF_WORDS + 12], 4);
          HOLD(p >= 0 && p < (int)grown.size(), "leaf record %zu names primitive %d", rec, p);
          if (p >= 0 && p < (int)grown.size()) { ++prim_seen[p]; below.push_back(p); }
        }
      } else {
        HOLD(count == 0, "wide node %zu slot %d: an empty slot with %d facets", index, sl, count);
        continue;
      }
      // the slot's box as the layout comment above kWideWords decodes it
      int so = below.empty() ? -1 : prim_solid[below[0]];
      for (int p : below) {
        if (prim_solid[p] != so) so = -1;
        for (int a = 0; a < 3; ++a) {
          const uint32_t bl = (w[8 + 2 * a + (sl >> 2)] >> (8 * (sl & 3))) & 0xffu, bh = (w[14 + 2 * a + (sl >> 2)] >> (8 * (sl & 3))) & 0xffu;
          const double lo = corner[a] + bl * unit[a], hi = corner[a] + bh * unit[a];
          HOLD(lo <= grown[p].lo[a] && hi >= grown[p].hi[a], "wide node %zu slot %d axis %d: [%.9g, %.9g] does not hold primitive %d: [%.17g, %.17g]", index,
               sl, a, lo, hi, p, grown[p].lo[a], grown[p].hi[a]);
        }
      }
      const uint32_t word = (w[20 + (sl >> 1)] >> (16 * (sl & 1))) & 0xffffu;
      HOLD(word == (uint32_t)((so >= 0 && so < 0xffff) ? so : 0xffff), "wide node %zu slot %d: solid word %04x, the primitives below say %d", index, sl, word, so);
      all.insert(all.end(), below.begin(), below.end());
    }
    return all;
  }
};

void check(const Layout& l) {
  const int n = (int)l.type.size();
  const int32_t gtype[2] = {ODW_OPT_VACUUM, ODW_OPT_VACUUM}, grecord[2] = {1, 1};
  const double gior[2] = {1.0, 1.0}, grefl[2] = {0.0, 0.0}, gabs[2] = {INFINITY, INFINITY};
  odw_scene_desc d;
  std::memset(&d, 0, sizeof d);
  d.n_prims = n;
  d.prim_type = l.type.data(); d.prim_group = l.group.data(); d.prim_solid = l.solid.data(); d.prim_flags = l.flags.data();
  d.prim_xform = l.xform.data(); d.prim_params = l.params.data(); d.prim_cond_off = l.cond_off.data();
  d.n_groups = 2;
  d.group_type = gtype; d.group_ior = gior; d.group_refl = grefl; d.group_abslen = gabs; d.group_record = grecord;

  HostScene hs;
  std::string err;
  int rc = scene_host_tables(&d, hs, err);
  HOLD(rc == ODW_OK, "scene refused (%d): %s", rc, err.c_str());
  if (rc) return;
  std::vector<Box> boxes;
  compute_boxes(hs, kTol, boxes);
  if (!l.boxes.empty()) boxes = l.boxes;
  if (l.all_dead) hs.dead.assign(n, 1);
  const std::vector<Box> plain = boxes;
  BuildOptions opt;
  opt.force_tree = l.force_tree;
  SceneAccel A;
  rc = build_accel(hs, std::move(boxes), kTol, 4, opt, A, err);
  if (rc != ODW_OK) {
    HOLD(l.may_refuse && rc == ODW_ERR_UNSUPPORTED && !err.empty(), "build refused (%d): %s", rc, err.c_str());
    HOLD(A.nodes.empty() && A.order.empty(), "a refused build left %zu nodes", A.nodes.size());
    printf("%-20s %5d primitives: refused, \"%s\"\n", l.name.c_str(), n, err.c_str());
    return;
  }
  HOLD(!A.nodes.empty(), "no tree");
  if (A.nodes.empty()) return;
  HOLD(bvh_order_fits(A.order.size()), "%zu entries in the leaf order", A.order.size());

  Walk w(l, A, plain);
  const bool wrapper = WideBvh::far_box(A.nodes[0].lo1);
  HOLD(wrapper == l.wrapper, "wrapper root: %d, expected %d", (int)wrapper, (int)l.wrapper);
  if (wrapper) {
    ++w.node_seen[0];
    w.child(0, 0, 0);                                  // (the builder met this leaf at depth 0)
    check_far_child(l, A.nodes[0]);
  } else {
    w.node(0, 0);
  }
  // ---- coverage
  for (size_t k = 0; k < A.nodes.size(); ++k) HOLD(w.node_seen[k] == 1, "node %zu is reached %d times from node 0", k, w.node_seen[k]);
  for (size_t e = 0; e < A.order.size(); ++e) HOLD(w.entry_seen[e] == 1, "order[%zu] lies in %d leaves", e, w.entry_seen[e]);
  int live = 0;
  for (int p = 0; p < n; ++p) {
    const int expected = l.all_dead ? (p == 0) : !hs.dead[p];
    live += expected;
    HOLD(w.prim_seen[p] == expected, "primitive %d lies in %d leaves, expected %d", p, w.prim_seen[p], expected);
  }
  HOLD((int)A.order.size() == live, "%zu entries for %d live primitives", A.order.size(), live);
  // ---- depth
  HOLD(A.max_depth == w.height, "max_depth %d, the tree is %d levels high", A.max_depth, w.height);
  HOLD(A.max_depth + 2 <= ODW_BVH_STACK, "max_depth %d + 2 beyond the stack of %d", A.max_depth, ODW_BVH_STACK);
  HOLD(w.height >= l.min_depth, "%d levels, the layout has to reach %d", w.height, l.min_depth);
  // ---- the eight-wide tree
  HOLD((A.kind() == kAccelWide) == (l.wide != 0), "eight-wide tree: kind %d, expected %d", (int)A.kind(), l.wide);
  int wide_depth = -1, wide_most = 0;
  if (A.kind() == kAccelWide) {
    std::vector<int> prim_solid(n);
    for (int p = 0; p < n; ++p) prim_solid[p] = hs.prim_i32[4 * (size_t)p + 2] >> ODW_SOLID_SHIFT;
    for (int p = 0; p < n; ++p) HOLD(prim_solid[p] == l.solid[p], "primitive %d: solid %d in the flag word, %d given", p, prim_solid[p], l.solid[p]);
    WideWalk ww{l, A, w.grown, prim_solid, {}, {}, {}};
    ww.rec_seen.assign(A.leaf_recs.size() / ODW_LEAF_WORDS, 0);
    ww.prim_seen.assign(n, 0);
    ww.node_seen.assign(A.wide_nodes.size() / kWideWords, 0);
    ww.node(0, 0);
    for (size_t k = 0; k < ww.node_seen.size(); ++k) HOLD(ww.node_seen[k] == 1, "wide node %zu is reached %d times", k, ww.node_seen[k]);
    for (int p = 0; p < n; ++p) HOLD(ww.prim_seen[p] == !hs.dead[p], "facet %d lies in %d leaf records", p, ww.prim_seen[p]);
    for (size_t k = 0; k < ww.rec_seen.size(); ++k) HOLD(ww.rec_seen[k] == 1, "leaf record %zu belongs to %d slots", k, ww.rec_seen[k]);
    HOLD(ww.depth <= kWideMaxDepth, "eight-wide tree %d levels deep, kWideMaxDepth is %d", ww.depth, kWideMaxDepth);
    wide_depth = ww.depth; wide_most = ww.most;
  }
  printf("%-20s %5d primitives: %5zu nodes, %5d leaves (at most %d primitives), depth %2d of %d", l.name.c_str(), n, A.nodes.size(), w.leaves,
         w.largest_leaf, w.height, ODW_BVH_STACK - 2);
  if (wide_depth >= 0) printf(", eight-wide: %zu nodes, depth %d, at most %d facets in a slot", A.wide_nodes.size() / kWideWords, wide_depth, wide_most);
  printf("%s\n", wrapper ? ", wrapper root" : "");
}

}  // namespace

int main() {
  const double zero[3] = {0.0, 0.0, 0.0}, T[3] = {3000.0, -7000.0, 11000.0};
  const Layout layouts[] = {lattice(false, zero, "lattice"), lattice(true, zero, "mixed lattice"), cloud(), staggered(), big(), seventy(), line(),
                            lattice(false, T, "moved lattice"), coincident("80 coincident", 80), coincident("1000 coincident", 1000), chain(),
                            random_boxes(), two_axes(), single(), none_alive(), cubes(), huge_extents()};
  for (const Layout& l : layouts) check(l);
  // the guard of build_accel: the leaf order stays below 1 << 24 entries
  if (!bvh_order_fits(((size_t)1 << 24) - 1) || bvh_order_fits((size_t)1 << 24) || !bvh_order_fits(0)) {
    fprintf(stderr, "bvh_order_fits: the limit is not 1 << 24\n");
    ++bad;
  }
  printf("%zu layouts checked, %d mismatches\n", sizeof layouts / sizeof layouts[0], bad);
  return bad ? 1 : 0;
}
