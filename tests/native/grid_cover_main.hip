// grid_cover_main.hip -- what the walk of odw_grid.hip relies on in the tables build_grid (csrc/odw_build.h) hands it,
// checked by brute force, under AddressSanitizer + UndefinedBehaviorSanitizer.
//
// A program of its own (tests/test_native_grid_cover.py compiles and runs it; no GPU, no Python, nothing preloaded).
// It builds the grids of the layouts of tests/grid_cases.py (the random ones from a generator of its own: the same
// character, not the same numbers), of a line of 300 small spheres (more than 128 slabs on one axis: the even division,
// whose planes cut through boxes) and of a cloud crowded past 255 items in a cell (which build_grid refuses), and holds:
//   the planes increase strictly and enclose every box;
//   every (cell, primitive) pair whose closed box touches the closed cell is listed, exactly once, and no other;
//   counts and offsets of the cell words agree with the lists;
//   the sphere records repeat the primitive's centre, radius, group, solid and flag word;
//   lds_bytes and in_lds follow the kernel's own offset arithmetic.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "odw_kernels.hip"
#include "odw_grid.hip"
#include "odw_mesh.hip"
#include "odw_build.h"

namespace {

constexpr double kTol = 1e-6;

struct Solid { int type; double c[3], h[3]; };     // centre and half-widths (sphere: h[0] the radius)

struct Layout {
  const char* name;
  std::vector<Solid> solids;
  bool grid;                 // build_grid takes it
  int spheres, in_lds;       // expected where it does
  int nx_expected;           // > 0: cells along x
};

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

Solid sphere(double x, double y, double z, double r) { return {ODW_PRIM_SPHERE, {x, y, z}, {r, r, r}}; }

Layout lattice(bool mixed) {
  Layout l{mixed ? "mixed lattice" : "lattice", {}, true, mixed ? 0 : 1, 1, 5};
  int i = 0;
  for (int x = 0; x < 5; ++x)
    for (int y = 0; y < 4; ++y)
      for (int z = 0; z < 4; ++z, ++i) {
        Solid s = sphere(10.0 * x, 10.0 * y, 10.0 * z, 2.0);
        if (mixed && i % 3 == 1) s.type = ODW_PRIM_BOX;
        l.solids.push_back(s);
      }
  return l;
}

Layout cloud() {
  Layout l{"cloud", {}, true, 1, 1, 0};
  Rng g{3};
  for (int i = 0; i < 90; ++i) {
    const double x = g.next(-30, 30), y = g.next(-30, 30), z = g.next(-30, 30);
    l.solids.push_back(sphere(x, y, z, g.next(1, 9)));
  }
  return l;
}

Layout staggered() {
  Layout l{"staggered", {}, true, 1, 1, 5};
  for (int i = 0; i < 5; ++i)
    for (int j = 0; j < 4; ++j)
      for (int k = 0; k < 4; ++k) l.solids.push_back(sphere(6.0 * i + 3 * (j % 2), 6.0 * j + 3 * (k % 2), 6.0 * k + 3 * (i % 2), 2.5));
  return l;
}

Layout big() {
  Layout l{"13^3 lattice", {}, true, 1, 0, 13};
  for (int i = 0; i < 13; ++i)
    for (int j = 0; j < 13; ++j)
      for (int k = 0; k < 13; ++k) l.solids.push_back(sphere(10.0 * i, 10.0 * j, 10.0 * k, 2 + 0.001 * (i % 7)));
  return l;
}

Layout seventy() {
  Layout l{"seventy", {}, true, 0, 0, 0};
  Rng g{5};
  const int kinds[3] = {ODW_PRIM_SPHERE, ODW_PRIM_BOX, ODW_PRIM_ELLIPSOID};
  for (int i = 0; i < 70; ++i) {
    Solid s{kinds[i % 3], {g.next(-200, 200), g.next(-200, 200), g.next(-200, 200)}, {g.next(1, 3), g.next(1, 3), g.next(1, 3)}};
    if (s.type == ODW_PRIM_SPHERE) s.h[1] = s.h[2] = s.h[0];
    l.solids.push_back(s);
  }
  return l;
}

Layout line() {
  Layout l{"line of 300", {}, true, 1, 1, 128};
  for (int i = 0; i < 300; ++i) l.solids.push_back(sphere(1.0 * i, 0.0, 0.0, 0.25));
  return l;
}

Layout crowded() {
  Layout l{"crowded", {}, false, 0, 0, 0};
  Rng g{7};
  for (int i = 0; i < 300; ++i) l.solids.push_back(sphere(g.next(-0.5, 0.5), g.next(-0.5, 0.5), g.next(-0.5, 0.5), g.next(2, 6)));
  return l;
}

int bad = 0;
#define HOLD(cond, ...) do { if (!(cond)) { if (++bad < 40) { fprintf(stderr, "%s: ", l.name); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } } while (0)

void check(const Layout& l) {
  const int n = (int)l.solids.size();
  std::vector<int32_t> type(n), group(n), solid(n), flags(n), cond_off(n + 1, 0);
  std::vector<double> xform, params;
  for (int p = 0; p < n; ++p) {
    const Solid& s = l.solids[p];
    type[p] = s.type; group[p] = p % 2; solid[p] = p;
    flags[p] = ODW_FLAG_CONVEX | ((s.type == ODW_PRIM_BOX ? 0x3f : 1) << ODW_FACEMASK_SHIFT);
    // local = global - origin: a box's frame sits at its lower corner, the others' at their centre
    for (int r = 0; r < 3; ++r) {
      for (int k = 0; k < 3; ++k) xform.push_back(r == k ? 1.0 : 0.0);
      xform.push_back(-(s.type == ODW_PRIM_BOX ? s.c[r] - s.h[r] : s.c[r]));
    }
    if (s.type == ODW_PRIM_BOX) for (double v : {2 * s.h[0], 2 * s.h[1], 2 * s.h[2], 0.0}) params.push_back(v);
    else if (s.type == ODW_PRIM_SPHERE) for (double v : {s.h[0], 0.0, 0.0, 0.0}) params.push_back(v);
    else for (double v : {s.h[0], s.h[1], s.h[2], 0.0}) params.push_back(v);
  }
  const int32_t gtype[2] = {ODW_OPT_VACUUM, ODW_OPT_VACUUM}, grecord[2] = {1, 1};
  const double gior[2] = {1.0, 1.0}, grefl[2] = {0.0, 0.0}, gabs[2] = {INFINITY, INFINITY};
  odw_scene_desc d;
  std::memset(&d, 0, sizeof d);
  d.n_prims = n;
  d.prim_type = type.data(); d.prim_group = group.data(); d.prim_solid = solid.data(); d.prim_flags = flags.data();
  d.prim_xform = xform.data(); d.prim_params = params.data(); d.prim_cond_off = cond_off.data();
  d.n_groups = 2;
  d.group_type = gtype; d.group_ior = gior; d.group_refl = grefl; d.group_abslen = gabs; d.group_record = grecord;

  HostScene hs;
  std::string err;
  int rc = scene_host_tables(&d, hs, err);
  HOLD(rc == ODW_OK, "scene refused (%d): %s", rc, err.c_str());
  if (rc) return;
  std::vector<Box> boxes;
  compute_boxes(hs, kTol, boxes);
  const std::vector<Box> bx = boxes;
  SceneAccel A;
  rc = build_accel(hs, std::move(boxes), kTol, 4, BuildOptions(), A, err);
  HOLD(rc == ODW_OK, "build refused (%d): %s", rc, err.c_str());
  if (rc) return;
  // the boxes hold the solids with the tolerance's slack
  for (int p = 0; p < n; ++p)
    for (int a = 0; a < 3; ++a)
      HOLD(bx[p].lo[a] <= l.solids[p].c[a] - l.solids[p].h[a] - kTol && bx[p].hi[a] >= l.solids[p].c[a] + l.solids[p].h[a] + kTol &&
           bx[p].hi[a] - bx[p].lo[a] < 2 * l.solids[p].h[a] + 1e-3, "box of primitive %d, axis %d", p, a);
  const DeviceGrid& G = A.grid;
  if (!l.grid) {
    // every box holds the origin: whatever the planes, one cell lists all 300 -- more than a cell word counts
    for (int p = 0; p < n; ++p)
      for (int a = 0; a < 3; ++a) HOLD(bx[p].lo[a] < 0 && bx[p].hi[a] > 0, "box %d does not hold the origin", p);
    HOLD(n > (int)kGridMaxCellItems && G.nx == 0 && A.kind() == kAccelTree && !A.nodes.empty(), "a crowded scene got a grid (nx %d)", G.nx);
    printf("%-14s %4d primitives: no grid, %zu tree nodes\n", l.name, n, A.nodes.size());
    return;
  }
  HOLD(A.kind() == kAccelGrid && G.nx > 0 && G.ny > 0 && G.nz > 0, "no grid");
  if (A.kind() != kAccelGrid) return;
  const int dim[3] = {G.nx, G.ny, G.nz};
  HOLD(dim[0] <= kGridMaxAxis && dim[1] <= kGridMaxAxis && dim[2] <= kGridMaxAxis, "more than 128 cells on an axis");
  HOLD(l.nx_expected == 0 || G.nx == l.nx_expected, "nx = %d, expected %d", G.nx, l.nx_expected);
  HOLD((int)A.planes.size() == dim[0] + dim[1] + dim[2] + 3, "%zu planes", A.planes.size());
  const double* pl[3] = {A.planes.data(), A.planes.data() + dim[0] + 1, A.planes.data() + dim[0] + dim[1] + 2};
  // ---- planes: strictly increasing, around every box
  int cut_through = 0;
  for (int a = 0; a < 3; ++a) {
    for (int k = 0; k < dim[a]; ++k) HOLD(pl[a][k] < pl[a][k + 1], "axis %d: plane %d does not lie below the next", a, k);
    for (int p = 0; p < n; ++p) {
      HOLD(pl[a][0] < bx[p].lo[a] && bx[p].hi[a] < pl[a][dim[a]], "axis %d: box %d is not enclosed", a, p);
      for (int k = 1; k < dim[a]; ++k) cut_through += bx[p].lo[a] < pl[a][k] && pl[a][k] < bx[p].hi[a];
    }
  }
  // ---- cell words and lists
  const size_t ncell = (size_t)dim[0] * dim[1] * dim[2];
  HOLD(A.cells.size() == ncell, "%zu cell words for %zu cells", A.cells.size(), ncell);
  size_t total = 0;
  for (size_t c = 0; c < ncell; ++c) {
    HOLD((A.cells[c] & 0xffffffu) == total, "cell %zu: offset %u, expected %zu", c, A.cells[c] & 0xffffffu, total);
    total += A.cells[c] >> 24;
  }
  HOLD((size_t)G.n_items == total, "n_items %d, the counts add up to %zu", G.n_items, total);
  const size_t listed = G.spheres ? A.sphere_recs.size() / 6 : A.item_prim.size();
  HOLD(listed >= total && listed <= total + 1, "%zu items behind %zu listed", listed, total);
  auto item = [&](size_t k) -> int {
    if (!G.spheres) return (int)A.item_prim[k];
    uint64_t bits;
    std::memcpy(&bits, &A.sphere_recs[6 * k + 4], sizeof bits);
    return (int)(uint32_t)bits;
  };
  // ---- every pair whose closed box touches the closed cell, once; no other
  std::vector<int> seen(n);
  size_t pairs = 0, most = 0;
  for (int z = 0; z < dim[2]; ++z)
    for (int y = 0; y < dim[1]; ++y)
      for (int x = 0; x < dim[0]; ++x) {
        const size_t c = x + (size_t)dim[0] * (y + (size_t)dim[1] * z);
        const uint32_t first = A.cells[c] & 0xffffffu, count = A.cells[c] >> 24;
        most = std::max<size_t>(most, count);
        std::fill(seen.begin(), seen.end(), 0);
        for (uint32_t k = 0; k < count && first + k < listed; ++k) {
          const int p = item(first + k);
          HOLD(p >= 0 && p < n, "cell %zu lists primitive %d", c, p);
          if (p >= 0 && p < n) ++seen[p];
        }
        const int at[3] = {x, y, z};
        for (int p = 0; p < n; ++p) {
          bool touches = true;
          for (int a = 0; a < 3; ++a) touches = touches && bx[p].lo[a] <= pl[a][at[a] + 1] && bx[p].hi[a] >= pl[a][at[a]];
          HOLD(seen[p] == (touches ? 1 : 0), "cell (%d, %d, %d) lists primitive %d %d times, its box %s it", x, y, z, p, seen[p],
               touches ? "touches" : "does not touch");
          pairs += touches;
        }
      }
  HOLD(pairs == total, "%zu pairs touch, %zu are listed", pairs, total);
  // ---- sphere records
  HOLD(G.spheres == l.spheres, "spheres %d, expected %d", G.spheres, l.spheres);
  if (G.spheres)
    for (size_t k = 0; k < total; ++k) {
      const double* o = &A.sphere_recs[6 * k];
      uint64_t bits, word;
      std::memcpy(&bits, &o[4], sizeof bits);
      std::memcpy(&word, &o[5], sizeof word);
      const int p = (int)(uint32_t)bits;
      if (p < 0 || p >= n) continue;
      const Solid& s = l.solids[p];
      HOLD(o[0] == s.c[0] && o[1] == s.c[1] && o[2] == s.c[2] && o[3] == s.h[0], "record %zu: centre or radius of primitive %d", k, p);
      HOLD((int)((bits >> 32) & 0xff) == group[p] && (int)(bits >> 40) == solid[p], "record %zu: group or solid of primitive %d", k, p);
      HOLD((uint32_t)word == (uint32_t)hs.prim_i32[4 * (size_t)p + 2] && (int)((uint32_t)word >> ODW_SOLID_SHIFT) == solid[p] &&
           ((uint32_t)word & 0xff) == (uint32_t)(ODW_FLAG_CONVEX | (hs.prim_i32[4 * (size_t)p + 2] & ODW_FLAG_ISOLATED)),
           "record %zu: flag word %08x of primitive %d", k, (unsigned)word, p);
    }
  // ---- the block's LDS, by the kernel's offsets (odw_grid_kernel)
  {
    const int nb = dim[0] + dim[1] + dim[2] + 3;
    const int word_off = 2 * nb;
    const int ring_off = (word_off + ODW_GRID_WAVES * ODW_GRID_WAVE_WORDS + 1) / 2;
    const int cell_off = 2 * (ring_off + ODW_GRID_WAVES * ODW_GRID_RING_DOUBLES);
    const size_t item_off = (((size_t)cell_off + ncell + 3) & ~(size_t)3) / 2;
    const size_t n_words = G.spheres ? (size_t)G.n_items * 6 : ((size_t)G.n_items + 1) / 2;
    const size_t staged = (item_off + n_words) * sizeof(double), fixed = (size_t)cell_off * sizeof(uint32_t);
    const int in_lds = staged + 16 <= 144 * 1024 ? 1 : 0;
    HOLD(G.in_lds == in_lds && G.in_lds == l.in_lds, "in_lds %d, by the kernel's offsets %d, expected %d", G.in_lds, in_lds, l.in_lds);
    HOLD(G.lds_bytes == (in_lds ? staged : fixed) + 16, "lds_bytes %u, by the kernel's offsets %zu", G.lds_bytes, (in_lds ? staged : fixed) + 16);
    HOLD(G.lds_bytes <= 155 * 1024, "lds_bytes %u beyond what a launch may ask for", G.lds_bytes);
    // what the copy loops of the kernel read: cells [0, ncell), items [0, n_words) doubles
    HOLD(A.item_bytes() >= n_words * sizeof(double), "the kernel stages %zu bytes of items, the table has %zu", n_words * sizeof(double), A.item_bytes());
  }
  if (!std::strcmp(l.name, "line of 300")) HOLD(cut_through > 0, "the even division cuts through no box");
  printf("%-14s %4d primitives: %3d x %3d x %3d cells, %6zu items (at most %3zu in a cell), %s, %s, %u bytes of LDS, %d planes through boxes\n",
         l.name, n, dim[0], dim[1], dim[2], total, most, G.spheres ? "sphere records" : "primitive numbers", G.in_lds ? "in LDS" : "global",
         G.lds_bytes, cut_through);
}

}  // namespace

int main() {
  const Layout layouts[] = {lattice(false), lattice(true), cloud(), staggered(), big(), seventy(), line(), crowded()};
  for (const Layout& l : layouts) check(l);
  printf("%zu layouts checked, %d mismatches\n", sizeof layouts / sizeof layouts[0], bad);
  return bad ? 1 : 0;
}
