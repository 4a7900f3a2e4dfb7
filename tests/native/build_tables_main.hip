// build_tables_main.hip -- the host builders of csrc/odw_build.h under AddressSanitizer + UndefinedBehaviorSanitizer.
//
// A program of its own (tests/test_native_build_tables.py compiles and runs it; no GPU, no Python, nothing preloaded).
// It makes descriptors that reach every branch of scene_host_tables, compute_boxes and build_accel -- flat scenes, the
// grid with sphere records and with primitive numbers, scenes the grid refuses, the binary tree with a wrapped root, the
// eight-wide tree with and without cones -- and holds the structure, the sizes and a hash of every table against
// constants; then descriptors the library refuses.  `--print` writes the table of constants instead of comparing.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "odw_kernels.hip"
#include "odw_grid.hip"
#include "odw_mesh.hip"
#include "odw_build.h"

namespace {

// ---- scenes ---------------------------------------------------------------------------------------------------------
struct Scene {
  std::vector<int32_t> type, group, solid, flags, cond_off{0}, cond_prim, cond_inside, tri_edges;
  std::vector<double> xform, params, tri_normals;
  bool facets = false;                       // hand tri_edges / tri_normals to the library
  // groups: 0 a lens, 1 a recording absorber
  int32_t gtype[2] = {ODW_OPT_LENS, ODW_OPT_ABSORBER}, grecord[2] = {0, 1};
  double gior[2] = {1.5, 1.0}, grefl[2] = {0.0, 0.0}, gabs[2] = {INFINITY, INFINITY};

  // an analytic primitive whose frame is rotated by `tilt` about x and centred at c; conds: {primitive, cond_inside}
  int add(int t, int g, int s, int fl, int facemask, const double c[3], double p0, double p1, double p2,
          std::vector<std::pair<int, int>> conds = {}, double tilt = 0.0) {
    const double cs = std::cos(tilt), sn = std::sin(tilt);
    const double R[9] = {1, 0, 0, 0, cs, sn, 0, -sn, cs};
    for (int r = 0; r < 3; ++r) {
      for (int k = 0; k < 3; ++k) xform.push_back(R[3 * r + k]);
      xform.push_back(-(R[3 * r] * c[0] + R[3 * r + 1] * c[1] + R[3 * r + 2] * c[2]));   // local = R (global - c)
    }
    return row(t, g, s, fl, facemask, p0, p1, p2, conds);
  }
  // a facet v0, v1, v2 (counter-clockwise from outside), its vertex normals and which of its edges are face edges
  int facet(int g, int s, int fl, const double* v0, const double* v1, const double* v2, const double* n3, int edges) {
    for (const double* v : {v0, v1, v2}) xform.insert(xform.end(), v, v + 3);
    xform.insert(xform.end(), 3, 0.0);
    const int p = row(ODW_PRIM_TRIANGLE, g, s, fl, 1, 0, 0, 0, {});
    std::copy(n3, n3 + 9, tri_normals.begin() + 9 * (size_t)p);
    tri_edges[p] = edges;
    return p;
  }
  int row(int t, int g, int s, int fl, int facemask, double p0, double p1, double p2, const std::vector<std::pair<int, int>>& conds) {
    type.push_back(t); group.push_back(g); solid.push_back(s); flags.push_back(fl | (facemask << ODW_FACEMASK_SHIFT));
    for (double v : {p0, p1, p2, 0.0}) params.push_back(v);
    for (const auto& c : conds) { cond_prim.push_back(c.first); cond_inside.push_back(c.second); }
    cond_off.push_back((int32_t)cond_prim.size());
    tri_edges.push_back(7);
    tri_normals.insert(tri_normals.end(), 9, 0.0);
    return (int)type.size() - 1;
  }
  odw_scene_desc desc() const {
    odw_scene_desc d;
    std::memset(&d, 0, sizeof d);
    d.n_prims = (int32_t)type.size();
    d.prim_type = type.data(); d.prim_group = group.data(); d.prim_solid = solid.data(); d.prim_flags = flags.data();
    d.prim_xform = xform.data(); d.prim_params = params.data(); d.prim_cond_off = cond_off.data();
    d.n_conds = (int32_t)cond_prim.size();
    d.cond_prim = cond_prim.data(); d.cond_inside = cond_inside.data();
    d.n_groups = 2;
    d.group_type = gtype; d.group_ior = gior; d.group_refl = grefl; d.group_abslen = gabs; d.group_record = grecord;
    if (facets) { d.tri_normals = tri_normals.data(); d.tri_edges = tri_edges.data(); }
    return d;
  }
};

constexpr int kInside = 1, kOpens = 2;     // cond_inside bits (odw_trace.h)

// boxes cut by operands, a union over clauses, a dead operand, isolated and neighbouring solids, every analytic
// kind but the paraboloid (which the flat kernels do not take)
Scene flat_scene() {
  Scene s;
  const double a[3] = {0, 0, -4}, b[3] = {0, 0, 4}, box[3] = {20, 0, 0}, op[3] = {21, 2, 2}, in[3] = {23, 2, 2};
  const double cyl[3] = {25.03, 2, 0}, cone[3] = {0, 20, 0}, torus[3] = {0, -20, 0};
  s.add(ODW_PRIM_SPHERE, 0, 0, ODW_FLAG_CONVEX, 1, a, 5, 0, 0, {{1, kInside}});                   // a lens: the Common of two
  s.add(ODW_PRIM_SPHERE, 0, 0, ODW_FLAG_CONVEX, 1, b, 5, 0, 0, {{0, kInside}});                   // spheres
  s.add(ODW_PRIM_BOX, 1, 1, 0, 0x3f, box, 4, 4, 4, {{3, kInside | kOpens}, {4, 0}, {4, kInside | kOpens}});   // two clauses
  s.add(ODW_PRIM_SPHERE, 1, 1, 0, 0, op, 2, 0, 0);                                                // an operand without a face: dead
  s.add(ODW_PRIM_SPHERE, 1, 1, 0, 1, in, 1.5, 0, 0, {{2, kInside}});
  s.add(ODW_PRIM_CYLINDER, 1, 2, ODW_FLAG_CONVEX, 7, cyl, 1, 3, 0);                               // within 4 distTol of solid 1
  s.add(ODW_PRIM_CONE, 1, 3, ODW_FLAG_CONVEX, 7, cone, 1, 0.5, 2);
  s.add(ODW_PRIM_TORUS, 0, 4, ODW_FLAG_FLIP_NORMAL, 1, torus, 3, 0.5, 0, {}, 0.5);
  return s;
}

Scene sphere_array(bool with_box) {
  Scene s;
  for (int z = 0; z < 3; ++z)
    for (int y = 0; y < 5; ++y)
      for (int x = 0; x < 5; ++x) {
        const double c[3] = {3.0 * x, 3.0 * y, 3.0 * z};
        s.add(ODW_PRIM_SPHERE, 0, (int)s.type.size(), ODW_FLAG_CONVEX, 1, c, 1, 0, 0);
      }
  const double c[3] = {20, 0, 0};
  if (with_box) s.add(ODW_PRIM_BOX, 1, 75, ODW_FLAG_CONVEX, 0x3f, c, 2, 2, 2);
  return s;
}

Scene mixed_scene(bool with_paraboloid) {
  Scene s;
  for (int k = 0; k < 12; ++k) {
    const double c[3] = {5.0 * (k % 4), 5.0 * (k / 4), 0.25 * k};
    const int kinds[4] = {ODW_PRIM_BOX, ODW_PRIM_SPHERE, ODW_PRIM_CYLINDER, ODW_PRIM_CONE};
    const int t = kinds[k % 4];
    s.add(t, k % 2, k, ODW_FLAG_CONVEX, t == ODW_PRIM_BOX ? 0x3f : (t == ODW_PRIM_SPHERE ? 1 : 7), c, 1, t == ODW_PRIM_CONE ? 0.5 : 2, 2, {}, 0.1 * k);
  }
  const double c[3] = {0, 20, 0};
  if (with_paraboloid) s.add(ODW_PRIM_PARABOLOID, 0, 12, 0, 5, c, 2, 3, 0);
  return s;
}

Scene concentric_spheres() {
  Scene s;
  const double c[3] = {0, 0, 0};
  for (int k = 0; k < 300; ++k) s.add(ODW_PRIM_SPHERE, k % 2, k, ODW_FLAG_CONVEX, 1, c, 1.0 + 0.01 * k, 0, 0);
  return s;
}

// the two facets of a rectangle: one box, one leaf, a root wrapped around it
Scene one_leaf_scene() {
  Scene s;
  s.facets = true;
  const double v[4][3] = {{0, 0, 1}, {2, 0, 1}, {2, 3, 1}, {0, 3, 1}};
  const double n3[9] = {0, 0, 1, 0, 0, 1, 0, 0, 1};
  s.facet(1, 0, 0, v[0], v[1], v[2], n3, 6);
  s.facet(1, 0, 0, v[0], v[2], v[3], n3, 5);
  return s;
}

// a UV-sphere of 8 x 6 facets around the origin (a strictly convex polyhedron, one tessellated face) beside a box
Scene facet_scene() {
  Scene s;
  s.facets = true;
  constexpr int kSeg = 8, kRing = 4;
  const double R = 10.0, pi = 3.14159265358979323846;
  auto vert = [&](int ring, int seg, double* v, double* nrm) {
    const double th = pi * ring / kRing, ph = 2.0 * pi * (seg % kSeg) / kSeg;
    nrm[0] = std::sin(th) * std::cos(ph); nrm[1] = std::sin(th) * std::sin(ph); nrm[2] = std::cos(th);
    if (ring == 0) { nrm[0] = nrm[1] = 0; nrm[2] = 1; }
    if (ring == kRing) { nrm[0] = nrm[1] = 0; nrm[2] = -1; }
    for (int a = 0; a < 3; ++a) v[a] = R * nrm[a];
  };
  const int fl = ODW_FLAG_CONVEX | ODW_FLAG_STRICTLY_CONVEX;
  for (int r = 0; r < kRing; ++r)
    for (int g = 0; g < kSeg; ++g) {
      double v[4][3], n[4][3];                   // upper left, upper right, lower left, lower right (seen from outside)
      vert(r, g, v[0], n[0]); vert(r, g + 1, v[1], n[1]); vert(r + 1, g, v[2], n[2]); vert(r + 1, g + 1, v[3], n[3]);
      auto tri = [&](int i, int j, int k) {
        double n3[9];
        for (int a = 0; a < 3; ++a) { n3[a] = n[i][a]; n3[3 + a] = n[j][a]; n3[6 + a] = n[k][a]; }
        s.facet(0, 0, fl, v[i], v[j], v[k], n3, 0);
      };
      if (r > 0) tri(0, 2, 1);                   // (the upper edge of the first band is the pole)
      if (r < kRing - 1) tri(1, 2, 3);
    }
  const double c[3] = {15, -1, -1};
  s.add(ODW_PRIM_BOX, 1, 1, ODW_FLAG_CONVEX, 0x3f, c, 2, 2, 2);
  return s;
}

// ---- what a run is held against -------------------------------------------------------------------------------------
// FNV-1a over the bytes of: headers, dead flags, flag words (prim_i32), planes, cells, items, nodes, order, wide words,
// leaf records.  The constants are a record of what the builders produce (`--print` writes them): the kernels read
// these bytes, so a hash that differs is a change of results or of speed to be accounted for, not a constant to refresh.
struct Expect {
  const char* name;
  int structure;
  uint64_t sizes[6];       // primitives, tree nodes, grid cells, grid items, bytes of dynamic LDS of a grid block, dead primitives
  int spheres, in_lds;
  uint64_t hash[10];
};

uint64_t fnv1a(const void* p, size_t bytes, uint64_t h = 1469598103934665603ull) {
  const unsigned char* c = (const unsigned char*)p;
  for (size_t i = 0; i < bytes; ++i) { h ^= c[i]; h *= 1099511628211ull; }
  return h;
}

struct Run { const char* name; Scene scene; double dist_tol; int flat_limit; bool mesh_kernel, cones, cone_stats; };

const Expect kExpected[] = {
    {"flat", 0, {8ull, 0ull, 0ull, 0ull, 0ull, 1ull}, 0, 0,
     {0x4b0d65f3268371efull, 0x3b4f2a54323ee780ull, 0xd4ea0bd5052ee234ull, 0x14650fb0739d0383ull, 0x14650fb0739d0383ull,
      0x14650fb0739d0383ull, 0x14650fb0739d0383ull, 0x14650fb0739d0383ull, 0x14650fb0739d0383ull, 0x14650fb0739d0383ull}},
    {"grid_spheres", 1, {75ull, 41ull, 75ull, 75ull, 63440ull, 0ull}, 1, 1,
     {0xf1ae128479778d28ull, 0xd2348a8e37364da1ull, 0xdcb28f4a2de1dd5cull, 0xb8bbf3079483f834ull, 0xe6a91f4c75ae1fcfull,
      0x82772fe3ddd02f9aull, 0x63bf9e5dcab0b0beull, 0x0dbb24f12f3be1f8ull, 0x14650fb0739d0383ull, 0x14650fb0739d0383ull}},
    {"grid_generic", 1, {76ull, 42ull, 48ull, 76ull, 60032ull, 0ull}, 0, 1,
     {0xf3af3b00775c02f1ull, 0x659510a7d145e893ull, 0x02818506dea09ce5ull, 0x8c6699f0fd0e3887ull, 0xf0b841317d3e996eull,
      0x6f8cb430a5967f63ull, 0xe920115fd61472b7ull, 0xb4e5ad7600286d13ull, 0x14650fb0739d0383ull, 0x14650fb0739d0383ull}},
    {"mixed_flat", 0, {12ull, 0ull, 0ull, 0ull, 0ull, 0ull}, 0, 0,
     {0x37b6f54eec470b7eull, 0xc327e8bf29be1593ull, 0x01080043cf17d8adull, 0x14650fb0739d0383ull, 0x14650fb0739d0383ull,
      0x14650fb0739d0383ull, 0x14650fb0739d0383ull, 0x14650fb0739d0383ull, 0x14650fb0739d0383ull, 0x14650fb0739d0383ull}},
    {"mixed_limit4", 1, {12ull, 11ull, 12ull, 12ull, 59600ull, 0ull}, 0, 1,
     {0x37b6f54eec470b7eull, 0xc327e8bf29be1593ull, 0x01080043cf17d8adull, 0x856b67d9df2cac18ull, 0x00814daf00d082b7ull,
      0x419cc31e0d461583ull, 0x6ad45938bfa37fdaull, 0x31eafecfb7d9c283ull, 0x14650fb0739d0383ull, 0x14650fb0739d0383ull}},
    {"mixed_paraboloid", 1, {13ull, 12ull, 12ull, 13ull, 59608ull, 0ull}, 0, 1,
     {0xcdc90af07d0c663full, 0x5ae60fd3edfea8c9ull, 0x13039ce82337fcc4ull, 0x633f5b1d301ae56full, 0xd08e0d46ae3b4d8full,
      0xdd0de302aec51d6full, 0xde0eeb78ae386303ull, 0x9c4db103b1efb2ffull, 0x14650fb0739d0383ull, 0x14650fb0739d0383ull}},
    {"tree_only", 2, {300ull, 59ull, 0ull, 0ull, 0ull, 0ull}, 0, 0,
     {0x6e2a9719416ee7f7ull, 0xc4080cd4d9a6eb13ull, 0xf66fe19386a9de53ull, 0x14650fb0739d0383ull, 0x14650fb0739d0383ull,
      0x14650fb0739d0383ull, 0x16f5f1dad3e0aa05ull, 0xe14228008b3c75d7ull, 0x14650fb0739d0383ull, 0x14650fb0739d0383ull}},
    {"one_leaf", 2, {2ull, 1ull, 0ull, 0ull, 0ull, 0ull}, 0, 0,
     {0xb6dbd04013e6c1ebull, 0x9a691300c548b8fbull, 0x495e01c9e47c7343ull, 0x14650fb0739d0383ull, 0x14650fb0739d0383ull,
      0x14650fb0739d0383ull, 0x807b2c8acb50c51aull, 0xa803617659589552ull, 0x14650fb0739d0383ull, 0x14650fb0739d0383ull}},
    {"wide_tol1e-2", 3, {49ull, 24ull, 0ull, 0ull, 0ull, 0ull}, 0, 0,
     {0xc06241d32a36f280ull, 0xf7dd0a8e4de56259ull, 0x33680c99d65e2cd8ull, 0x14650fb0739d0383ull, 0x14650fb0739d0383ull,
      0x14650fb0739d0383ull, 0x05e562996f19ed96ull, 0x6ad610726c07a413ull, 0x5c334b1953a8ac96ull, 0x359e25c4b3634262ull}},
    {"wide_tol1e-6", 3, {49ull, 24ull, 0ull, 0ull, 0ull, 0ull}, 0, 0,
     {0x4dab04c8f6e1e0feull, 0xf7dd0a8e4de56259ull, 0x33680c99d65e2cd8ull, 0x14650fb0739d0383ull, 0x14650fb0739d0383ull,
      0x14650fb0739d0383ull, 0xa429d2a23afb8173ull, 0x20c83a6a0655ca23ull, 0x84e3cf23a52218adull, 0x81e152fed8298b0full}},
    {"wide_no_cones", 3, {49ull, 24ull, 0ull, 0ull, 0ull, 0ull}, 0, 0,
     {0xc06241d32a36f280ull, 0xf7dd0a8e4de56259ull, 0x33680c99d65e2cd8ull, 0x14650fb0739d0383ull, 0x14650fb0739d0383ull,
      0x14650fb0739d0383ull, 0x05e562996f19ed96ull, 0x6ad610726c07a413ull, 0x3e16eaafc9af5a52ull, 0x359e25c4b3634262ull}},
    {"no_mesh_kernel", 2, {49ull, 24ull, 0ull, 0ull, 0ull, 0ull}, 0, 0,
     {0xc06241d32a36f280ull, 0xf7dd0a8e4de56259ull, 0x33680c99d65e2cd8ull, 0x14650fb0739d0383ull, 0x14650fb0739d0383ull,
      0x14650fb0739d0383ull, 0x05e562996f19ed96ull, 0x6ad610726c07a413ull, 0x14650fb0739d0383ull, 0x14650fb0739d0383ull}},
};


// descriptor -> HostScene -> boxes -> SceneAccel, as odw_build_check and a context's first launch do it
int build_tables(const odw_scene_desc& d, const Run& r, Expect& got, std::string& err) {
  HostScene hs;
  int rc = scene_host_tables(&d, hs, err);
  if (rc) return rc;
  std::vector<Box> boxes;
  compute_boxes(hs, r.dist_tol, boxes);
  BuildOptions opt;
  opt.mesh_kernel = r.mesh_kernel;
  opt.cones = r.cones;
  opt.cone_stats = r.cone_stats;
  SceneAccel A;
  if ((rc = build_accel(hs, std::move(boxes), r.dist_tol, r.flat_limit, opt, A, err))) return rc;
  got.structure = A.kind();
  uint64_t dead = 0;
  for (char c : hs.dead) dead += c ? 1 : 0;
  const uint64_t sizes[6] = {(uint64_t)hs.n_prims, (uint64_t)A.nodes.size(), (uint64_t)A.grid.nx * (uint64_t)A.grid.ny * (uint64_t)A.grid.nz,
                             (uint64_t)A.grid.n_items, (uint64_t)A.grid.lds_bytes, dead};
  std::memcpy(got.sizes, sizes, sizeof sizes);
  got.spheres = A.grid.spheres;
  got.in_lds = A.grid.in_lds;
  got.hash[0] = fnv1a(hs.prim_hdr.data(), hs.prim_hdr.size() * sizeof(double));
  got.hash[1] = fnv1a(hs.dead.data(), hs.dead.size());
  got.hash[2] = fnv1a(hs.prim_i32.data(), hs.prim_i32.size() * sizeof(int32_t));
  got.hash[3] = fnv1a(A.planes.data(), A.planes.size() * sizeof(double));
  got.hash[4] = fnv1a(A.cells.data(), A.cells.size() * sizeof(uint32_t));
  got.hash[5] = fnv1a(A.items(), A.item_bytes());
  got.hash[6] = fnv1a(A.nodes.data(), A.nodes.size() * sizeof(BvhNode));
  got.hash[7] = fnv1a(A.order.data(), A.order.size() * sizeof(int));
  got.hash[8] = fnv1a(A.wide_nodes.data(), A.wide_nodes.size() * sizeof(uint32_t));
  // (the root's box as the presort reads it belongs to the wide tree)
  if (!A.wide_nodes.empty()) got.hash[8] = fnv1a(A.wide_hi, sizeof A.wide_hi, fnv1a(A.wide_lo, sizeof A.wide_lo, got.hash[8]));
  got.hash[9] = fnv1a(A.leaf_recs.data(), A.leaf_recs.size() * sizeof(float));
  return ODW_OK;
}

// ---- descriptors the library refuses: the code it answers with, and no crash ---------------------------------------
int check_refusals() {
  int bad = 0;
  const Run tmpl = {"refusal", Scene(), 1e-2, 64, true, true, false};
  auto expect = [&](const char* what, const Scene& s, int code, const odw_scene_desc* given = nullptr) {
    Expect got;
    std::memset(&got, 0, sizeof got);
    std::string err;
    const odw_scene_desc d = given ? *given : s.desc();
    const int rc = build_tables(d, tmpl, got, err);
    if (rc != code || err.empty()) { fprintf(stderr, "refusal '%s': code %d (%s), expected %d\n", what, rc, err.c_str(), code); ++bad; }
  };
  const double c[3] = {0, 0, 0};
  { Scene s = flat_scene(); s.type[6] = 7; expect("unknown primitive type", s, ODW_ERR_UNSUPPORTED); }
  { Scene s = flat_scene(); s.group[1] = 2; expect("group out of range", s, ODW_ERR_INVALID); }
  { Scene s = flat_scene(); s.cond_off[3] = 1; expect("bad condition offsets", s, ODW_ERR_INVALID); }
  { Scene s = one_leaf_scene(); s.add(ODW_PRIM_SPHERE, 0, 1, 0, 1, c, 1, 0, 0, {{0, kInside}}); expect("condition against a triangle", s, ODW_ERR_UNSUPPORTED); }
  { Scene s = flat_scene(); s.cond_inside[0] = 4; expect("cond_inside = 4", s, ODW_ERR_INVALID); }
  { Scene s = flat_scene(); s.cond_inside[2] = kInside; expect("first clause unmarked", s, ODW_ERR_INVALID); }
  { Scene s = one_leaf_scene(); for (int a = 0; a < 3; ++a) s.xform[12 + 6 + a] = s.xform[12 + 3 + a]; expect("degenerate triangle", s, ODW_ERR_INVALID); }
  { Scene s = mixed_scene(true); s.params[4 * 12 + 1] = 0.0; expect("paraboloid of height 0", s, ODW_ERR_INVALID); }
  { Scene s = flat_scene(); odw_scene_desc d = s.desc(); d.prim_params = nullptr; expect("null table pointer", s, ODW_ERR_INVALID, &d); }
  return bad;
}

}  // namespace

int main(int argc, char** argv) {
  const bool print = argc > 1 && std::strcmp(argv[1], "--print") == 0;
  const Run runs[] = {
      {"flat", flat_scene(), 1e-2, 64, true, true, false},
      {"grid_spheres", sphere_array(false), 1e-2, 64, true, true, false},
      {"grid_generic", sphere_array(true), 1e-2, 64, true, true, false},
      {"mixed_flat", mixed_scene(false), 1e-2, 64, true, true, false},
      {"mixed_limit4", mixed_scene(false), 1e-2, 4, true, true, false},
      {"mixed_paraboloid", mixed_scene(true), 1e-2, 64, true, true, false},
      {"tree_only", concentric_spheres(), 1e-2, 64, true, true, false},
      {"one_leaf", one_leaf_scene(), 1e-2, 64, false, true, false},
      {"wide_tol1e-2", facet_scene(), 1e-2, 64, true, true, false},
      {"wide_tol1e-6", facet_scene(), 1e-6, 64, true, true, true},
      {"wide_no_cones", facet_scene(), 1e-2, 64, true, false, false},
      {"no_mesh_kernel", facet_scene(), 1e-2, 64, false, true, false},
  };
  int bad = 0;
  size_t k = 0;
  for (const Run& r : runs) {
    Expect got;
    std::memset(&got, 0, sizeof got);
    got.name = r.name;
    std::string err;
    const odw_scene_desc d = r.scene.desc();
    const int rc = build_tables(d, r, got, err);
    if (rc) { fprintf(stderr, "%s: refused (%d): %s\n", r.name, rc, err.c_str()); ++bad; ++k; continue; }
    if (print) {
      printf("    {\"%s\", %d, {%lluull, %lluull, %lluull, %lluull, %lluull, %lluull}, %d, %d,\n     {", got.name, got.structure,
             (unsigned long long)got.sizes[0], (unsigned long long)got.sizes[1], (unsigned long long)got.sizes[2],
             (unsigned long long)got.sizes[3], (unsigned long long)got.sizes[4], (unsigned long long)got.sizes[5], got.spheres, got.in_lds);
      for (int i = 0; i < 10; ++i) printf("0x%016llxull%s", (unsigned long long)got.hash[i], i == 9 ? "}},\n" : (i == 4 ? ",\n      " : ", "));
    } else {
      static const char* tables[10] = {"headers", "dead flags", "flag words", "planes", "cells", "items", "nodes", "order", "wide words", "leaf records"};
      if (k >= sizeof kExpected / sizeof kExpected[0] || std::strcmp(kExpected[k].name, r.name)) { fprintf(stderr, "%s: no expectation\n", r.name); ++bad; ++k; continue; }
      const Expect& e = kExpected[k];
      if (got.structure != e.structure) { fprintf(stderr, "%s: structure %d, expected %d\n", r.name, got.structure, e.structure); ++bad; }
      for (int i = 0; i < 6; ++i)
        if (got.sizes[i] != e.sizes[i]) { fprintf(stderr, "%s: sizes[%d] = %llu, expected %llu\n", r.name, i, (unsigned long long)got.sizes[i], (unsigned long long)e.sizes[i]); ++bad; }
      if (got.spheres != e.spheres || got.in_lds != e.in_lds) { fprintf(stderr, "%s: spheres %d in_lds %d, expected %d %d\n", r.name, got.spheres, got.in_lds, e.spheres, e.in_lds); ++bad; }
      for (int i = 0; i < 10; ++i)
        if (got.hash[i] != e.hash[i]) { fprintf(stderr, "%s: the %s differ (hash %016llx, expected %016llx)\n", r.name, tables[i], (unsigned long long)got.hash[i], (unsigned long long)e.hash[i]); ++bad; }
    }
    ++k;
  }
  bad += check_refusals();
  if (!print) printf("%zu scenes built, %d mismatches\n", k, bad);
  return bad ? 1 : 0;
}
