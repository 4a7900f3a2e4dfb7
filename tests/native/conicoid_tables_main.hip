// conicoid_tables_main.hip -- what the host builders of csrc/odw_build.h make of the conicoid (primitive kind 8) under
// AddressSanitizer + UndefinedBehaviorSanitizer.
//
// A program of its own (tests/test_native_conicoid_tables.py compiles and runs it; no GPU, no Python, nothing
// preloaded).  For every family of the conic constant: scene_host_tables fills the rim, compute_boxes' box holds points
// of the surface and of the cap under a turned frame, build_accel hands the scene to the grid or the binary tree (and,
// beside facets, to the binary tree, not the eight-wide one), flat_but_for_rare_quadrics counts the kind, and the value
// image -- written into a vector of exactly the layout's size, so that a write past either end is the sanitizer's --
// holds H + tol, (rim + tol)^2 and 1 + K where the layout says.  Then the descriptors the library refuses.
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

int checks = 0, mismatches = 0;

void expect(bool ok, const char* what, double at) {
  ++checks;
  if (ok) return;
  ++mismatches;
  std::printf("MISMATCH %s (at %g)\n", what, at);
}

struct Scene {
  std::vector<int32_t> type, group, solid, flags, cond_off{0}, cond_prim, cond_inside;
  std::vector<double> xform, params;
  int32_t gtype[2] = {ODW_OPT_LENS, ODW_OPT_ABSORBER}, grecord[2] = {0, 1};
  double gior[2] = {1.5, 1.0}, grefl[2] = {0.0, 0.0}, gabs[2] = {INFINITY, INFINITY};

  // a primitive whose frame is turned by `tilt` about x and centred at c
  void add(int t, int facemask, const double c[3], double p0, double p1, double p2, double p3, double tilt) {
    const double cs = std::cos(tilt), sn = std::sin(tilt);
    const double R[9] = {1, 0, 0, 0, cs, sn, 0, -sn, cs};
    for (int r = 0; r < 3; ++r) {
      for (int k = 0; k < 3; ++k) xform.push_back(R[3 * r + k]);
      xform.push_back(-(R[3 * r] * c[0] + R[3 * r + 1] * c[1] + R[3 * r + 2] * c[2]));   // local = R (global - c)
    }
    type.push_back(t); group.push_back(0); solid.push_back((int32_t)type.size() - 1);
    flags.push_back(ODW_FLAG_CONVEX | (facemask << ODW_FACEMASK_SHIFT));
    for (double v : {p0, p1, p2, p3}) params.push_back(v);
    cond_off.push_back(0);
  }
  // a facet given by its three corners
  void facet(const double* v0, const double* v1, const double* v2) {
    for (const double* v : {v0, v1, v2}) xform.insert(xform.end(), v, v + 3);
    xform.insert(xform.end(), 3, 0.0);
    type.push_back(ODW_PRIM_TRIANGLE); group.push_back(1); solid.push_back((int32_t)type.size() - 1);
    flags.push_back(1 << ODW_FACEMASK_SHIFT);
    params.insert(params.end(), 4, 0.0);
    cond_off.push_back(0);
  }
  odw_scene_desc desc() const {
    odw_scene_desc d;
    std::memset(&d, 0, sizeof d);
    d.n_prims = (int32_t)type.size();
    d.prim_type = type.data(); d.prim_group = group.data(); d.prim_solid = solid.data(); d.prim_flags = flags.data();
    d.prim_xform = xform.data(); d.prim_params = params.data(); d.prim_cond_off = cond_off.data();
    d.cond_prim = cond_prim.data(); d.cond_inside = cond_inside.data();
    d.n_groups = 2;
    d.group_type = gtype; d.group_ior = gior; d.group_refl = grefl; d.group_abslen = gabs; d.group_record = grecord;
    return d;
  }
};

const double kCentre[3] = {3.0, -7.0, 11.0};
constexpr double kTilt = 0.7, kTol = 1e-6;

void family(double R, double K, double H) {
#pragma clang fp contract(off)
  Scene s;
  s.add(ODW_PRIM_CONICOID, 5, kCentre, R, K, H, 123.0, kTilt);          // (the rim is the library's to fill)
  const odw_scene_desc d = s.desc();
  HostScene hs;
  std::string err;
  int rc = scene_host_tables(&d, hs, err);
  expect(rc == ODW_OK, "scene_host_tables accepts", K);
  if (rc) return;
  const double* par = &hs.prim_f64[12];
  const double rim = std::sqrt(2.0 * R * H - (1.0 + K) * H * H);
  expect(par[0] == R && par[1] == K && par[2] == H && par[3] == rim, "parameters, rim filled", K);
  std::vector<Box> boxes;
  compute_boxes(hs, kTol, boxes);
  expect(!hs.dead[0], "alive", K);
  // points of the surface and of the cap, in the turned frame, lie in the box; the box is no larger than the cylinder's
  const double cs = std::cos(kTilt), sn = std::sin(kTilt);
  for (int i = 0; i <= 16; ++i)
    for (int j = 0; j < 24; ++j) {
      const double rho = rim * i / 16.0, phi = 6.283185307179586 * j / 24.0;
      for (int cap = 0; cap < 2; ++cap) {
        const double l[3] = {rho * std::cos(phi), rho * std::sin(phi), cap ? H : rho * rho / (R + std::sqrt(R * R - (1.0 + K) * rho * rho))};
        // global = R^T local + c
        const double g[3] = {l[0] + kCentre[0], cs * l[1] - sn * l[2] + kCentre[1], sn * l[1] + cs * l[2] + kCentre[2]};
        bool in = true;
        for (int a = 0; a < 3; ++a) in = in && g[a] >= boxes[0].lo[a] && g[a] <= boxes[0].hi[a];
        expect(in, "surface and cap inside the box", K);
      }
    }
  for (int a = 0; a < 3; ++a) expect(boxes[0].hi[a] - boxes[0].lo[a] <= 2.0 * rim + H + 1e-3, "box no wider than rim and height allow", K);
  BuildOptions opt;
  SceneAccel A;
  rc = build_accel(hs, boxes, kTol, 64, opt, A, err);
  expect(rc == ODW_OK && (A.kind() == kAccelGrid || A.kind() == kAccelTree), "grid or binary tree, not the flat loop", K);
  expect(flat_but_for_rare_quadrics(hs, 64), "flat but for its rare quadric", K);
  expect(!flat_but_for_rare_quadrics(hs, 0), "not beyond the flat limit", K);
  // the value image
  expect(spec_derived_count(ODW_PRIM_CONICOID) == 3, "three derived constants", K);
  const SpecLayout L = spec_image_layout(hs);
  DeviceLimits lim;
  std::memset(&lim, 0, sizeof lim);
  lim.max_ray_length = 1000.0; lim.dist_tol = kTol; lim.power_tol = 1e-9; lim.max_intersections = 100;
  std::vector<double> img((size_t)L.size, -1.0);
  spec_image_build(hs, lim, L, img.data());
  expect(L.der[0] >= 0 && L.der[0] + 3 == L.size, "derived constants close the image", K);
  if (L.der[0] >= 0 && L.der[0] + 3 <= L.size) {
    const double* der = &img[(size_t)L.der[0]];
    expect(der[0] == H + kTol, "H + tol", K);
    expect(der[1] == (rim + kTol) * (rim + kTol), "(rim + tol)^2", K);
    expect(der[2] == 1.0 + K, "1 + K", K);
  }
  for (int k = 0; k < 4; ++k) expect(img[(size_t)L.par[0] + k] == par[k], "parameters in the image", K);
}

void beside_facets() {
  Scene s;
  s.add(ODW_PRIM_CONICOID, 5, kCentre, 10.0, -2.25, 8.0, 0.0, kTilt);
  const double v[4][3] = {{40, 0, 1}, {42, 0, 1}, {42, 3, 1}, {40, 3, 1}};
  s.facet(v[0], v[1], v[2]);
  s.facet(v[0], v[2], v[3]);
  const odw_scene_desc d = s.desc();
  HostScene hs;
  std::string err;
  int rc = scene_host_tables(&d, hs, err);
  expect(rc == ODW_OK, "facets beside a conicoid accepted", 0);
  if (rc) return;
  std::vector<Box> boxes;
  compute_boxes(hs, kTol, boxes);
  BuildOptions opt;
  SceneAccel A;
  rc = build_accel(hs, boxes, kTol, 64, opt, A, err);
  expect(rc == ODW_OK && A.kind() == kAccelTree, "facets beside a conicoid: the binary tree", A.kind());
  expect(!flat_but_for_rare_quadrics(hs, 64), "facets: not a flat scene", 0);
}

void refusals() {
  struct Bad { double R, K, H; int facemask, code; const char* what; };
  const Bad bad[] = {
      {0.0, -1.0, 5.0, 5, ODW_ERR_INVALID, "R = 0"},
      {-2.0, -1.0, 5.0, 5, ODW_ERR_INVALID, "R < 0"},
      {10.0, -1.0, 0.0, 5, ODW_ERR_INVALID, "H = 0"},
      {10.0, -3.0, -1.0, 5, ODW_ERR_INVALID, "H < 0"},
      {10.0, 1.0, 5.000001, 5, ODW_ERR_INVALID, "K = 1 beyond its half"},
      {10.0, NAN, 5.0, 5, ODW_ERR_INVALID, "K not a number"},
      {NAN, 0.0, 5.0, 5, ODW_ERR_INVALID, "R not a number"},
      {10.0, 0.0, NAN, 5, ODW_ERR_INVALID, "H not a number"},
      {INFINITY, 0.0, 5.0, 5, ODW_ERR_INVALID, "R infinite"},
      {10.0, -INFINITY, 5.0, 5, ODW_ERR_INVALID, "K infinite"},
      {10.0, -1.0, 5.0, 7, ODW_ERR_UNSUPPORTED, "face 1"},
      {10.0, -1.0, 5.0, 2, ODW_ERR_UNSUPPORTED, "face 1 alone"},
  };
  for (const Bad& b : bad) {
    Scene s;
    s.add(ODW_PRIM_CONICOID, b.facemask, kCentre, b.R, b.K, b.H, 0.0, 0.0);
    const odw_scene_desc d = s.desc();
    HostScene hs;
    std::string err;
    const int rc = scene_host_tables(&d, hs, err);
    expect(rc == b.code && err.find("conicoid") != std::string::npos, b.what, rc);
  }
  // the equator itself is allowed; so are faces 0 and 2 alone, and none (a pure operand)
  for (int facemask : {5, 1, 4, 0}) {
    Scene s;
    s.add(ODW_PRIM_CONICOID, facemask, kCentre, 10.0, 1.0, 5.0, 0.0, 0.0);
    const odw_scene_desc d = s.desc();
    HostScene hs;
    std::string err;
    expect(scene_host_tables(&d, hs, err) == ODW_OK, "accepted face mask at the equator", facemask);
  }
  { Scene s; s.add(9, 1, kCentre, 1, 1, 1, 0, 0); const odw_scene_desc d = s.desc(); HostScene hs; std::string err;
    expect(scene_host_tables(&d, hs, err) == ODW_ERR_UNSUPPORTED, "kind 9 is unknown", 9); }
}

}  // namespace

int main() {
  family(10.0, -2.25, 8.0);
  family(10.0, -1.0, 8.0);
  family(10.0, -0.5, 8.0);
  family(10.0, 0.0, 8.0);
  family(10.0, 0.0, 10.0);      // a hemisphere: up to the equator
  family(10.0, 1.0, 4.0);
  family(0.37, -40.0, 55.0);    // a needle
  beside_facets();
  refusals();
  std::printf("conicoid tables: %d checks, %d mismatches\n", checks, mismatches);
  return mismatches ? 1 : 0;
}
