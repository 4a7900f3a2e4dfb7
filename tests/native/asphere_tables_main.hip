// asphere_tables_main.hip -- what the host builders of csrc/odw_build.h make of the even asphere (primitive kind 9) under
// AddressSanitizer + UndefinedBehaviorSanitizer.
//
// A program of its own (tests/test_native_asphere_tables.py compiles and runs it; no GPU, no Python, nothing
// preloaded).  For several prescriptions: scene_host_tables keeps the parameters and fills the table row (coefficients,
// M, L, lowest sag), M and L bound the sampled maxima of what they bound, compute_boxes' box holds a dense sample of the
// surface, the wall and the cap under a turned frame, build_accel hands the scene to the grid or the binary tree (beside
// facets: the binary tree), and the value image -- written into a vector of exactly the layout's size, so that a write
// past either end is the sanitizer's -- holds the row behind the parameters and H + tol, (rim + tol)^2, rim^2 where the
// layout says.  Then the descriptors the library refuses, and a zero-filled descriptor without aspheres.
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
  std::vector<double> xform, params, coef;
  bool with_coef = true;
  int32_t gtype[2] = {ODW_OPT_LENS, ODW_OPT_ABSORBER}, grecord[2] = {0, 1};
  double gior[2] = {1.5, 1.0}, grefl[2] = {0.0, 0.0}, gabs[2] = {INFINITY, INFINITY};

  // a primitive whose frame is turned by `tilt` about x and centred at c
  void add(int t, int facemask, const double c[3], const double p[4], const double* co, double tilt) {
    const double cs = std::cos(tilt), sn = std::sin(tilt);
    const double R[9] = {1, 0, 0, 0, cs, sn, 0, -sn, cs};
    for (int r = 0; r < 3; ++r) {
      for (int k = 0; k < 3; ++k) xform.push_back(R[3 * r + k]);
      xform.push_back(-(R[3 * r] * c[0] + R[3 * r + 1] * c[1] + R[3 * r + 2] * c[2]));   // local = R (global - c)
    }
    type.push_back(t); group.push_back(0); solid.push_back((int32_t)type.size() - 1);
    flags.push_back(ODW_FLAG_CONVEX | (facemask << ODW_FACEMASK_SHIFT));
    params.insert(params.end(), p, p + 4);
    for (int k = 0; k < ODW_ASPH_COEFS; ++k) coef.push_back(co ? co[k] : 0.0);
    cond_off.push_back(0);
  }
  void facet(const double* v0, const double* v1, const double* v2) {
    for (const double* v : {v0, v1, v2}) xform.insert(xform.end(), v, v + 3);
    xform.insert(xform.end(), 3, 0.0);
    type.push_back(ODW_PRIM_TRIANGLE); group.push_back(1); solid.push_back((int32_t)type.size() - 1);
    flags.push_back(1 << ODW_FACEMASK_SHIFT);
    params.insert(params.end(), 4, 0.0);
    coef.insert(coef.end(), ODW_ASPH_COEFS, 0.0);
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
    if (with_coef) d.prim_coef = coef.data();
    return d;
  }
};

const double kCentre[3] = {3.0, -7.0, 11.0};
constexpr double kTilt = 0.7, kTol = 1e-6;

// the sag and its first two derivatives by rho, written out term by term (long double: the reference of the bounds)
void profile(const double* p, const double* co, long double rho, long double& s, long double& s1, long double& s2) {
  const long double c = p[0], kk = 1.0L + (long double)p[1], u = rho * rho;
  const long double q = std::sqrt(1.0L - kk * c * c * u);
  s = c * u / (1.0L + q);
  s1 = c * rho / q;
  s2 = c / (q * q * q);
  long double pw = 1.0L;                                     // rho^(2i-2)
  for (int i = 1; i <= ODW_ASPH_COEFS; ++i) {
    const long double a = co[i - 1];
    s += a * pw * u;
    s1 += 2.0L * i * a * pw * rho;
    s2 += 2.0L * i * (2.0L * i - 1.0L) * a * pw;
    pw *= u;
  }
}

void family(const double p[4], const double co[ODW_ASPH_COEFS]) {
#pragma clang fp contract(off)
  Scene s;
  s.add(ODW_PRIM_ASPHERE, 7, kCentre, p, co, kTilt);
  const odw_scene_desc d = s.desc();
  HostScene hs;
  std::string err;
  int rc = scene_host_tables(&d, hs, err);
  expect(rc == ODW_OK, "scene_host_tables accepts", p[1]);
  if (rc) { std::printf("  (%s)\n", err.c_str()); return; }
  const double* par = &hs.prim_f64[12];
  const double H = p[2], rim = p[3];
  expect(par[0] == p[0] && par[1] == p[1] && par[2] == H && par[3] == rim, "parameters kept", p[1]);
  expect(!(hs.prim_i32[2] & ODW_FLAG_CONVEX), "never the convex-solid hint", p[1]);
  expect(hs.asph.size() == ODW_ASPH_ROW, "one row of the asphere table", (double)hs.asph.size());
  if (hs.asph.size() != ODW_ASPH_ROW) return;
  const double* row = hs.asph.data();
  for (int k = 0; k < ODW_ASPH_COEFS; ++k) expect(row[k] == co[k], "coefficients in the row", k);
  const double M = row[8], L = row[9], z_min = row[10];
  // the bounds against dense samples over the disc rho <= rim (1 + 1e-3)
  long double m_max = 0, l_max = 0, lowest = INFINITY, highest = -INFINITY;
  for (int i = 0; i <= 4000; ++i) {
    const long double rho = (long double)rim * (1.0L + 1e-3L) * i / 4000.0L;
    long double sg, s1, s2;
    profile(p, co, rho, sg, s1, s2);
    l_max = std::max(l_max, std::fabs(s1));
    m_max = std::max(m_max, std::fabs(s2));
    if (i > 0) m_max = std::max(m_max, std::fabs(s1 / rho));
    if (rho <= rim) { lowest = std::min(lowest, sg); highest = std::max(highest, sg); }
  }
  expect((long double)M >= m_max, "M bounds |s_rr| and |s_r / r|", (double)m_max);
  expect((long double)L >= l_max, "L bounds |s_r|", (double)l_max);
  expect((long double)z_min <= lowest, "z_min at or below the lowest sag", (double)lowest);
  expect(std::isfinite(M) && std::isfinite(L) && M < 1e3 * ((double)m_max + 1e-12) + 1.0, "M is finite and no wild guess", M);
  expect((long double)H > highest, "the height lies above the surface", (double)highest);
  std::vector<Box> boxes;
  compute_boxes(hs, kTol, boxes);
  expect(!hs.dead[0], "alive", p[1]);
  // surface, wall and cap in the turned frame lie in the box
  const double cs = std::cos(kTilt), sn = std::sin(kTilt);
  for (int i = 0; i <= 64; ++i)
    for (int j = 0; j < 24; ++j) {
      const double rho = rim * i / 64.0, phi = 6.283185307179586 * j / 24.0;
      for (int part = 0; part < 3; ++part) {
        const double rr = part == 1 ? rim : rho;
        const double sg = asph_sag(p[0], p[1], co, rr * rr);
        const double z = part == 0 ? sg : (part == 1 ? sg + (H - sg) * i / 64.0 : H);
        const double l[3] = {rr * std::cos(phi), rr * std::sin(phi), z};
        const double g[3] = {l[0] + kCentre[0], cs * l[1] - sn * l[2] + kCentre[1], sn * l[1] + cs * l[2] + kCentre[2]};
        bool in = true;
        for (int a = 0; a < 3; ++a) in = in && g[a] >= boxes[0].lo[a] && g[a] <= boxes[0].hi[a];
        expect(in, "surface, wall and cap inside the box", p[1]);
      }
    }
  for (int a = 0; a < 3; ++a)
    expect(boxes[0].hi[a] - boxes[0].lo[a] <= 2.0 * rim + (H - z_min) + 1e-3, "box no wider than disc and height allow", p[1]);
  BuildOptions opt;
  SceneAccel A;
  rc = build_accel(hs, boxes, kTol, 64, opt, A, err);
  expect(rc == ODW_OK && (A.kind() == kAccelGrid || A.kind() == kAccelTree), "grid or binary tree, not the flat loop", p[1]);
  expect(flat_but_for_rare_quadrics(hs, 64), "flat but for its rare kind", p[1]);
  // the value image
  expect(spec_derived_count(ODW_PRIM_ASPHERE) == 3, "three derived constants", p[1]);
  const SpecLayout Lay = spec_image_layout(hs);
  DeviceLimits lim;
  std::memset(&lim, 0, sizeof lim);
  lim.max_ray_length = 1000.0; lim.dist_tol = kTol; lim.power_tol = 1e-9; lim.max_intersections = 100;
  std::vector<double> img((size_t)Lay.size, -1.0);
  spec_image_build(hs, lim, Lay, img.data());
  expect(Lay.box[0] == Lay.par[0] + 4 + ODW_ASPH_ROW, "the parameter block is 4 + 12 words", Lay.box[0] - Lay.par[0]);
  expect(Lay.der[0] >= 0 && Lay.der[0] + 3 == Lay.size, "derived constants close the image", p[1]);
  if (Lay.der[0] >= 0 && Lay.der[0] + 3 <= Lay.size) {
    const double* der = &img[(size_t)Lay.der[0]];
    expect(der[0] == H + kTol, "H + tol", p[1]);
    expect(der[1] == (rim + kTol) * (rim + kTol), "(rim + tol)^2", p[1]);
    expect(der[2] == rim * rim, "rim^2", p[1]);
  }
  for (int k = 0; k < 4; ++k) expect(img[(size_t)Lay.par[0] + k] == par[k], "parameters in the image", p[1]);
  for (int k = 0; k < ODW_ASPH_ROW; ++k) expect(img[(size_t)Lay.par[0] + 4 + k] == row[k], "the table row in the image", k);
}

void beside_facets() {
  Scene s;
  const double p[4] = {0.05, -0.8, 6.0, 10.0}, co[8] = {0, 1e-5, -2e-8, 3e-11, 0, 0, 0, 0};
  s.add(ODW_PRIM_ASPHERE, 7, kCentre, p, co, kTilt);
  const double v[4][3] = {{40, 0, 1}, {42, 0, 1}, {42, 3, 1}, {40, 3, 1}};
  s.facet(v[0], v[1], v[2]);
  s.facet(v[0], v[2], v[3]);
  const odw_scene_desc d = s.desc();
  HostScene hs;
  std::string err;
  int rc = scene_host_tables(&d, hs, err);
  expect(rc == ODW_OK, "facets beside an asphere accepted", 0);
  if (rc) return;
  expect(hs.asph.size() == 3 * ODW_ASPH_ROW, "the table has a row per primitive", (double)hs.asph.size());
  std::vector<Box> boxes;
  compute_boxes(hs, kTol, boxes);
  BuildOptions opt;
  SceneAccel A;
  rc = build_accel(hs, boxes, kTol, 64, opt, A, err);
  expect(rc == ODW_OK && A.kind() == kAccelTree, "facets beside an asphere: the binary tree", A.kind());
  expect(!flat_but_for_rare_quadrics(hs, 64), "facets: not a flat scene", 0);
}

void refusals() {
  struct Bad { double c, K, H, rim, a2; int facemask, code; bool coef; const char* what; };
  const Bad bad[] = {
      {NAN, 0.0, 5.0, 10.0, 0.0, 7, ODW_ERR_INVALID, true, "c not a number"},
      {0.05, INFINITY, 5.0, 10.0, 0.0, 7, ODW_ERR_INVALID, true, "K infinite"},
      {0.05, 0.0, NAN, 10.0, 0.0, 7, ODW_ERR_INVALID, true, "H not a number"},
      {0.05, 0.0, 5.0, INFINITY, 0.0, 7, ODW_ERR_INVALID, true, "rim infinite"},
      {0.05, 0.0, 5.0, 10.0, NAN, 7, ODW_ERR_INVALID, true, "a coefficient not a number"},
      {0.05, 0.0, 5.0, 0.0, 0.0, 7, ODW_ERR_INVALID, true, "rim = 0"},
      {0.05, 0.0, 5.0, -3.0, 0.0, 7, ODW_ERR_INVALID, true, "rim < 0"},
      {0.1, 0.0, 9.0, 9.95, 0.0, 7, ODW_ERR_INVALID, true, "(1 + K) c^2 rim^2 = 0.99"},
      {0.05, 0.0, 1.0, 10.0, 0.0, 7, ODW_ERR_INVALID, true, "H below the sag at the rim"},
      {0.05, 0.0, 2.6795, 10.0, 0.0, 7, ODW_ERR_INVALID, true, "H at the sag at the rim: not above the conservative maximum"},
      {-0.05, 0.0, 0.0, 10.0, 0.0, 7, ODW_ERR_INVALID, true, "H at the vertex of a surface that bends down"},
      {0.05, 0.0, 5.0, 10.0, 0.0, 7, ODW_ERR_UNSUPPORTED, false, "an asphere and no prim_coef: the kind is unknown"},
      {0.05, 0.0, 5.0, 10.0, 0.0, 15, ODW_ERR_UNSUPPORTED, true, "face 3"},
      {0.05, 0.0, 5.0, 10.0, 0.0, 0x81, ODW_ERR_UNSUPPORTED, true, "face 7"},
  };
  for (const Bad& b : bad) {
    Scene s;
    const double p[4] = {b.c, b.K, b.H, b.rim}, co[8] = {0, b.a2, 0, 0, 0, 0, 0, 0};
    s.add(ODW_PRIM_ASPHERE, b.facemask, kCentre, p, co, 0.0);
    s.with_coef = b.coef;
    const odw_scene_desc d = s.desc();
    HostScene hs;
    std::string err;
    const int rc = scene_host_tables(&d, hs, err);
    expect(rc == b.code && err.find("asphere") != std::string::npos, b.what, rc);
  }
  // accepted: every subset of the three faces; the limit 0.98 itself; a flat plate; a surface that bends down
  for (int facemask : {7, 1, 2, 4, 5, 0}) {
    Scene s;
    const double p[4] = {0.05, 0.0, 5.0, 10.0}, co[8] = {0};
    s.add(ODW_PRIM_ASPHERE, facemask, kCentre, p, co, 0.0);
    const odw_scene_desc d = s.desc();
    HostScene hs;
    std::string err;
    expect(scene_host_tables(&d, hs, err) == ODW_OK, "accepted face mask", facemask);
  }
  {
    Scene s;
    const double p1[4] = {0.0, 0.0, 1.0, 10.0}, p2[4] = {-0.05, -3.0, 0.5, 10.0}, co[8] = {0};
    s.add(ODW_PRIM_ASPHERE, 7, kCentre, p1, co, 0.0);
    s.add(ODW_PRIM_ASPHERE, 7, kCentre, p2, co, 0.0);
    const odw_scene_desc d = s.desc();
    HostScene hs;
    std::string err;
    expect(scene_host_tables(&d, hs, err) == ODW_OK, "a flat plate and a surface that bends down", 0);
    expect(hs.asph.size() == 2 * ODW_ASPH_ROW && hs.asph[8] >= 0.0, "their rows", (double)hs.asph.size());
  }
  { Scene s; const double p[4] = {1, 1, 1, 0}; s.add(10, 1, kCentre, p, nullptr, 0); const odw_scene_desc d = s.desc(); HostScene hs; std::string err;
    expect(scene_host_tables(&d, hs, err) == ODW_ERR_UNSUPPORTED, "kind 10 is unknown", 10); }
}

// a zero-filled descriptor that never sets prim_coef, without aspheres: what it always was, and no asphere table
void without_aspheres() {
  Scene s;
  const double box[4] = {2.0, 3.0, 4.0, 0.0}, cyl[4] = {2.0, 5.0, 0.0, 0.0};
  s.add(ODW_PRIM_BOX, 63, kCentre, box, nullptr, kTilt);
  s.add(ODW_PRIM_CYLINDER, 7, kCentre, cyl, nullptr, 0.0);
  s.with_coef = false;
  const odw_scene_desc d = s.desc();
  expect(d.prim_coef == nullptr, "the field stays null", 0);
  HostScene hs;
  std::string err;
  expect(scene_host_tables(&d, hs, err) == ODW_OK, "accepted without prim_coef", 0);
  expect(hs.asph.empty(), "no asphere table", (double)hs.asph.size());
  std::vector<Box> boxes;
  compute_boxes(hs, kTol, boxes);
  BuildOptions opt;
  SceneAccel A;
  expect(build_accel(hs, boxes, kTol, 64, opt, A, err) == ODW_OK && A.kind() != kAccelGrid && A.kind() != kAccelTree, "the flat loop", A.kind());
  const SpecLayout Lay = spec_image_layout(hs);
  expect(Lay.par[1] - Lay.par[0] == 4 + 6 + 3 + __builtin_popcount(xf_stored(xf_pattern(&hs.prim_f64[16]))), "parameter blocks of 4 words", Lay.par[1] - Lay.par[0]);
  std::vector<double> img((size_t)Lay.size, -1.0);
  DeviceLimits lim;
  std::memset(&lim, 0, sizeof lim);
  lim.max_ray_length = 1000.0; lim.dist_tol = kTol; lim.power_tol = 1e-9; lim.max_intersections = 100;
  spec_image_build(hs, lim, Lay, img.data());
  expect(img[(size_t)Lay.par[1]] == 2.0 && img[(size_t)Lay.par[1] + 1] == 5.0, "the cylinder's parameters", 0);
}

}  // namespace

int main() {
  const double general[4] = {0.05, -0.8, 6.0, 10.0}, general_co[8] = {0, 1e-5, -2e-8, 3e-11, 0, 0, 0, 0};
  family(general, general_co);
  const double moat[4] = {0.0, 0.0, 3.0, 16.0}, moat_co[8] = {-0.02, 1e-4, 0, 0, 0, 0, 0, 0};
  family(moat, moat_co);
  const double down[4] = {-0.04, -1.0, 1.0, 10.0}, down_co[8] = {0.0075, 0, 0, 0, 0, 0, 0, 0};
  family(down, down_co);
  const double steep[4] = {0.0995, 0.0, 9.5, 9.9}, steep_co[8] = {0};                       // (1 + K) c^2 rim^2 = 0.9703
  family(steep, steep_co);
  const double oblate[4] = {0.05, 2.0, 5.0, 11.0}, oblate_co[8] = {0, -1e-6, 0, 0, 0, 0, 0, 1e-19};
  family(oblate, oblate_co);
  const double plate[4] = {0.0, 0.0, 2.0, 25.0}, plate_co[8] = {0, 2e-6, 0, -1e-12, 0, 0, 0, 0};   // a Schmidt-like corrector
  family(plate, plate_co);
  beside_facets();
  refusals();
  without_aspheres();
  std::printf("asphere tables: %d checks, %d mismatches\n", checks, mismatches);
  return mismatches ? 1 : 0;
}
