// spec_image_main.hip -- the value-image builder of csrc/odw_build.h (box_centre_half, spec_image_layout,
// spec_image_build) under AddressSanitizer + UndefinedBehaviorSanitizer.
//
// A program of its own (tests/test_spec_image.py compiles and runs it; no GPU, no Python, nothing preloaded).
//  * box_centre_half on random intervals -- wide, thin, far from the origin, negative -- and on flat ones (lo == hi,
//    zero included): c - h <= lo and c + h >= hi in float64, h >= 0 and no wider than the roundings ask for;
//  * a scene of every primitive kind built by hand, its image written into a vector of exactly the layout's size (a
//    write past either end is the sanitizer's): boxes contain the headers' boxes, derived constants equal the
//    operations written out here, frames hold the entries that are neither 0 nor +-1, and an image built again after
//    the values changed under the same structure differs where it must.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "odw_kernels.hip"
#include "odw_grid.hip"
#include "odw_mesh.hip"
#include "odw_build.h"

namespace {

int mismatches = 0;

void expect(bool ok, const char* what, long at) {
  if (ok) return;
  ++mismatches;
  std::printf("MISMATCH %s (at %ld)\n", what, at);
}

uint64_t bits(double v) {
  uint64_t u;
  std::memcpy(&u, &v, sizeof u);
  return u;
}

// xorshift64*: the same cases on every run
struct Rng {
  uint64_t s;
  double next() {
    s ^= s >> 12; s ^= s << 25; s ^= s >> 27;
    return (double)((s * 2685821237109323ull) >> 11) * (1.0 / 9007199254740992.0);
  }
};

void check_interval(double lo, double hi, long at) {
#pragma clang fp contract(off)
  double c = 0, h = -1;
  box_centre_half(lo, hi, c, h);
  expect(h >= 0.0, "h >= 0", at);
  expect(c - h <= lo, "c - h <= lo", at);
  expect(c + h >= hi, "c + h >= hi", at);
  const double mag = std::max(std::fabs(lo), std::fabs(hi));
  const double ulp = std::nextafter(mag, INFINITY) - mag;
  expect(h <= 0.5 * (hi - lo) + 4.0 * ulp, "h tight", at);
}

void intervals() {
  Rng rng{88172645463325252ull};
  for (long k = 0; k < 200000; ++k) {
    const double scale = std::pow(10.0, -9.0 + 18.0 * rng.next());
    const double lo = (rng.next() - 0.5) * scale;
    const double width = k % 4 == 0 ? 0.0 : (k % 4 == 1 ? std::pow(10.0, -12.0 + 6.0 * rng.next()) : scale * rng.next());
    check_interval(lo, lo + width, k);
  }
  check_interval(0.0, 0.0, -1);
  check_interval(-0.0, 0.0, -2);
  check_interval(1e30, 1e30, -3);                  // (the box compute_boxes gives a dead primitive)
  check_interval(-1.0, std::nextafter(-1.0, 0.0), -4);
  check_interval(1.0, std::nextafter(1.0, 2.0), -5);
}

// a scene of one group per optical kind and one primitive of every kind that has constants, by hand
struct Hand {
  std::vector<int32_t> type, group, solid, flags, cond_off, cond_prim, cond_inside, gtype, grec, ggt, gorder;
  std::vector<double> xform, params, ior, refl, abslen, lpm, gdir;
  std::vector<uint64_t> seq;
  odw_scene_desc desc() {
    odw_scene_desc d;
    std::memset(&d, 0, sizeof d);
    d.n_prims = (int32_t)type.size();
    d.n_conds = (int32_t)cond_prim.size();
    d.n_groups = (int32_t)gtype.size();
    d.prim_type = type.data(); d.prim_group = group.data(); d.prim_solid = solid.data(); d.prim_flags = flags.data();
    d.prim_xform = xform.data(); d.prim_params = params.data(); d.prim_cond_off = cond_off.data();
    d.cond_prim = cond_prim.data(); d.cond_inside = cond_inside.data();
    d.group_type = gtype.data(); d.group_ior = ior.data(); d.group_refl = refl.data(); d.group_abslen = abslen.data();
    d.group_record = grec.data(); d.group_grating_type = ggt.data(); d.group_grating_lpm = lpm.data();
    d.group_grating_dir = gdir.data(); d.group_grating_order = gorder.data();
    d.seq_mask = seq.data();
    return d;
  }
};

Hand hand_scene(Rng& rng, double grow) {
  Hand h;
  const int kinds[] = {ODW_PRIM_BOX, ODW_PRIM_SPHERE, ODW_PRIM_CYLINDER, ODW_PRIM_CONE, ODW_PRIM_TORUS, ODW_PRIM_PARABOLOID,
                       ODW_PRIM_BOX};
  int p = 0;
  for (int kind : kinds) {
    h.type.push_back(kind);
    h.group.push_back(p % 2);
    h.solid.push_back(p);
    const int faces = kind == ODW_PRIM_BOX ? 0x3f : (kind == ODW_PRIM_SPHERE || kind == ODW_PRIM_TORUS) ? 1 : (kind == ODW_PRIM_PARABOLOID ? 5 : 7);
    h.flags.push_back(faces << ODW_FACEMASK_SHIFT);
    h.cond_off.push_back(0);
    // frames: identity with a translation, a quarter turn (entries 0 and +-1), a general rotation
    double m[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    if (p % 3 == 1) { const double q[12] = {0, -1, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0}; std::memcpy(m, q, sizeof m); }
    if (p % 3 == 2) {
      const double a = 0.3 + 0.1 * p, c = std::cos(a), s = std::sin(a);
      const double q[12] = {c, -s, 0, 0, s, c, 0, 0, 0, 0, 1, 0};
      std::memcpy(m, q, sizeof m);
    }
    m[3] = 20.0 * (rng.next() - 0.5); m[7] = p == 4 ? 0.0 : 20.0 * (rng.next() - 0.5); m[11] = -30.0 * p;
    for (double v : m) h.xform.push_back(v);
    double par[4] = {grow * (2.0 + 8.0 * rng.next()), grow * (1.0 + rng.next()), grow * (3.0 + 5.0 * rng.next()), 0.0};
    if (kind == ODW_PRIM_TORUS) par[0] += 4.0 * grow;            // R1 > R2
    for (double v : par) h.params.push_back(v);
    ++p;
  }
  h.cond_off.push_back(0);
  for (int g = 0; g < 2; ++g) {
    h.gtype.push_back(g == 0 ? ODW_OPT_MIRROR : ODW_OPT_LENS);
    h.ior.push_back(1.0 + 0.5 * g); h.refl.push_back(0.9); h.abslen.push_back(INFINITY);
    h.grec.push_back(1); h.ggt.push_back(0); h.gorder.push_back(1); h.lpm.push_back(0.0);
    h.gdir.push_back(1.0); h.gdir.push_back(0.0); h.gdir.push_back(0.0);
  }
  h.seq.push_back(0);
  return h;
}

std::vector<double> image_of(Hand& h, double tol, double max_len, SpecLayout& L, HostScene& hs) {
  odw_scene_desc d = h.desc();
  std::string err;
  const int rc = scene_host_tables(&d, hs, err);
  expect(rc == ODW_OK, err.c_str(), rc);
  if (rc != ODW_OK) return {};
  std::vector<Box> boxes;
  compute_boxes(hs, tol, boxes);
  L = spec_image_layout(hs);
  DeviceLimits lim;
  lim.max_ray_length = max_len; lim.dist_tol = tol; lim.power_tol = 1e-6; lim.max_intersections = 100;
  std::vector<double> img((size_t)L.size);
  img.shrink_to_fit();
  spec_image_build(hs, lim, L, img.data());
  return img;
}

void scene_checks() {
#pragma clang fp contract(off)
  Rng rng{0x9E3779B97F4A7C15ull};
  const double tol = 1e-6, max_len = 1000.0;
  Hand h = hand_scene(rng, 1.0);
  SpecLayout L;
  HostScene hs;
  const std::vector<double> img = image_of(h, tol, max_len, L, hs);
  if (img.empty()) return;
  expect(bits(img[0]) == bits(tol) && bits(img[1]) == bits(max_len + tol) && bits(img[2]) == bits(2.0 * tol), "limits", 0);
  for (int p = 0; p < L.n; ++p) {
    const double* pf = &hs.prim_f64[16 * (size_t)p];
    const double* par = pf + 12;
    int at = L.frame[p];
    for (int i = 0; i < 12; ++i) {
      const bool unit = i % 4 != 3 && (pf[i] == 1.0 || pf[i] == -1.0);
      if (pf[i] != 0.0 && !unit) expect(bits(img[at++]) == bits(pf[i]), "frame entry", p * 100 + i);
    }
    expect(at == L.par[p], "frame size", p);
    for (int k = 0; k < 4; ++k) expect(bits(img[L.par[p] + k]) == bits(par[k]), "parameter", p * 10 + k);
    expect(L.box[p] >= 0, "own box", p);
    if (L.box[p] >= 0)
      for (int a = 0; a < 3; ++a) {
        const double lo = hs.prim_hdr[8 * (size_t)p + a], hi = hs.prim_hdr[8 * (size_t)p + 3 + a];
        const double c = img[L.box[p] + a], hh = img[L.box[p] + 3 + a];
        expect(c - hh <= lo && c + hh >= hi && hh >= 0.0, "box contains the header's", p * 10 + a);
      }
    const int type = hs.prim_i32[4 * p];
    const double* d = L.der[p] >= 0 ? &img[L.der[p]] : nullptr;
    if (type == ODW_PRIM_BOX) {
      for (int a = 0; a < 3; ++a) expect(d && bits(d[a]) == bits(par[a] + tol), "box S + tol", p * 10 + a);
    } else if (type == ODW_PRIM_TORUS) {
      const double rin = std::fma(par[0] - par[1], 0.9999999, -1e-9);
      expect(d && bits(d[0]) == bits(std::fma(par[0] + par[1], 1.0000001, 1e-9)), "torus bound", p);
      expect(d && bits(d[1]) == bits(std::fma(par[1], 1.0000001, 1e-9)), "torus zs", p);
      expect(d && bits(d[2]) == bits(rin) && bits(d[3]) == bits(rin * rin), "torus rin", p);
    } else if (type == ODW_PRIM_CYLINDER) {
      const double R = par[0], H = par[1], rr = R * R;
      expect(d && bits(d[0]) == bits(H + tol) && bits(d[1]) == bits(rr * (1.0 - 1e-9)), "cylinder H + tol, lim", p);
      expect(d && bits(d[2]) == bits((R + tol) * (R + tol)) && bits(d[3]) == bits(d[2]), "cylinder caps", p);
    } else if (type == ODW_PRIM_CONE) {
      expect(d && bits(d[0]) == bits(par[2] + tol), "cone H + tol", p);
      expect(d && bits(d[2]) == bits((par[0] + tol) * (par[0] + tol)) && bits(d[3]) == bits((par[1] + tol) * (par[1] + tol)), "cone caps", p);
    } else if (type == ODW_PRIM_PARABOLOID) {
      expect(d && bits(d[0]) == bits(par[1] + tol) && bits(d[3]) == bits((par[2] + tol) * (par[2] + tol)), "paraboloid", p);
    } else {
      expect(L.der[p] < 0, "sphere has no constants", p);
    }
  }
  // other values under the same structure, other limits: the same layout, another image where the values enter
  Rng rng2{0x9E3779B97F4A7C15ull};
  Hand h2 = hand_scene(rng2, 1.25);
  SpecLayout L2;
  HostScene hs2;
  const std::vector<double> img2 = image_of(h2, tol, max_len, L2, hs2);
  expect(L2.size == L.size && L2.frame == L.frame && L2.par == L.par && L2.box == L.box && L2.der == L.der, "layout is structure", 0);
  if (img2.size() == img.size())
    for (int p = 0; p < L.n; ++p) {
      expect(bits(img2[L.par[p]]) != bits(img[L.par[p]]), "parameters follow the scene", p);
      if (L.der[p] >= 0) expect(bits(img2[L.der[p]]) != bits(img[L.der[p]]), "constants follow the scene", p);
      expect(bits(img2[L.box[p] + 3]) != bits(img[L.box[p] + 3]), "boxes follow the scene", p);
    }
  SpecLayout L3;
  HostScene hs3;
  const std::vector<double> img3 = image_of(h, 1e-3, 500.0, L3, hs3);
  if (img3.size() == img.size()) {
    expect(bits(img3[0]) == bits(1e-3) && bits(img3[1]) == bits(500.0 + 1e-3), "limits follow", 0);
    for (int p = 0; p < L.n; ++p)
      if (L.der[p] >= 0 && hs.prim_i32[4 * p] != ODW_PRIM_TORUS) expect(bits(img3[L.der[p]]) != bits(img[L.der[p]]), "constants follow the tolerance", p);
  }
  std::printf("%d primitives, image of %d doubles, in the arguments: %s\n", L.n, L.size, L.fits(sizeof(TraceParams)) ? "yes" : "no");
}

}  // namespace

int main() {
  intervals();
  scene_checks();
  std::printf("value image: %d mismatches\n", mismatches);
  return mismatches ? 1 : 0;
}
