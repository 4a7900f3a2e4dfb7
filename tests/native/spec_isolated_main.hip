// spec_isolated_main.hip -- the mask of isolated solids in the value image of the compiled kernels (csrc/odw_build.h:
// spec_isolated_mask, spec_image_layout, spec_image_build) under AddressSanitizer + UndefinedBehaviorSanitizer.
//
// A program of its own (tests/test_spec_isolated_build.py compiles and runs it; no GPU, no Python, nothing preloaded).
// A scene built by hand -- a lens of two primitives (solid 0), a box far from everything (solid 1), a box whose distance
// from the lens is the parameter (solid 2), and a box with a solid id the mask has no bit for (solid 70) --, its image
// written whole into a vector of exactly its words (a write past either end is the sanitizer's):
//  * the word lies behind the image's last double (at the layout's size; the image a kernel reads is one word longer);
//  * bit s of the word is set exactly where compute_boxes has flagged the primitives of solid s, for s < 64;
//  * the word follows the values -- the box moved to within 4 distTol of the lens clears the lens's bit and its own --
//    while the layout stays what it was.
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
    d.group_record = grec.data(); d.group_grating_type = ggt.data(); d.group_grating_order = gorder.data();
    d.group_grating_lpm = lpm.data(); d.group_grating_dir = gdir.data();
    d.seq_mask = seq.data();
    return d;
  }
  void prim(int kind, int g, int sid, int faces, double x, double y, double z, double p0, double p1, double p2) {
    type.push_back(kind); group.push_back(g); solid.push_back(sid);
    flags.push_back(faces << ODW_FACEMASK_SHIFT);
    cond_off.push_back(0);
    // a frame maps global to local coordinates: the primitive stands at (x, y, z)
    const double m[12] = {1, 0, 0, -x, 0, 1, 0, -y, 0, 0, 1, -z};
    for (double v : m) xform.push_back(v);
    const double par[4] = {p0, p1, p2, 0.0};
    for (double v : par) params.push_back(v);
  }
};

// near_x: where the movable box begins along x (the lens's cylinder ends at x = 8)
Hand hand_scene(double near_x) {
  Hand h;
  h.prim(ODW_PRIM_SPHERE, 1, 0, 1, 0.0, 0.0, 2.0, 3.0, 0.0, 0.0);     // (inside the cylinder's box: the lens spans x = -8 .. 8)
  h.prim(ODW_PRIM_CYLINDER, 1, 0, 7, 0.0, 0.0, -1.0, 8.0, 5.0, 0.0);
  h.prim(ODW_PRIM_BOX, 0, 1, 0x3f, -20.0, -20.0, 70.0, 40.0, 40.0, 2.0);
  h.prim(ODW_PRIM_BOX, 0, 2, 0x3f, near_x, -20.0, -5.0, 6.0, 40.0, 20.0);
  h.prim(ODW_PRIM_BOX, 0, 70, 0x3f, -20.0, -20.0, -90.0, 40.0, 40.0, 2.0);
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

struct Built {
  HostScene hs;
  SpecLayout L;
  std::vector<double> img;
  uint64_t word = 0;
};

bool build(double near_x, double tol, Built& b) {
  Hand h = hand_scene(near_x);
  odw_scene_desc d = h.desc();
  std::string err;
  const int rc = scene_host_tables(&d, b.hs, err);
  expect(rc == ODW_OK, err.c_str(), rc);
  if (rc != ODW_OK) return false;
  std::vector<Box> boxes;
  compute_boxes(b.hs, tol, boxes);
  b.L = spec_image_layout(b.hs);
  DeviceLimits lim;
  lim.max_ray_length = 1000.0; lim.dist_tol = tol; lim.power_tol = 1e-6; lim.max_intersections = 100;
  b.img.assign((size_t)b.L.words(), -1.0);
  b.img.shrink_to_fit();
  spec_image_build(b.hs, lim, b.L, b.img.data(), nullptr, true);
  // (the doubles alone: the word behind them is left as it was)
  std::vector<double> plain((size_t)b.L.size + 1, -1.0);
  spec_image_build(b.hs, lim, b.L, plain.data());
  expect(plain.back() == -1.0 && std::memcmp(plain.data(), b.img.data(), (size_t)b.L.size * sizeof(double)) == 0, "the doubles alone", 0);
  std::memcpy(&b.word, &b.img[(size_t)b.L.iso], sizeof b.word);
  return true;
}

void check(const Built& b, long at) {
  const SpecLayout& L = b.L;
  expect(L.iso >= kSpecImageLimits && L.iso < L.words(), "the word lies inside the image", at);
  expect(L.iso == L.size && L.words() == L.size + 1 && L.iso > L.par[L.n - 1] + 3, "behind the last double", at);
  uint64_t want = 0;
  for (int p = 0; p < b.hs.n_prims; ++p) {
    const int32_t w = b.hs.prim_i32[4 * (size_t)p + 2];
    const int sid = w >> ODW_SOLID_SHIFT;
    if ((w & ODW_FLAG_ISOLATED) && sid < 64) want |= 1ull << sid;
    if (sid < 64) expect((((b.word >> sid) & 1ull) != 0) == ((w & ODW_FLAG_ISOLATED) != 0), "bit = flag", at * 100 + p);
  }
  expect(b.word == want && b.word == spec_isolated_mask(b.hs), "the word is the mask of the flags", at);
}

void scene_checks() {
  const double tol = 1e-6;
  Built away, near;
  if (!build(9.0, tol, away) || !build(8.0 + 5e-6, tol, near)) return;
  check(away, 1);
  check(near, 2);
  // clear of everything: the lens, both mirrors; the solid of id 70 is flagged by compute_boxes and has no bit
  expect(away.word == 0x7ull, "away: solids 0, 1 and 2", (long)away.word);
  expect((away.hs.prim_i32[4 * 4 + 2] & ODW_FLAG_ISOLATED) != 0, "solid 70 carries the flag", 0);
  // the box within 4 distTol of the lens: neither is isolated, the far mirror still is
  expect(near.word == 0x2ull, "near: solid 1 alone", (long)near.word);
  expect(near.L.size == away.L.size && near.L.iso == away.L.iso && near.L.frame == away.L.frame && near.L.par == away.L.par &&
         near.L.box == away.L.box && near.L.der == away.L.der, "layout is structure", 0);
  std::printf("%d primitives, image of %d doubles, mask word at %d: away %#llx, near %#llx\n", away.L.n, away.L.size, away.L.iso,
              (unsigned long long)away.word, (unsigned long long)near.word);
}

}  // namespace

int main() {
  scene_checks();
  std::printf("isolated mask: %d mismatches\n", mismatches);
  return mismatches ? 1 : 0;
}
