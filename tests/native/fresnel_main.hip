// fresnel_main.hip -- the host twin of the Fresnel reflectance and odw_set_fresnel's validation (csrc/odw_build.h:
// fresnel_reflectance, fresnel_validate) under AddressSanitizer + UndefinedBehaviorSanitizer.
//
// A program of its own (tests/test_native_fresnel.py compiles and runs it; no GPU, no Python, nothing preloaded).  Every
// array is a vector of exactly the size the function is given (a read or write past either end is the sanitizer's).  The
// reflectance is held against the angle form of the formula in long double -- sines and tangents of i -+ t, no expression
// shared with the amplitude form under test -- and against its closed forms; the validation against tables made to be
// refused, one reason each.
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

int mismatches = 0, checks = 0;

void expect(bool ok, const char* what, double a = 0, double b = 0) {
  ++checks;
  if (ok) return;
  ++mismatches;
  std::printf("MISMATCH %s (%.17g, %.17g)\n", what, a, b);
}

bool refused(int rc, const std::string& err, const char* word) { return rc == ODW_ERR_INVALID && err.find(word) != std::string::npos; }

// R from the angle of incidence i (radians, 0 < i < pi / 2), not totally reflected
long double angle_form(long double n1, long double n2, long double i) {
  const long double t = asinl(n1 / n2 * sinl(i));
  const long double rs = sinl(i - t) / sinl(i + t), rp = tanl(i - t) / tanl(i + t);
  return 0.5L * (rs * rs + rp * rp);
}

}  // namespace

int main() {
  // ---- the reflectance ----
  {
    const double pairs[6][2] = {{1.0, 1.3}, {1.3, 1.0}, {1.0, 1.5}, {1.5, 1.0}, {1.0, 1.9}, {1.9, 1.0}};
    for (const auto& p : pairs) {
      const double n1 = p[0], n2 = p[1];
      for (int k = 1; k < 1000; ++k) {
        const long double i = (long double)k / 1000.0L * 1.5690L;      // up to 89.9 degrees
        const double cos_i = (double)cosl(i);
        const double mu = n1 / n2, root = 1.0 - mu * mu * (1.0 - cos_i * cos_i);
        const double R = fresnel_reflectance(n1, n2, cos_i);
        if (root < 0) { expect(R == 1.0, "total reflection", R, cos_i); continue; }
        expect(R >= 0.0 && R <= 1.0, "range", R, cos_i);
        if (std::fabs(root) < 1e-3) continue;                // (near the critical angle sqrt(root) amplifies rounding without bound)
        expect(std::fabs((double)((long double)R - angle_form(n1, n2, acosl((long double)cos_i)))) < 1e-12, "angle form", R, cos_i);
        // the four-argument form the device twin mirrors
        expect(fresnel_reflectance(n1, n2, cos_i, std::sqrt(root)) == R, "four arguments", R, cos_i);
      }
      const double r0 = (n1 - n2) / (n1 + n2);
      expect(std::fabs(fresnel_reflectance(n1, n2, 1.0) - r0 * r0) < 1e-15, "normal incidence", n1, n2);
      expect(std::fabs(fresnel_reflectance(n1, n2, 0.0) - 1.0) < 1e-15 || n1 > n2, "grazing incidence", n1, n2);
      // Brewster: tan i = n2 / n1, cos_t = sin_i, rp = 0
      const double ib = std::atan2(n2, n1), ci = std::cos(ib), ct = std::sin(ib);
      const double rs = (n1 * ci - n2 * ct) / (n1 * ci + n2 * ct);
      expect(std::fabs(fresnel_reflectance(n1, n2, ci) - 0.5 * rs * rs) < 1e-15, "Brewster", n1, n2);
      // reciprocity: R(n1 -> n2, i) = R(n2 -> n1, t)
      for (int k = 0; k < 80; ++k) {
        const double i = 0.0174 * k, si = std::sin(i) * n1 / n2;
        if (si >= 0.999) continue;
        expect(std::fabs(fresnel_reflectance(n1, n2, std::cos(i)) - fresnel_reflectance(n2, n1, std::sqrt(1.0 - si * si))) < 1e-12, "reciprocity", n1, i);
      }
    }
    expect(fresnel_reflectance(1.0, 1.0, 0.5) == 0.0, "no surface");       // (0.5: root = 0.25 and its square root are exact)
  }
  // ---- odw_set_fresnel's validation ----
  {
    const int G = 6;
    // groups: lens, mirror, reflection grating, transmission grating, absorber, vacuum
    std::vector<int32_t> gi = {ODW_OPT_LENS, 0, 0, 1, ODW_OPT_MIRROR, 0, 0, 1, ODW_OPT_GRATING, 0, 0, 1, ODW_OPT_GRATING, 0, 1, 1,
                               ODW_OPT_ABSORBER, 1, 0, 1, ODW_OPT_VACUUM, 1, 0, 1};
    std::vector<int32_t> mode(G, 0);
    std::string err;
    expect(fresnel_validate(G, mode.data(), gi.data(), err) == ODW_OK, "no mode");
    expect(fresnel_validate(0, nullptr, nullptr, err) == ODW_OK, "none");
    for (int m : {ODW_FRESNEL_LOSS, ODW_FRESNEL_SPLIT}) {
      mode.assign(G, 0);
      mode[0] = m;
      expect(fresnel_validate(G, mode.data(), gi.data(), err) == ODW_OK, "a lens", m);
      for (int g = 1; g < G; ++g) {
        std::vector<int32_t> m2(G, 0);
        m2[g] = m;
        char word[64];
        std::snprintf(word, sizeof word, "group %d: a Fresnel mode on a group that is not a lens", g);
        expect(refused(fresnel_validate(G, m2.data(), gi.data(), err), err, word), "group type", g, m);
        expect(fresnel_validate(G, m2.data(), nullptr, err) == ODW_OK, "no types at hand", g, m);
      }
    }
    for (int bad : {3, -1, 1 << 20}) {
      std::vector<int32_t> m2(G, 0);
      m2[0] = bad;
      expect(refused(fresnel_validate(G, m2.data(), gi.data(), err), err, "group 0: unknown Fresnel mode"), "unknown mode", bad);
    }
    expect(fresnel_validate(ODW_MAX_GROUPS + 1, mode.data(), nullptr, err) == ODW_ERR_INVALID, "too many groups");
    expect(fresnel_validate(-1, mode.data(), nullptr, err) == ODW_ERR_INVALID, "a negative count");
    expect(fresnel_validate(G, nullptr, gi.data(), err) == ODW_ERR_INVALID, "null modes");
    // a full table
    std::vector<int32_t> all((size_t)ODW_MAX_GROUPS, ODW_FRESNEL_SPLIT), lenses((size_t)ODW_MAX_GROUPS * 4, 0);
    for (int g = 0; g < ODW_MAX_GROUPS; ++g) lenses[4 * (size_t)g] = ODW_OPT_LENS;
    expect(fresnel_validate(ODW_MAX_GROUPS, all.data(), lenses.data(), err) == ODW_OK, "every group a lens");
  }
  std::printf("fresnel: %d checks, %d mismatches\n", checks, mismatches);
  return mismatches ? 1 : 0;
}
