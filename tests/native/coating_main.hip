// coating_main.hip -- the host twin of the coated reflectance and odw_set_coating's validation (csrc/odw_build.h:
// coated_reflectance, coating_validate) under AddressSanitizer + UndefinedBehaviorSanitizer.
//
// A program of its own (tests/test_native_coating.py compiles and runs it; no GPU, no Python, nothing preloaded).  Every
// array is a vector of exactly the size the function is given (a read or write past either end is the sanitizer's).  The
// reflectance is held against the characteristic matrices in std::complex<long double> -- explicit 2 x 2 products, no
// expression shared with the real recurrences under test -- and against its closed forms; the validation against tables
// made to be refused, one reason each.
#include <hip/hip_runtime.h>

#include <cmath>
#include <complex>
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

typedef std::complex<long double> cld;

// |r|^2 of the stack `met` (in the order the ray meets it) between the admittances e0 and es
long double stack_R(long double e0, long double es, const std::vector<std::pair<long double, long double>>& eta_delta) {
  cld m00 = 1, m01 = 0, m10 = 0, m11 = 1;
  for (const auto& l : eta_delta) {
    const cld a = cosl(l.second), b = cld(0, sinl(l.second) / l.first), c = cld(0, l.first * sinl(l.second));
    const cld n00 = m00 * a + m01 * c, n01 = m00 * b + m01 * a, n10 = m10 * a + m11 * c, n11 = m10 * b + m11 * a;
    m00 = n00; m01 = n01; m10 = n10; m11 = n11;
  }
  const cld B = m00 + m01 * es, C = m10 + m11 * es;
  return std::norm((e0 * B - C) / (e0 * B + C));
}

long double matrix_form(long double n1, long double n2, long double cos_i, bool entering, const std::vector<double>& layers,
                        long double wl) {
  const long double s2 = n1 * n1 * (1 - cos_i * cos_i), cos_t = sqrtl(1 - s2 / (n2 * n2));
  const int k = (int)layers.size() / 2;
  std::vector<std::pair<long double, long double>> s, p;
  for (int i = 0; i < k; ++i) {
    const int j = entering ? i : k - 1 - i;
    const long double nj = layers[2 * (size_t)j], dj = layers[2 * (size_t)j + 1], cj = sqrtl(1 - s2 / (nj * nj));
    const long double delta = 2 * acosl(-1.0L) * nj * dj * cj / wl;
    s.push_back({nj * cj, delta});
    p.push_back({nj / cj, delta});
  }
  return 0.5L * (stack_R(n1 * cos_i, n2 * cos_t, s) + stack_R(n1 / cos_i, n2 / cos_t, p));
}

}  // namespace

int main() {
  const std::vector<std::vector<double>> stacks = {{1.38, 550.0 / 4 / 1.38},
                                                   {1.38, 99.6, 2.1, 130.9},
                                                   {1.38, 99.6, 2.0, 137.5, 1.62, 84.9},
                                                   {1.38, 90.0, 2.3, 20.0, 1.46, 35.0, 2.3, 110.0}};
  // ---- the reflectance ----
  {
    for (const std::vector<double>& st : stacks) {
      const int k = (int)st.size() / 2;
      for (double wl : {450.0, 550.0, 650.0}) {
        for (int side = 0; side < 2; ++side) {
          const double n1 = side ? 1.5 : 1.0, n2 = side ? 1.0 : 1.5;
          const bool entering = side == 0;
          for (int a = 0; a <= (side ? 410 : 850); ++a) {          // entering 0 .. 85 degrees, leaving 0 .. 41 degrees
            const double cos_i = std::cos(a * 0.1 * 3.14159265358979323846 / 180.0);
            const double R = coated_reflectance(n1, n2, cos_i, entering, k, st.data(), wl);
            expect(R >= 0.0 && R <= 1.0, "range", R, cos_i);
            expect(std::fabs((double)((long double)R - matrix_form(n1, n2, cos_i, entering, st, wl))) < 1e-12, "matrix form", R, cos_i);
            const double mu = n1 / n2, root = 1.0 - mu * mu * (1.0 - cos_i * cos_i);
            expect(coated_reflectance(n1, n2, cos_i, std::sqrt(root), entering, k, st.data(), wl) == R, "eight arguments", R, cos_i);
            // the stack seen from the other side at the same transverse wave vector
            const double back = coated_reflectance(n2, n1, std::sqrt(root), !entering, k, st.data(), wl);
            expect(std::fabs(back - R) < 1e-12, "other side", R, back);
          }
          // total reflection: 1, whatever the stack
          if (side) expect(coated_reflectance(n1, n2, 0.5, entering, k, st.data(), wl) == 1.0, "total reflection");
        }
      }
    }
    // closed forms
    const double q = (1.5 - 1.38 * 1.38) / (1.5 + 1.38 * 1.38);
    expect(std::fabs(coated_reflectance(1.0, 1.5, 1.0, true, 1, stacks[0].data(), 550.0) - q * q) < 1e-15, "quarter wave");
    const std::vector<double> half = {1.38, 550.0 / 2 / 1.38}, none = {1.38, 0.0};
    expect(std::fabs(coated_reflectance(1.0, 1.5, 1.0, true, 1, half.data(), 550.0) - 0.04) < 1e-12, "half wave");
    for (int a = 0; a <= 85; ++a) {
      const double cos_i = std::cos(a * 3.14159265358979323846 / 180.0);
      expect(std::fabs(coated_reflectance(1.0, 1.5, cos_i, true, 1, none.data(), 550.0) - fresnel_reflectance(1.0, 1.5, cos_i)) < 1e-15,
             "no thickness", cos_i);
      expect(coated_reflectance(1.0, 1.5, cos_i, true, 0, nullptr, 550.0) == fresnel_reflectance(1.0, 1.5, cos_i), "no layers", cos_i);
    }
    // a layer that would hold an evanescent wave: the bare reflectance, bit for bit
    const std::vector<double> low = {1.38, 100.0};
    for (int a = 56; a <= 69; ++a) {
      const double cos_i = std::cos(a * 3.14159265358979323846 / 180.0);
      expect(coated_reflectance(1.7, 1.6, cos_i, true, 1, low.data(), 550.0) == fresnel_reflectance(1.7, 1.6, cos_i), "evanescent", cos_i);
      const std::vector<double> two = {1.65, 80.0, 1.38, 100.0};
      expect(coated_reflectance(1.7, 1.6, cos_i, true, 2, two.data(), 550.0) == fresnel_reflectance(1.7, 1.6, cos_i), "evanescent, second layer", cos_i);
      expect(coated_reflectance(1.7, 1.6, cos_i, false, 2, two.data(), 550.0) == fresnel_reflectance(1.7, 1.6, cos_i), "evanescent, reversed", cos_i);
    }
    // orientation: V at 450 nm from the glass
    const double right = coated_reflectance(1.5, 1.0, 1.0, false, 2, stacks[1].data(), 450.0);
    const double wrong = coated_reflectance(1.5, 1.0, 1.0, true, 2, stacks[1].data(), 450.0);
    expect(std::fabs(right - 0.0075) < 1e-4 && std::fabs(wrong - 0.1716) < 1e-4, "orientation", right, wrong);
  }
  // ---- odw_set_coating's validation ----
  {
    const int G = 4, W = 2 * ODW_COAT_LAYERS;
    std::vector<int32_t> mode = {0, ODW_FRESNEL_LOSS, ODW_FRESNEL_SPLIT, 0}, cnt(G, 0);
    std::vector<double> lay((size_t)G * W, 0.0);
    std::string err;
    expect(coating_validate(G, cnt.data(), lay.data(), mode.data(), err) == ODW_OK, "no coating");
    expect(coating_validate(G, cnt.data(), nullptr, mode.data(), err) == ODW_OK, "no coating, no table");
    expect(coating_validate(0, nullptr, nullptr, nullptr, err) == ODW_OK, "none");
    for (int k = 1; k <= ODW_COAT_LAYERS; ++k) {
      cnt.assign(G, 0);
      cnt[1] = k;
      cnt[2] = ODW_COAT_LAYERS + 1 - k;
      for (int g = 1; g <= 2; ++g)
        for (int j = 0; j < cnt[g]; ++j) { lay[(size_t)g * W + 2 * j] = 1.0 + 0.3 * j; lay[(size_t)g * W + 2 * j + 1] = 40.0 * j; }
      expect(coating_validate(G, cnt.data(), lay.data(), mode.data(), err) == ODW_OK, "stacks", k);
      expect(coating_validate(G, cnt.data(), lay.data(), nullptr, err) == ODW_OK, "no modes at hand", k);
      expect(coating_validate(G, cnt.data(), nullptr, mode.data(), err) == ODW_ERR_INVALID, "layers without a table", k);
      for (int g : {0, 3}) {
        std::vector<int32_t> c2 = cnt;
        c2[g] = 1;
        std::vector<double> l2 = lay;
        l2[(size_t)g * W] = 1.38;
        char word[80];
        std::snprintf(word, sizeof word, "group %d: a coating on a group without a Fresnel mode", g);
        expect(refused(coating_validate(G, c2.data(), l2.data(), mode.data(), err), err, word), "no mode", g, k);
      }
    }
    for (int bad : {ODW_COAT_LAYERS + 1, -1, 1 << 20}) {
      std::vector<int32_t> c2(G, 0);
      c2[1] = bad;
      expect(refused(coating_validate(G, c2.data(), lay.data(), mode.data(), err), err, "group 1:") && err.find("layers (a coating has at most 4)") != std::string::npos,
             "layer count", bad);
    }
    cnt.assign(G, 0);
    cnt[2] = 3;
    for (int j = 0; j < 3; ++j) {
      for (double bad : {0.9, 0.0, -1.5, (double)NAN, (double)INFINITY}) {
        std::vector<double> l2((size_t)G * W, 0.0);
        for (int i = 0; i < 3; ++i) { l2[2 * (size_t)W + 2 * i] = 1.4; l2[2 * (size_t)W + 2 * i + 1] = 100.0; }
        l2[2 * (size_t)W + 2 * j] = bad;
        char word[64];
        std::snprintf(word, sizeof word, "group 2: layer %d: index", j);
        expect(refused(coating_validate(G, cnt.data(), l2.data(), mode.data(), err), err, word), "index", j, bad);
      }
      for (double bad : {-1e-9, -100.0, (double)NAN, (double)INFINITY}) {
        std::vector<double> l2((size_t)G * W, 0.0);
        for (int i = 0; i < 3; ++i) { l2[2 * (size_t)W + 2 * i] = 1.4; l2[2 * (size_t)W + 2 * i + 1] = 100.0; }
        l2[2 * (size_t)W + 2 * j + 1] = bad;
        char word[64];
        std::snprintf(word, sizeof word, "group 2: layer %d: thickness", j);
        expect(refused(coating_validate(G, cnt.data(), l2.data(), mode.data(), err), err, word), "thickness", j, bad);
      }
    }
    // rows beyond a group's count are not read as layers: garbage there is no refusal
    {
      std::vector<double> l2((size_t)G * W, -7.0);
      l2[2 * (size_t)W] = 1.38; l2[2 * (size_t)W + 1] = 99.6;
      cnt.assign(G, 0);
      cnt[2] = 1;
      expect(coating_validate(G, cnt.data(), l2.data(), mode.data(), err) == ODW_OK, "rows beyond the count");
    }
    expect(coating_validate(ODW_MAX_GROUPS + 1, cnt.data(), lay.data(), nullptr, err) == ODW_ERR_INVALID, "too many groups");
    expect(coating_validate(-1, cnt.data(), lay.data(), nullptr, err) == ODW_ERR_INVALID, "a negative count");
    expect(coating_validate(G, nullptr, lay.data(), nullptr, err) == ODW_ERR_INVALID, "null counts");
    // a full table
    std::vector<int32_t> all((size_t)ODW_MAX_GROUPS, ODW_COAT_LAYERS), modes((size_t)ODW_MAX_GROUPS, ODW_FRESNEL_LOSS);
    std::vector<double> full((size_t)ODW_MAX_GROUPS * W, 1.5);
    expect(coating_validate(ODW_MAX_GROUPS, all.data(), full.data(), modes.data(), err) == ODW_OK, "every group coated");
  }
  std::printf("coating: %d checks, %d mismatches\n", checks, mismatches);
  return mismatches ? 1 : 0;
}
