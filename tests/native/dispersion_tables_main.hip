// dispersion_tables_main.hip -- the dispersion and spectrum builders and validators of csrc/odw_build.h (disp_index,
// disp_validate, disp_check_range, spectrum_validate, spectrum_table) under AddressSanitizer + UndefinedBehaviorSanitizer.
//
// A program of its own (tests/test_native_dispersion_tables.py compiles and runs it; no GPU, no Python, nothing
// preloaded).  Every array is a vector of exactly the size the function is given (a read or write past either end is
// the sanitizer's).  The index is held against the formulas written out here in long double (agreement to 4 ulp of
// the double: the two roundings differ) and against the catalogue's N-BK7 numbers; the validators against tables made
// to be refused, one reason each; the spectrum table against the layout the kernels read.
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

const double kBk7[6] = {1.03961212, 0.231792344, 1.01046945, 0.00600069867, 0.0200179144, 103.560653};

long double sellmeier_ld(const double* c, double wl) {
  const long double l = (long double)wl / 1000.0L, l2 = l * l;
  long double s = 1.0L;
  for (int i = 0; i < 3; ++i) s += (long double)c[i] * l2 / (l2 - (long double)c[3 + i]);
  return sqrtl(s);
}

long double cauchy_ld(const double* c, double wl) {
  const long double l = (long double)wl / 1000.0L, l2 = l * l;
  return (long double)c[0] + (long double)c[1] / l2 + (long double)c[2] / (l2 * l2);
}

}  // namespace

int main() {
  // ---- the index ----
  {
    std::vector<double> bk7(kBk7, kBk7 + 6), cau = {1.5950, 0.0105, 0.0002, 0.0, 0.0, 0.0};
    for (int k = 0; k < 1000; ++k) {
      const double wl = 350.0 + 1650.0 * (double)k / 999.0;
      const double a = disp_index(ODW_DISP_SELLMEIER, bk7.data(), wl), b = disp_index(ODW_DISP_CAUCHY, cau.data(), wl);
      expect(std::fabs((double)((long double)a - sellmeier_ld(bk7.data(), wl))) <= 4 * 2.3e-16 * a, "Sellmeier", a, wl);
      expect(std::fabs((double)((long double)b - cauchy_ld(cau.data(), wl))) <= 4 * 2.3e-16 * b, "Cauchy", b, wl);
    }
    const double lines[3] = {486.1327, 587.5618, 656.2725}, cat[3] = {1.52238, 1.51680, 1.51432};
    for (int k = 0; k < 3; ++k) expect(std::fabs(disp_index(ODW_DISP_SELLMEIER, bk7.data(), lines[k]) - cat[k]) < 5e-6, "catalogue", cat[k]);
    expect(std::isnan(disp_index(ODW_DISP_NONE, bk7.data(), 500.0)), "kind 0");
  }
  // ---- odw_set_dispersion's validation ----
  {
    const int G = 5;
    // groups: lens, mirror, reflection grating, transmission grating, absorber
    std::vector<int32_t> gi = {ODW_OPT_LENS, 0, 0, 1, ODW_OPT_MIRROR, 0, 0, 1, ODW_OPT_GRATING, 0, 0, 1, ODW_OPT_GRATING, 0, 1, 1, ODW_OPT_ABSORBER, 1, 0, 1};
    std::vector<int32_t> kind(G, 0);
    std::vector<double> coef((size_t)G * ODW_DISP_COEFS, 0.0);
    std::string err;
    for (int g = 0; g < G; ++g) std::memcpy(&coef[(size_t)g * ODW_DISP_COEFS], kBk7, sizeof kBk7);
    expect(disp_validate(G, kind.data(), coef.data(), gi.data(), err) == ODW_OK, "all constant");
    kind[0] = ODW_DISP_SELLMEIER; kind[3] = ODW_DISP_CAUCHY;
    expect(disp_validate(G, kind.data(), coef.data(), gi.data(), err) == ODW_OK, "lens and transmission grating");
    expect(disp_validate(0, nullptr, nullptr, nullptr, err) == ODW_OK, "none");
    for (int g : {1, 2, 4}) {
      std::vector<int32_t> k2(G, 0);
      k2[g] = ODW_DISP_SELLMEIER;
      expect(refused(disp_validate(G, k2.data(), coef.data(), gi.data(), err), err, "neither a lens nor a transmission grating"), "group type", g);
      expect(disp_validate(G, k2.data(), coef.data(), nullptr, err) == ODW_OK, "no types at hand", g);
    }
    { std::vector<int32_t> k2 = kind; k2[0] = 3; expect(refused(disp_validate(G, k2.data(), coef.data(), gi.data(), err), err, "unknown dispersion kind 3"), "kind 3"); }
    { std::vector<int32_t> k2 = kind; k2[0] = -1; expect(refused(disp_validate(G, k2.data(), coef.data(), gi.data(), err), err, "unknown dispersion kind"), "kind -1"); }
    for (int k = 0; k < ODW_DISP_COEFS; ++k) {
      std::vector<double> c2 = coef;
      c2[(size_t)3 * ODW_DISP_COEFS + k] = k & 1 ? INFINITY : std::nan("");
      expect(refused(disp_validate(G, kind.data(), c2.data(), gi.data(), err), err, "group 3: non-finite"), "non-finite", k);
      c2 = coef;
      c2[(size_t)1 * ODW_DISP_COEFS + k] = std::nan("");      // (a group of kind 0: its coefficients are nobody's business)
      expect(disp_validate(G, kind.data(), c2.data(), gi.data(), err) == ODW_OK, "unused row", k);
    }
    expect(disp_validate(ODW_MAX_GROUPS + 1, kind.data(), coef.data(), nullptr, err) == ODW_ERR_INVALID, "too many groups");
    expect(disp_validate(G, nullptr, coef.data(), nullptr, err) == ODW_ERR_INVALID, "null kind");
    // ---- the range check ----
    kind[3] = 0;
    expect(disp_check_range(G, kind.data(), coef.data(), 350.0, 2000.0, err) == ODW_OK, "N-BK7 over its range");
    expect(disp_check_range(G, kind.data(), coef.data(), 587.5618, 587.5618, err) == ODW_OK, "one wavelength");
    expect(refused(disp_check_range(G, kind.data(), coef.data(), 120.0, 400.0, err), err, "group 0: Sellmeier pole at 141.4"), "pole C2");
    expect(refused(disp_check_range(G, kind.data(), coef.data(), 70.0, 80.0, err), err, "group 0: Sellmeier pole at 77.4"), "pole C1");
    expect(refused(disp_check_range(G, kind.data(), coef.data(), 9000.0, 11000.0, err), err, "Sellmeier pole at 10176"), "pole C3");
    expect(refused(disp_check_range(G, kind.data(), coef.data(), 60.0, 70.0, err), err, "group 0: index"), "no index below the first pole");
    expect(refused(disp_check_range(G, kind.data(), coef.data(), 0.0, 500.0, err), err, "finite and > 0"), "lo = 0");
    expect(refused(disp_check_range(G, kind.data(), coef.data(), 600.0, 500.0, err), err, "finite and > 0"), "hi < lo");
    expect(refused(disp_check_range(G, kind.data(), coef.data(), 500.0, INFINITY, err), err, "finite and > 0"), "hi = inf");
    std::vector<double> low((size_t)G * ODW_DISP_COEFS, 0.0);
    low[0] = 0.9; low[1] = 0.001;
    kind[0] = ODW_DISP_CAUCHY;
    expect(refused(disp_check_range(G, kind.data(), low.data(), 500.0, 600.0, err), err, "group 0: index 0.9"), "index below 1");
    // a negative C has no pole
    std::vector<double> neg(coef);
    neg[3] = -0.006;
    kind[0] = ODW_DISP_SELLMEIER;
    expect(disp_check_range(G, kind.data(), neg.data(), 50.0, 120.0, err) == ODW_OK, "negative C1: no pole");
  }
  // ---- spectra ----
  {
    std::string err;
    std::vector<double> wl = {486.1327, 587.5618, 656.2725}, cdf = {0.25, 0.75, 1.0};
    expect(spectrum_validate(ODW_SPECTRUM_LINES, 3, wl.data(), cdf.data(), err) == ODW_OK, "three lines");
    std::vector<double> one_w = {550.0}, one_c = {1.0};
    expect(spectrum_validate(ODW_SPECTRUM_LINES, 1, one_w.data(), one_c.data(), err) == ODW_OK, "one line");
    expect(refused(spectrum_validate(ODW_SPECTRUM_DENSITY, 1, one_w.data(), one_c.data(), err), err, "bad argument"), "a density of one knot");
    expect(refused(spectrum_validate(3, 3, wl.data(), cdf.data(), err), err, "unknown mode"), "mode 3");
    expect(refused(spectrum_validate(ODW_SPECTRUM_LINES, 3, nullptr, cdf.data(), err), err, "bad argument"), "null");
    expect(refused(spectrum_validate(ODW_SPECTRUM_DENSITY, 3, wl.data(), cdf.data(), err), err, "run from 0 to 1"), "density from 0.25");
    { std::vector<double> w2 = {656.0, 587.0, 486.0}; expect(refused(spectrum_validate(ODW_SPECTRUM_LINES, 3, w2.data(), cdf.data(), err), err, "not ascending"), "descending"); }
    { std::vector<double> w2 = {486.0, 486.0, 656.0}; expect(refused(spectrum_validate(ODW_SPECTRUM_LINES, 3, w2.data(), cdf.data(), err), err, "not ascending"), "repeated"); }
    { std::vector<double> w2 = {-486.0, 587.0, 656.0}; expect(refused(spectrum_validate(ODW_SPECTRUM_LINES, 3, w2.data(), cdf.data(), err), err, "> 0"), "negative"); }
    { std::vector<double> w2 = {486.0, std::nan(""), 656.0}; expect(spectrum_validate(ODW_SPECTRUM_LINES, 3, w2.data(), cdf.data(), err) == ODW_ERR_INVALID, "nan"); }
    { std::vector<double> c2 = {0.25, 0.2, 1.0}; expect(refused(spectrum_validate(ODW_SPECTRUM_LINES, 3, wl.data(), c2.data(), err), err, "not monotone"), "cdf falls"); }
    { std::vector<double> c2 = {0.25, 0.75, 0.99}; expect(refused(spectrum_validate(ODW_SPECTRUM_LINES, 3, wl.data(), c2.data(), err), err, "run from 0 to 1"), "cdf ends below 1"); }
    { std::vector<double> c2 = {0.25, 1.5, 1.0}; expect(spectrum_validate(ODW_SPECTRUM_LINES, 3, wl.data(), c2.data(), err) == ODW_ERR_INVALID, "cdf above 1"); }
    { std::vector<double> c2 = {0.25, std::nan(""), 1.0}; expect(spectrum_validate(ODW_SPECTRUM_LINES, 3, wl.data(), c2.data(), err) == ODW_ERR_INVALID, "cdf nan"); }
    // the device table: pairs, then slopes (numpy.interp's)
    for (int n : {2, 3, 4097}) {
      std::vector<double> e((size_t)n), c((size_t)n);
      for (int j = 0; j < n; ++j) { e[(size_t)j] = 400.0 + 300.0 * (double)j / (double)(n - 1); c[(size_t)j] = (double)j / (double)(n - 1); }
      c[(size_t)n - 1] = 1.0;
      expect(spectrum_validate(ODW_SPECTRUM_DENSITY, n, e.data(), c.data(), err) == ODW_OK, "a density table", n);
      std::vector<double> tab;
      spectrum_table(n, e.data(), c.data(), tab);
      expect(tab.size() == 3 * (size_t)n, "table size", n);
      for (int j = 0; j < n; ++j) {
        expect(tab[2 * (size_t)j] == c[(size_t)j] && tab[2 * (size_t)j + 1] == e[(size_t)j], "pairs", j);
        const double want = j + 1 < n ? (e[(size_t)j + 1] - e[(size_t)j]) / (c[(size_t)j + 1] - c[(size_t)j]) : 0.0;
        expect(tab[2 * (size_t)n + (size_t)j] == want, "slope", j);
      }
    }
  }
  std::printf("dispersion tables: %d checks, %d mismatches\n", checks, mismatches);
  return mismatches ? 1 : 0;
}
