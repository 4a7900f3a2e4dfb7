// slope_tables_main.hip -- the slope builder of csrc/odw_build.h (append_slopes) under AddressSanitizer +
// UndefinedBehaviorSanitizer.
//
// A program of its own (tests/test_native_slope_tables.py compiles and runs it; no GPU, no Python, nothing preloaded).
// It feeds the builder tables of 2, 3 and 4096 knots, several tables in one buffer, and a table with a repeated cdf
// knot, in vectors of exactly the size the builder is given (a write or read past either end is the sanitizer's), and
// holds every slope against the division written out here, the layout (pairs untouched, slopes behind them, 0 for the
// last knot of a table) and the interpolation cdf[j] == u ? edge[j] : slope[j] * (u - cdf[j]) + edge[j] against the
// form with the division per sample.
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

void expect(bool ok, const char* what, size_t n_knots, size_t at) {
  if (ok) return;
  ++mismatches;
  std::printf("MISMATCH %s (tables of %zu knots, at %zu)\n", what, n_knots, at);
}

uint64_t bits(double v) {
  uint64_t u;
  std::memcpy(&u, &v, sizeof u);
  return u;
}

// xorshift64*: the same tables on every run
struct Rng {
  uint64_t s;
  double next() {
    s ^= s >> 12; s ^= s << 25; s ^= s >> 27;
    return (double)((s * 2685821237109323ull) >> 11) * (1.0 / 9007199254740992.0);
  }
};

// n_tables tables of n_knots knots: cdf from 0 to 1, non-decreasing, `repeat` knots of every table equal to their
// predecessor; edges increasing
void check(size_t n_tables, size_t n_knots, size_t repeat, uint64_t seed) {
  Rng rng{seed};
  std::vector<double> edges(n_knots), cdf(n_tables * n_knots);
  double e = -1.0;
  for (size_t j = 0; j < n_knots; ++j) { edges[j] = e; e += 0.001 + rng.next(); }
  for (size_t t = 0; t < n_tables; ++t) {
    double* c = &cdf[t * n_knots];
    std::vector<double> w(n_knots, 0.0);
    double sum = 0;
    for (size_t j = 1; j < n_knots; ++j) { w[j] = 0.01 + rng.next(); sum += w[j]; }
    for (size_t k = 0; k < repeat && n_knots > 2; ++k) {           // cells the density vanishes on
      const size_t j = 1 + (size_t)(rng.next() * (double)(n_knots - 2));
      sum -= w[j];
      w[j] = 0.0;
    }
    double run = 0;
    c[0] = 0.0;
    for (size_t j = 1; j < n_knots; ++j) { run += w[j]; c[j] = run / sum; }
    c[n_knots - 1] = 1.0;
    for (size_t j = 1; j < n_knots; ++j) if (c[j] < c[j - 1]) c[j] = c[j - 1];
  }
  std::vector<double> tab(n_tables * n_knots * 2);
  for (size_t t = 0; t < n_tables; ++t)
    for (size_t j = 0; j < n_knots; ++j) { tab[2 * (t * n_knots + j)] = cdf[t * n_knots + j]; tab[2 * (t * n_knots + j) + 1] = edges[j]; }
  const std::vector<double> pairs = tab;
  tab.shrink_to_fit();
  append_slopes(tab, n_tables, n_knots);
  expect(tab.size() == 3 * n_tables * n_knots, "size", n_knots, 0);
  expect(std::memcmp(tab.data(), pairs.data(), pairs.size() * sizeof(double)) == 0, "pairs moved", n_knots, 0);
  const double* slope = tab.data() + 2 * n_tables * n_knots;
  size_t infinite = 0;
  for (size_t t = 0; t < n_tables; ++t) {
    const double* c = &cdf[t * n_knots];
    const double* s = slope + t * n_knots;
    expect(bits(s[n_knots - 1]) == 0, "last knot", n_knots, t);
    for (size_t j = 0; j + 1 < n_knots; ++j) {
      const double den = c[j + 1] - c[j], num = edges[j + 1] - edges[j];
      if (den == 0.0) { expect(std::isinf(s[j]) && s[j] > 0, "repeated knot", n_knots, j); ++infinite; }
      else expect(bits(s[j]) == bits(num / den), "slope", n_knots, j);
    }
    // the kernels' interpolation against the one that divides per sample, at the knots and between them
    for (size_t k = 0; k < 4 * n_knots + 64; ++k) {
      double u = rng.next();
      if (k < n_knots && c[k] < 1.0) u = c[k];
      if (k == n_knots) u = 0.0;
      if (k == n_knots + 1) u = std::nextafter(1.0, 0.0);
      size_t lo = 0, hi = n_knots - 1;
      while (hi - lo > 1) { const size_t mid = (lo + hi) >> 1; if (u >= c[mid]) lo = mid; else hi = mid; }
      const double prod = s[lo] * (u - c[lo]);
      const double got = c[lo] == u ? edges[lo] : prod + edges[lo];
      const double q = (edges[lo + 1] - edges[lo]) / (c[lo + 1] - c[lo]);
      const double prod2 = q * (u - c[lo]);
      const double want = c[lo] == u ? edges[lo] : prod2 + edges[lo];
      expect(bits(got) == bits(want) && std::isfinite(got), "interpolation", n_knots, k);
    }
  }
  std::printf("%zu table(s) of %zu knots, %zu repeated: ok so far (%zu infinite slopes)\n", n_tables, n_knots, repeat, infinite);
}

}  // namespace

int main() {
  check(1, 2, 0, 1);
  check(1, 3, 0, 2);
  check(3, 3, 1, 3);
  check(1, 4096, 0, 4);
  check(5, 4096, 0, 5);
  check(2, 64, 9, 6);                 // repeated knots
  check(1, 4096, 500, 7);
  // 0 / 0: a knot repeated in cdf and edge
  {
    std::vector<double> tab = {0.0, 0.0, 0.5, 1.0, 0.5, 1.0, 1.0, 2.0};
    append_slopes(tab, 1, 4);
    expect(tab.size() == 12 && tab[8] == 2.0 && std::isnan(tab[9]) && tab[10] == 2.0 && tab[11] == 0.0, "0 / 0", 4, 0);
  }
  std::printf("slope tables: %d mismatches\n", mismatches);
  return mismatches ? 1 : 0;
}
