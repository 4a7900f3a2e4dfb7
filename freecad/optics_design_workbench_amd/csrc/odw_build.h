// odw_build.h -- a scene's host tables and its acceleration structures, computed on the host.
//
// Descriptor -> HostScene (scene_host_tables) -> boxes, headers, dead primitives (compute_boxes) -> SceneAccel
// (build_accel): the rectilinear grid, the SAH binary tree and the eight-wide tree with its leaf records, as plain
// vectors in the layouts the kernels read.  No device context, no HIP call, no getenv: odw_capi.hip uploads what comes
// out of here (upload_accel), tests/native/build_tables_main.hip runs it under a CPU sanitizer.
// Included after odw_kernels.hip, odw_grid.hip and odw_mesh.hip, whose layout constants it uses.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <map>
#include <string>
#include <utility>
#include <vector>

namespace {

using namespace odw;

// what scene_host_tables and compute_boxes make of a descriptor
struct HostScene {
  std::vector<double> prim_f64;
  std::vector<int32_t> prim_i32;
  std::vector<int32_t> cond;              // prim | opens a clause << 30 | inside << 31
  std::vector<double> prim_hdr;           // 64-byte headers (boxes + the four integers): compute_boxes
  std::vector<char> dead;                 // primitives no ray can meet (no face, or an empty box): compute_boxes
  std::vector<double> group_f64, group_gdir;
  std::vector<int32_t> group_i32;
  std::vector<uint64_t> seq;
  std::vector<double> asph;               // ODW_ASPH_ROW doubles per primitive (aspheres: coefficients, bounds), or empty: no asphere
  bool lean = false;                      // no grating group, no finite absorption length: LEAN kernels
  // the scalars of DeviceScene that are known here
  int32_t n_prims = 0, n_groups = 0, seq_enabled = 0, seq_len = 0;
  uint64_t all_mask = 0, ignore_mask = 0;
};

inline int refuse(std::string& err, int code, const char* msg) {
  err = msg;
  return code;
}

// ---- validation and the host copies of a descriptor's tables ---------------------------------
// a condition as the kernels read it (odw_device.h: cond_operand, cond_opens, the sign = must be inside)
int32_t pack_cond(int32_t prim, int32_t inside) {
  return (int32_t)((uint32_t)prim | ((uint32_t)(inside >> 1) & 1u) << 30 | ((uint32_t)inside & 1u) << 31);
}

// every list that opens a clause after its first word opens one with its first word too (offsets already checked)
bool clauses_marked(const int32_t* cond_off, int n, const std::vector<int32_t>& cond) {
  for (int p = 0; p < n; ++p) {
    const int off = cond_off[p], end = cond_off[p + 1];
    if (end <= off || cond_opens(cond[off])) continue;
    for (int c = off + 1; c < end; ++c)
      if (cond_opens(cond[c])) return false;
  }
  return true;
}

// ---- sampler tables --------------------------------------------------------------------------
// The slope of segment j of an inverse-CDF table, (edge[j+1] - edge[j]) / (cdf[j+1] - cdf[j]): what numpy.interp
// computes per sample and the kernels used to compute per ray.  A plain double division, correctly rounded like
// the device's, so the bits are the same.  A repeated cdf knot divides by zero as numpy does (+-inf, 0 / 0 = nan: no
// sample ever lands on such a segment, the search takes the last knot with cdf <= u).
inline double table_slope(double cdf0, double edge0, double cdf1, double edge1) {
  const double num = edge1 - edge0, den = cdf1 - cdf0;
  if (den == 0.0) return num > 0.0 ? INFINITY : num < 0.0 ? -INFINITY : std::numeric_limits<double>::quiet_NaN();
  return num / den;
}

// `tab` holds n_tables tables of n_knots interleaved (cdf, edge) pairs each; behind them go the slopes, one double
// per knot in the same order (the last knot of a table has no segment: 0).  The pairs stay where they are, 16-byte
// aligned; inv_cdf (odw_kernels.hip) reads the slope of the knot it found with one 8-byte load.
inline void append_slopes(std::vector<double>& tab, size_t n_tables, size_t n_knots) {
  const size_t n = n_tables * n_knots;
  tab.resize(3 * n);
  for (size_t t = 0; t < n_tables; ++t)
    for (size_t j = 0; j < n_knots; ++j) {
      const double* a = &tab[2 * (t * n_knots + j)];
      tab[2 * n + t * n_knots + j] = j + 1 < n_knots ? table_slope(a[0], a[1], a[2], a[3]) : 0.0;
    }
}

// ---- even aspheres ---------------------------------------------------------------------------
// sag s(u) of the asphere (c, K, a_1 .. a_8) at u = rho^2, as the definition reads (the radicand floored at 0)
inline double asph_sag(double c, double K, const double* co, double u) {
  double pl = 0.0;
  for (int i = ODW_ASPH_COEFS - 1; i >= 0; --i) pl = pl * u + co[i];
  return c * u / (1.0 + std::sqrt(std::max(1.0 - (1.0 + K) * c * c * u, 0.0))) + pl * u;
}
constexpr int kAsphSamples = 1024;       // samples of the sag on [0, rim]: the height check, the lowest sag

// The row of the asphere table for par = c, K, H, rim and the coefficients co: a_1 .. a_8, then M >= max(|s_rr|, |s_r / r|)
// and L >= |s_r| over the disc rho <= rim (1 + 1e-3), the conservative lowest sag (the box), a spare word.  Term by
// term in absolute values: conic part s_r = c rho / q, s_r / rho = c / q, s_rr = c / q^3 with q >= q_min on the disc;
// polynomial part s_r = sum 2 i a_i rho^(2i-1), s_rr = sum 2 i (2 i - 1) a_i rho^(2i-2) (which bounds s_r / rho too).
// Returns the largest sampled sag plus the slope bound times half the sample pitch: what H must lie above.
inline double asph_row(const double* par, const double* co, double* row) {
  const double c = par[0], K = par[1], rim = par[3];
  const double rmax = rim * (1.0 + 1e-3), umax = rmax * rmax;
  const double qmin = std::sqrt(std::max(1.0 - std::max(1.0 + K, 0.0) * c * c * umax, 1e-4));
  double M = std::fabs(c) / (qmin * qmin * qmin), L = std::fabs(c) * rmax / qmin;
  double up = 1.0;                                   // u^(i-1)
  for (int i = 1; i <= ODW_ASPH_COEFS; ++i) {
    M += 2.0 * i * (2.0 * i - 1.0) * std::fabs(co[i - 1]) * up;
    L += 2.0 * i * std::fabs(co[i - 1]) * up * rmax;
    up *= umax;
  }
  M *= 1.0 + 1e-12; L *= 1.0 + 1e-12;                // (the sums' own rounding)
  double smax = -INFINITY, smin = INFINITY;
  for (int k = 0; k <= kAsphSamples; ++k) {
    const double rho = rim * (double)k / (double)kAsphSamples, sg = asph_sag(c, K, co, rho * rho);
    smax = std::max(smax, sg);
    smin = std::min(smin, sg);
  }
  const double half = L * 0.5 * rim / (double)kAsphSamples;
  for (int i = 0; i < ODW_ASPH_COEFS; ++i) row[i] = co[i];
  row[8] = M; row[9] = L; row[10] = smin - half; row[11] = 0.0;
  return smax + half;
}

// ---- dispersion and spectra -------------------------------------------------------------------
// The index of a glass at wavelength_nm.  The order of IEEE operations is fixed, none of them contracted -- the
// device twin (odw_kernels.hip: disp_index_dev) performs the same sequence, and so does the numpy expression
// the tests hold both against:
//   l  = wavelength_nm / 1000          l2 = l * l
//   Sellmeier: s = 1; for i = 0, 1, 2 in this order: s = s + (B_i * l2) / (l2 - C_i);  n = sqrt(s)
//   Cauchy:    l4 = l2 * l2;  n = (A + B / l2) + C / l4
// kind 0 (and anything unknown, which the validation refuses before it gets here): NaN.
inline double disp_index(int kind, const double* coef, double wavelength_nm) {
#pragma clang fp contract(off)
  const double l = wavelength_nm / 1000.0;
  const double l2 = l * l;
  if (kind == ODW_DISP_SELLMEIER) {
    double s = 1.0;
    for (int i = 0; i < 3; ++i) {
      const double num = coef[i] * l2, den = l2 - coef[3 + i];
      s = s + num / den;
    }
    return std::sqrt(s);
  }
  if (kind == ODW_DISP_CAUCHY) {
    const double l4 = l2 * l2;
    const double t1 = coef[1] / l2, t2 = coef[2] / l4;
    return (coef[0] + t1) + t2;
  }
  return std::numeric_limits<double>::quiet_NaN();
}

// The band of a wavelength among n_edges strictly increasing edges (odw_set_detector_bands), numpy.histogram's rule:
// e_b <= wl < e_(b+1), wl == e_K in band K - 1, -1 outside [e_0, e_K] and for NaN.  Plain float64 comparisons -- the
// device twin (odw_kernels.hip: band_index_dev) is the same expression, and numpy.searchsorted(edges, wl, 'right') - 1
// with the last edge folded in is what the tests hold both against.
inline int band_index(const double* edges, int n_edges, double wl) {
  int c = 0;
  for (int k = 0; k < n_edges; ++k) c += wl >= edges[k] ? 1 : 0;
  return c == n_edges ? (wl == edges[n_edges - 1] ? n_edges - 2 : -1) : c - 1;
}

// odw_set_detector_bands' check of the edges (`who`: the entry point named in the message)
inline int bands_validate(const char* who, int n_edges, const double* edges, std::string& err) {
  char buf[200];
  if (n_edges < 2 || !edges) {
    std::snprintf(buf, sizeof buf, "%s: band edges: at least two edges (one band) are needed", who);
    err = buf;
    return ODW_ERR_INVALID;
  }
  if (n_edges - 1 > ODW_BAND_MAX) {
    std::snprintf(buf, sizeof buf, "%s: %d bands: a detector takes at most ODW_BAND_MAX = %d", who, n_edges - 1, ODW_BAND_MAX);
    err = buf;
    return ODW_ERR_INVALID;
  }
  for (int k = 0; k < n_edges; ++k) {
    const char* what = !std::isfinite(edges[k]) ? "is not finite" : !(edges[k] > 0) ? "is not positive"
                       : (k > 0 && !(edges[k] > edges[k - 1])) ? "is not above its predecessor (edges must be strictly increasing)" : nullptr;
    if (what) {
      std::snprintf(buf, sizeof buf, "%s: band edge %d (%.17g nm) %s", who, k, edges[k], what);
      err = buf;
      return ODW_ERR_INVALID;
    }
  }
  return ODW_OK;
}

// odw_set_dispersion's check of kind / coef; group_i32 (may be null: no scene at hand) adds the groups' types
inline int disp_validate(int n_groups, const int32_t* kind, const double* coef, const int32_t* group_i32, std::string& err) {
  if (n_groups < 0 || n_groups > ODW_MAX_GROUPS || (n_groups && (!kind || !coef)))
    return refuse(err, ODW_ERR_INVALID, "odw_set_dispersion: bad argument");
  for (int g = 0; g < n_groups; ++g) {
    if (kind[g] == ODW_DISP_NONE) continue;
    char buf[160];
    if (kind[g] != ODW_DISP_SELLMEIER && kind[g] != ODW_DISP_CAUCHY) {
      std::snprintf(buf, sizeof buf, "odw_set_dispersion: group %d: unknown dispersion kind %d", g, (int)kind[g]);
      err = buf;
      return ODW_ERR_INVALID;
    }
    for (int k = 0; k < ODW_DISP_COEFS; ++k)
      if (!std::isfinite(coef[ODW_DISP_COEFS * g + k])) {
        std::snprintf(buf, sizeof buf, "odw_set_dispersion: group %d: non-finite dispersion coefficient", g);
        err = buf;
        return ODW_ERR_INVALID;
      }
    if (group_i32) {
      const int t = group_i32[4 * g], gt = group_i32[4 * g + 2];
      if (!(t == ODW_OPT_LENS || (t == ODW_OPT_GRATING && gt == 1))) {
        std::snprintf(buf, sizeof buf, "odw_set_dispersion: group %d: a dispersion on a group that is neither a lens nor a transmission grating", g);
        err = buf;
        return ODW_ERR_INVALID;
      }
    }
  }
  return ODW_OK;
}

// The check before a launch: every dispersive group's index finite and >= 1 over [lo_nm, hi_nm] (kDispSamples evenly
// spaced wavelengths, the ends included; a Sellmeier index is monotone between its poles for positive B, C, so the ends
// decide there -- the samples between are for signs a catalogue does not print), no Sellmeier pole sqrt(C_i) inside
constexpr int kDispSamples = 33;
inline int disp_check_range(int n_groups, const int32_t* kind, const double* coef, double lo_nm, double hi_nm, std::string& err) {
  if (!(lo_nm > 0) || !(hi_nm >= lo_nm) || !std::isfinite(hi_nm)) return refuse(err, ODW_ERR_INVALID, "dispersion: wavelengths must be finite and > 0");
  for (int g = 0; g < n_groups; ++g) {
    if (kind[g] == ODW_DISP_NONE) continue;
    const double* c = coef + ODW_DISP_COEFS * g;
    char buf[200];
    if (kind[g] == ODW_DISP_SELLMEIER)
      for (int i = 0; i < 3; ++i) {
        if (!(c[3 + i] > 0)) continue;
        const double pole = 1000.0 * std::sqrt(c[3 + i]);
        if (pole >= lo_nm && pole <= hi_nm) {
          std::snprintf(buf, sizeof buf, "dispersion: group %d: Sellmeier pole at %.6g nm inside the wavelength range [%.6g, %.6g] nm", g, pole, lo_nm, hi_nm);
          err = buf;
          return ODW_ERR_INVALID;
        }
      }
    // (Cauchy: n = A + B x + C x^2 in x = 1 / lambda^2 has one extremum, at x = -B / (2 C): with the ends, it decides
    //  exactly -- judged in place of the last sample but one)
    double extremum_nm = 0.0;
    if (kind[g] == ODW_DISP_CAUCHY && c[2] != 0.0) {
      const double x = -c[1] / (2.0 * c[2]);
      if (x > 0.0) extremum_nm = 1000.0 / std::sqrt(x);
      if (!(extremum_nm >= lo_nm && extremum_nm <= hi_nm)) extremum_nm = 0.0;
    }
    for (int k = 0; k < kDispSamples; ++k) {
      double w = k == kDispSamples - 1 ? hi_nm : lo_nm + (hi_nm - lo_nm) * (double)k / (double)(kDispSamples - 1);
      if (k == kDispSamples - 2 && extremum_nm > 0.0) w = extremum_nm;
      const double n = disp_index(kind[g], c, w);
      if (!std::isfinite(n) || !(n >= 1.0)) {
        std::snprintf(buf, sizeof buf, "dispersion: group %d: index %.6g at %.6g nm (must be finite and >= 1)", g, n, w);
        err = buf;
        return ODW_ERR_INVALID;
      }
    }
  }
  return ODW_OK;
}

// odw_set_spectrum's validation (include/odw_trace.h says what the two modes hold)
inline int spectrum_validate(int mode, int n, const double* wl, const double* cdf, std::string& err) {
  if (mode != ODW_SPECTRUM_LINES && mode != ODW_SPECTRUM_DENSITY) return refuse(err, ODW_ERR_INVALID, "odw_set_spectrum: unknown mode");
  if (n < (mode == ODW_SPECTRUM_DENSITY ? 2 : 1) || !wl || !cdf) return refuse(err, ODW_ERR_INVALID, "odw_set_spectrum: bad argument");
  for (int j = 0; j < n; ++j) {
    if (!(wl[j] > 0) || !std::isfinite(wl[j])) return refuse(err, ODW_ERR_INVALID, "odw_set_spectrum: wavelengths must be finite and > 0");
    if (j && !(wl[j] > wl[j - 1])) return refuse(err, ODW_ERR_INVALID, "odw_set_spectrum: wavelengths not ascending");
    if (!(cdf[j] >= 0.0 && cdf[j] <= 1.0) || (j && cdf[j] < cdf[j - 1])) return refuse(err, ODW_ERR_INVALID, "odw_set_spectrum: cdf not monotone within [0, 1]");
  }
  if ((mode == ODW_SPECTRUM_DENSITY && cdf[0] != 0.0) || cdf[n - 1] != 1.0)
    return refuse(err, ODW_ERR_INVALID, "odw_set_spectrum: the cdf must run from 0 to 1");
  return ODW_OK;
}

// the device table of a spectrum: n interleaved (cdf, wavelength) pairs, then the segment slopes (append_slopes)
inline void spectrum_table(int n, const double* wl, const double* cdf, std::vector<double>& tab) {
  tab.assign((size_t)n * 2, 0.0);
  for (int j = 0; j < n; ++j) { tab[2 * (size_t)j] = cdf[j]; tab[2 * (size_t)j + 1] = wl[j]; }
  append_slopes(tab, 1, (size_t)n);
}

// ---- Fresnel reflection at lens surfaces ---------------------------------------------------------
// The unpolarised reflectance of a surface between the indices n1 (the side the ray comes from) and n2, cos_i the cosine
// of the angle of incidence and cos_t that of the refracted ray (snells_law: sqrt(root)).  The device twin
// (odw_kernels.hip: fresnel_reflectance_dev) writes the same expressions.
inline double fresnel_reflectance(double n1, double n2, double cos_i, double cos_t) {
  const double a = n1 * cos_i, b = n2 * cos_t, c = n2 * cos_i, e = n1 * cos_t;
  const double rs = (a - b) / (a + b), rp = (c - e) / (c + e);
  return 0.5 * (rs * rs + rp * rp);
}
// ... from the incidence alone, with mu and root as snells_law writes them; 1 under total internal reflection
inline double fresnel_reflectance(double n1, double n2, double cos_i) {
  const double mu = n1 / n2;
  const double root = 1.0 - mu * mu * (1.0 - cos_i * cos_i);
  if (root < 0) return 1.0;
  return fresnel_reflectance(n1, n2, cos_i, std::sqrt(root));
}

// odw_set_fresnel's check of the modes; group_i32 (may be null: no scene at hand) adds the groups' types
inline int fresnel_validate(int n_groups, const int32_t* mode, const int32_t* group_i32, std::string& err) {
  if (n_groups < 0 || n_groups > ODW_MAX_GROUPS || (n_groups && !mode))
    return refuse(err, ODW_ERR_INVALID, "odw_set_fresnel: bad argument");
  for (int g = 0; g < n_groups; ++g) {
    if (mode[g] == ODW_FRESNEL_NONE) continue;
    char buf[160];
    if (mode[g] != ODW_FRESNEL_LOSS && mode[g] != ODW_FRESNEL_SPLIT) {
      std::snprintf(buf, sizeof buf, "odw_set_fresnel: group %d: unknown Fresnel mode %d", g, (int)mode[g]);
      err = buf;
      return ODW_ERR_INVALID;
    }
    if (group_i32 && group_i32[4 * g] != ODW_OPT_LENS) {
      std::snprintf(buf, sizeof buf, "odw_set_fresnel: group %d: a Fresnel mode on a group that is not a lens", g);
      err = buf;
      return ODW_ERR_INVALID;
    }
  }
  return ODW_OK;
}

// ---- Thin-film coatings on lens groups -----------------------------------------------------------
// The unpolarised reflectance of a surface between n1 and n2 that carries a stack of k non-absorbing layers
// (layers: (index, thickness_nm) each, listed from the group's outside inwards; entering: the ray meets them in that
// order, else in reverse), cos_i and cos_t as for fresnel_reflectance, at wavelength_nm.  Characteristic matrices: all
// indices are real, so every layer matrix and every product is [[a, i b], [i c, d]] with real a, b, c, d -- four real
// recurrences per polarisation; sin, cos of the phase and the cosine in the layer are shared by both.  The p admittances
// of the two media (n / cos) enter R multiplied by cos_i cos_t: no division at grazing incidence.  A layer that would
// hold an evanescent wave: the bare reflectance (frustrated total reflection is not built).  The device twin
// (odw_kernels.hip: coated_reflectance_dev) writes the same expressions.
inline double coated_reflectance(double n1, double n2, double cos_i, double cos_t, bool entering, int k, const double* layers,
                                 double wavelength_nm) {
  if (k <= 0) return fresnel_reflectance(n1, n2, cos_i, cos_t);      // (no stack: the bare surface, bit for bit)
  const double s2 = n1 * n1 * (1.0 - cos_i * cos_i);
  const double w = 6.283185307179586 / wavelength_nm;
  double as = 1.0, bs = 0.0, cs = 0.0, ds = 1.0, ap = 1.0, bp = 0.0, cp = 0.0, dp = 1.0;
  for (int i = 0; i < k; ++i) {
    const int j = entering ? i : k - 1 - i;
    const double nj = layers[2 * j], dj = layers[2 * j + 1];
    const double q = 1.0 - s2 / (nj * nj);
    if (!(q > 0)) return fresnel_reflectance(n1, n2, cos_i, cos_t);
    const double cj = std::sqrt(q);
    const double delta = w * nj * dj * cj;
    const double sd = std::sin(delta), cd = std::cos(delta);
    const double es = nj * cj, ep = nj / cj;
    const double us = sd / es, vs = es * sd, up = sd / ep, vp = ep * sd;
    const double as1 = as * cd - bs * vs, bs1 = as * us + bs * cd, cs1 = cs * cd + ds * vs, ds1 = ds * cd - cs * us;
    const double ap1 = ap * cd - bp * vp, bp1 = ap * up + bp * cd, cp1 = cp * cd + dp * vp, dp1 = dp * cd - cp * up;
    as = as1; bs = bs1; cs = cs1; ds = ds1;
    ap = ap1; bp = bp1; cp = cp1; dp = dp1;
  }
  // s: eta = n cos.  p: eta = n / cos, both sides of the fraction times cos_i cos_t
  const double e0 = n1 * cos_i, e1 = n2 * cos_t;
  const double xs = e0 * as, ys = e1 * ds, zs = e0 * e1 * bs;
  const double rs = ((xs - ys) * (xs - ys) + (zs - cs) * (zs - cs)) / ((xs + ys) * (xs + ys) + (zs + cs) * (zs + cs));
  const double xp = n1 * cos_t * ap, yp = n2 * cos_i * dp, zp = n1 * n2 * bp, tp = cos_i * cos_t * cp;
  const double rp = ((xp - yp) * (xp - yp) + (zp - tp) * (zp - tp)) / ((xp + yp) * (xp + yp) + (zp + tp) * (zp + tp));
  return 0.5 * (rs + rp);
}
// ... from the incidence alone; 1 under total internal reflection
inline double coated_reflectance(double n1, double n2, double cos_i, bool entering, int k, const double* layers, double wavelength_nm) {
  const double mu = n1 / n2;
  const double root = 1.0 - mu * mu * (1.0 - cos_i * cos_i);
  if (root < 0) return 1.0;
  return coated_reflectance(n1, n2, cos_i, std::sqrt(root), entering, k, layers, wavelength_nm);
}

// odw_set_coating's check of the stacks; mode (may be null: no modes at hand) adds the groups' Fresnel modes
inline int coating_validate(int n_groups, const int32_t* n_layers, const double* layers, const int32_t* mode, std::string& err) {
  if (n_groups < 0 || n_groups > ODW_MAX_GROUPS || (n_groups && !n_layers))
    return refuse(err, ODW_ERR_INVALID, "odw_set_coating: bad argument");
  for (int g = 0; g < n_groups; ++g) {
    if (n_layers[g] == 0) continue;
    char buf[200];
    if (n_layers[g] < 0 || n_layers[g] > ODW_COAT_LAYERS) {
      std::snprintf(buf, sizeof buf, "odw_set_coating: group %d: %d layers (a coating has at most %d)", g, (int)n_layers[g], ODW_COAT_LAYERS);
      err = buf;
      return ODW_ERR_INVALID;
    }
    if (!layers) return refuse(err, ODW_ERR_INVALID, "odw_set_coating: bad argument");
    if (mode && mode[g] == ODW_FRESNEL_NONE) {
      std::snprintf(buf, sizeof buf, "odw_set_coating: group %d: a coating on a group without a Fresnel mode", g);
      err = buf;
      return ODW_ERR_INVALID;
    }
    for (int j = 0; j < n_layers[g]; ++j) {
      const double nj = layers[2 * (ODW_COAT_LAYERS * (size_t)g + j)], dj = layers[2 * (ODW_COAT_LAYERS * (size_t)g + j) + 1];
      if (!std::isfinite(nj) || nj < 1.0) {
        std::snprintf(buf, sizeof buf, "odw_set_coating: group %d: layer %d: index %g (finite and at least 1)", g, j, nj);
        err = buf;
        return ODW_ERR_INVALID;
      }
      if (!std::isfinite(dj) || dj < 0.0) {
        std::snprintf(buf, sizeof buf, "odw_set_coating: group %d: layer %d: thickness %g nm (finite and not negative)", g, j, dj);
        err = buf;
        return ODW_ERR_INVALID;
      }
    }
  }
  return ODW_OK;
}

// host half of odw_upload_scene: validation and the host copies of every table.  hs is complete only where the
// answer is ODW_OK
int scene_host_tables(const odw_scene_desc* s, HostScene& hs, std::string& err) {
  if (!s) return refuse(err, ODW_ERR_INVALID, "odw_upload_scene: null argument");
  if (s->n_prims < 0 || s->n_groups < 0 || s->n_groups > ODW_MAX_GROUPS || s->seq_len < 0 ||
      s->seq_len > ODW_MAX_SEQUENCE || s->n_conds < 0 || s->n_conds >= (1 << 24))
    return refuse(err, ODW_ERR_INVALID, "odw_upload_scene: counts out of range");
  if ((s->n_prims > 0 && (!s->prim_type || !s->prim_group || !s->prim_flags || !s->prim_xform || !s->prim_params ||
                          !s->prim_cond_off)) ||
      (s->n_conds > 0 && (!s->cond_prim || !s->cond_inside)) ||
      (s->n_groups > 0 && (!s->group_type || !s->group_ior || !s->group_refl || !s->group_abslen || !s->group_record)) ||
      (s->seq_len > 0 && !s->seq_mask))
    return refuse(err, ODW_ERR_INVALID, "odw_upload_scene: null table pointer");
  const int n = s->n_prims;
  int max_solid = 0;
  for (int p = 0; p < n && s->prim_solid; ++p) max_solid = std::max(max_solid, s->prim_solid[p]);
  hs.prim_f64.assign((size_t)n * 16, 0.0);
  hs.prim_i32.assign((size_t)n * 4, 0);
  for (int p = 0; p < n; ++p) {
    const int type = s->prim_type[p], group = s->prim_group[p];
    if (type < ODW_PRIM_BOX || type > ODW_PRIM_ASPHERE) return refuse(err, ODW_ERR_UNSUPPORTED, "unknown primitive type");
    if (group < 0 || group >= s->n_groups) return refuse(err, ODW_ERR_INVALID, "primitive group out of range");
    const int off = s->prim_cond_off[p], cnt = s->prim_cond_off[p + 1] - off;
    if (off < 0 || cnt < 0 || cnt > 255 || off + cnt > s->n_conds)
      return refuse(err, ODW_ERR_INVALID, "bad condition offsets");
    if (type == ODW_PRIM_TRIANGLE) {
      if (cnt) return refuse(err, ODW_ERR_UNSUPPORTED, "triangles cannot carry trimming conditions");
      const double* v = s->prim_xform + 12 * (size_t)p;
      double* d = &hs.prim_f64[16 * (size_t)p];
      double e1[3], e2[3], e3[3], nn[3];
      for (int k = 0; k < 3; ++k) { d[k] = v[k]; e1[k] = v[3 + k] - v[k]; e2[k] = v[6 + k] - v[k]; e3[k] = e2[k] - e1[k]; }
      nn[0] = e1[1] * e2[2] - e1[2] * e2[1];
      nn[1] = e1[2] * e2[0] - e1[0] * e2[2];
      nn[2] = e1[0] * e2[1] - e1[1] * e2[0];
      const double a2 = std::sqrt(nn[0] * nn[0] + nn[1] * nn[1] + nn[2] * nn[2]);   // twice the area
      if (!(a2 > 0) || !std::isfinite(a2)) return refuse(err, ODW_ERR_INVALID, "degenerate triangle");
      auto len3 = [](const double* x) { return std::sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]); };
      for (int k = 0; k < 3; ++k) { d[3 + k] = e1[k]; d[6 + k] = e2[k]; d[9 + k] = nn[k] / a2; }
      // a point at distance tol outside an edge has barycentric coordinate -tol/altitude
      d[12] = len3(e2) / a2;   // u: distance from edge (v0, v2)
      d[13] = len3(e1) / a2;   // v: distance from edge (v0, v1)
      d[14] = len3(e3) / a2;   // u+v: distance from edge (v1, v2)
      // edges shared with a neighbouring facet of the same face are not widened (sign = marker)
      const int face_edges = s->tri_edges ? s->tri_edges[p] : 7;
      for (int k = 0; k < 3; ++k)
        if (!((face_edges >> k) & 1)) d[12 + k] = -d[12 + k];
      d[15] = 0.0;
    } else {
      std::memcpy(&hs.prim_f64[16 * (size_t)p], s->prim_xform + 12 * (size_t)p, 12 * sizeof(double));
      std::memcpy(&hs.prim_f64[16 * (size_t)p + 12], s->prim_params + 4 * (size_t)p, 4 * sizeof(double));
      if (type == ODW_PRIM_SPHERE) {
        // the kernel intersects spheres without their frame: centre in global coordinates = -R^T t
        const double* m = &hs.prim_f64[16 * (size_t)p];
        for (int k = 0; k < 3; ++k)
          hs.prim_f64[16 * (size_t)p + 13 + k] = -(m[k] * m[3] + m[4 + k] * m[7] + m[8 + k] * m[11]);
      }
      if (type == ODW_PRIM_PARABOLOID) {
        double* par = &hs.prim_f64[16 * (size_t)p + 12];
        if (!(par[0] > 0) || !(par[1] > 0)) return refuse(err, ODW_ERR_INVALID, "paraboloid: focal length and height must be positive");
        par[2] = 2.0 * std::sqrt(par[0] * par[1]);            // rim radius at z = H
      }
      if (type == ODW_PRIM_ELLIPSOID) {
        // one face and no caps: a descriptor that asks for faces 1 or 2 (the caps of the other quadrics) describes a
        // solid this kind is not
        if (((s->prim_flags[p] >> ODW_FACEMASK_SHIFT) & 0xff) & ~1)
          return refuse(err, ODW_ERR_UNSUPPORTED, "ellipsoid: one face (bit 0 of the face mask), it has no caps");
        const double* par = &hs.prim_f64[16 * (size_t)p + 12];
        for (int k = 0; k < 3; ++k)
          if (!(par[k] > 0) || !std::isfinite(par[k])) return refuse(err, ODW_ERR_INVALID, "ellipsoid: the three radii must be positive");
      }
      if (type == ODW_PRIM_CONICOID) {
        // faces 0 (the conic surface) and 2 (the cap z = H); there is no face 1, the vertex is a point
        if (((s->prim_flags[p] >> ODW_FACEMASK_SHIFT) & 0xff) & ~5)
          return refuse(err, ODW_ERR_UNSUPPORTED, "conicoid: faces 0 (surface) and 2 (cap at z = H) only");
        double* par = &hs.prim_f64[16 * (size_t)p + 12];
        const double R = par[0], K = par[1], H = par[2];
        if (!(R > 0) || !std::isfinite(R) || !std::isfinite(K) || !(H > 0) || !std::isfinite(H))
          return refuse(err, ODW_ERR_INVALID, "conicoid: vertex radius and height must be positive and finite, the conic constant finite");
        // (K > -1: the solid ends at or before the equator z = R / (1 + K), where the surface stops being a graph over rho)
        if (K > -1.0 && !(H <= R / (1.0 + K)))
          return refuse(err, ODW_ERR_INVALID, "conicoid: for K > -1 the height must not exceed R / (1 + K)");
        const double rim2 = 2.0 * R * H - (1.0 + K) * H * H;
        if (!(rim2 > 0) || !std::isfinite(rim2)) return refuse(err, ODW_ERR_INVALID, "conicoid: no rim at this height");
        par[3] = std::sqrt(rim2);                              // rim radius at z = H
      }
      if (type == ODW_PRIM_ASPHERE) {
        // faces 0 (the asphere), 1 (the wall rho = rim), 2 (the cap z = H)
        if (((s->prim_flags[p] >> ODW_FACEMASK_SHIFT) & 0xff) & ~7)
          return refuse(err, ODW_ERR_UNSUPPORTED, "asphere: faces 0 (surface), 1 (wall) and 2 (cap at z = H) only");
        // (a descriptor without the table is the descriptor of before the field, in which the kind does not exist)
        if (!s->prim_coef) return refuse(err, ODW_ERR_UNSUPPORTED, "asphere: the scene holds an asphere and no coefficients (prim_coef is null): unknown primitive type");
        const double* par = &hs.prim_f64[16 * (size_t)p + 12];
        const double* co = s->prim_coef + ODW_ASPH_COEFS * (size_t)p;
        bool finite = true;
        for (int k = 0; k < 4; ++k) finite &= std::isfinite(par[k]);
        for (int k = 0; k < ODW_ASPH_COEFS; ++k) finite &= std::isfinite(co[k]);
        if (!finite) return refuse(err, ODW_ERR_INVALID, "asphere: curvature, conic constant, height, semi-diameter and coefficients must be finite");
        if (!(par[3] > 0)) return refuse(err, ODW_ERR_INVALID, "asphere: the semi-diameter must be positive");
        // (the conic part stays a graph of finite slope over the whole disc, with room for the tolerance)
        if (!((1.0 + par[1]) * par[0] * par[0] * par[3] * par[3] <= 0.98))
          return refuse(err, ODW_ERR_INVALID, "asphere: (1 + K) c^2 rim^2 must not exceed 0.98");
        if (hs.asph.empty()) hs.asph.assign((size_t)n * ODW_ASPH_ROW, 0.0);
        const double top = asph_row(par, co, &hs.asph[ODW_ASPH_ROW * (size_t)p]);
        if (!std::isfinite(top) || !(par[2] > top))
          return refuse(err, ODW_ERR_INVALID, "asphere: the height must lie above the largest sag on [0, rim]");
      }
    }
    hs.prim_i32[4 * p] = type;
    hs.prim_i32[4 * p + 1] = group;
    // flags | facemask << 8 in the low half, solid id above; scenes with more solids than fit lose the
    // convex-solid shortcut, nothing else
    const int solid = s->prim_solid ? s->prim_solid[p] : 0;
    const bool fits = s->prim_solid && solid >= 0 && solid < 0x7fff && max_solid < 0x7fff;
    // (an asphere never carries the convex-solid hint: a polynomial profile need not be convex)
    hs.prim_i32[4 * p + 2] = ((s->prim_flags[p] & 0xffff & ~ODW_FLAG_ISOLATED) & (fits && type != ODW_PRIM_ASPHERE ? ~0 : ~ODW_FLAG_CONVEX)) | ((fits ? solid : 0x7fff) << ODW_SOLID_SHIFT);
    hs.prim_i32[4 * p + 3] = off | (cnt << 24);
  }
  std::vector<int32_t> cond((size_t)std::max(1, s->n_conds), 0);
  for (int c = 0; c < s->n_conds; ++c) {
    if (s->cond_prim[c] < 0 || s->cond_prim[c] >= n || s->cond_prim[c] >= (1 << 30))
      return refuse(err, ODW_ERR_INVALID, "condition primitive out of range");
    if (s->prim_type[s->cond_prim[c]] == ODW_PRIM_TRIANGLE)
      return refuse(err, ODW_ERR_UNSUPPORTED, "trimming against a triangle (no inside/outside of a facet)");
    if (s->cond_inside[c] < 0 || s->cond_inside[c] > 3)
      return refuse(err, ODW_ERR_INVALID, "cond_inside: bit 0 inside, bit 1 opens a clause; nothing else");
    cond[c] = pack_cond(s->cond_prim[c], s->cond_inside[c]);
  }
  if (!clauses_marked(s->prim_cond_off, n, cond))
    return refuse(err, ODW_ERR_INVALID, "a trimming list of several clauses must mark its first condition too");
  hs.cond = cond;
  std::vector<double> gf(ODW_MAX_GROUPS * 4, 0.0), gd(ODW_MAX_GROUPS * 3, 0.0);
  std::vector<int32_t> gi(ODW_MAX_GROUPS * 4, 0);
  hs.lean = true;
  for (int g = 0; g < s->n_groups; ++g)
    if (s->group_type[g] == ODW_OPT_GRATING || !(s->group_abslen[g] == INFINITY)) hs.lean = false;
  for (int g = 0; g < s->n_groups; ++g) {
    if (s->group_type[g] < ODW_OPT_MIRROR || s->group_type[g] > ODW_OPT_VACUUM)
      return refuse(err, ODW_ERR_INVALID, "unknown optical type");
    gf[4 * g] = s->group_ior[g];
    gf[4 * g + 1] = s->group_refl[g];
    gf[4 * g + 2] = s->group_abslen[g];
    gf[4 * g + 3] = s->group_grating_lpm ? s->group_grating_lpm[g] : 1000.0;
    gi[4 * g] = s->group_type[g];
    gi[4 * g + 1] = s->group_record[g] ? 1 : 0;
    gi[4 * g + 2] = s->group_grating_type ? s->group_grating_type[g] : 0;
    gi[4 * g + 3] = s->group_grating_order ? s->group_grating_order[g] : 1;
    for (int k = 0; k < 3; ++k) gd[3 * g + k] = s->group_grating_dir ? s->group_grating_dir[3 * g + k] : (k == 2);
  }
  std::vector<uint64_t> seq((size_t)std::max(1, s->seq_len), 0);
  for (int i = 0; i < s->seq_len; ++i) seq[i] = s->seq_mask[i];
  hs.group_f64 = gf;
  hs.group_i32 = gi;
  hs.group_gdir = gd;
  hs.seq = seq;
  hs.n_prims = n;
  hs.n_groups = s->n_groups;
  hs.seq_enabled = s->seq_enabled ? 1 : 0;
  hs.seq_len = s->seq_len;
  hs.all_mask = (s->n_groups >= 64) ? ~0ull : ((1ull << s->n_groups) - 1ull);
  hs.ignore_mask = s->ignore_mask;
  return ODW_OK;
}

// ---- primitive bounding boxes in global coordinates -----------------------
// (z_min: an asphere's lowest sag, from its table row)
void local_bounds(int type, const double* par, double lo[3], double hi[3], double z_min = 0.0) {
  switch (type) {
    case ODW_PRIM_BOX:
      lo[0] = lo[1] = lo[2] = 0; hi[0] = par[0]; hi[1] = par[1]; hi[2] = par[2];
      break;
    case ODW_PRIM_SPHERE:
      for (int i = 0; i < 3; ++i) { lo[i] = -par[0]; hi[i] = par[0]; }
      break;
    case ODW_PRIM_CYLINDER:
      lo[0] = lo[1] = -par[0]; hi[0] = hi[1] = par[0]; lo[2] = 0; hi[2] = par[1];
      break;
    case ODW_PRIM_CONE: {
      const double r = std::max(par[0], par[1]);
      lo[0] = lo[1] = -r; hi[0] = hi[1] = r; lo[2] = 0; hi[2] = par[2];
      break;
    }
    case ODW_PRIM_PARABOLOID: {
      const double r = 2.0 * std::sqrt(std::max(par[0] * par[1], 0.0));
      lo[0] = lo[1] = -r; hi[0] = hi[1] = r; lo[2] = 0; hi[2] = par[1];
      break;
    }
    case ODW_PRIM_ELLIPSOID:
      for (int i = 0; i < 3; ++i) { lo[i] = -par[i]; hi[i] = par[i]; }
      break;
    case ODW_PRIM_CONICOID:   // (0 <= z <= H lies at or before the equator: the rim is the widest parallel)
      lo[0] = lo[1] = -par[3]; hi[0] = hi[1] = par[3]; lo[2] = 0; hi[2] = par[2];
      break;
    case ODW_PRIM_ASPHERE:    // the disc, from the conservative lowest sag to the cap
      lo[0] = lo[1] = -par[3]; hi[0] = hi[1] = par[3]; lo[2] = z_min; hi[2] = par[2];
      break;
    default: {  // torus
      const double r = par[0] + par[1];
      lo[0] = lo[1] = -r; hi[0] = hi[1] = r; lo[2] = -par[1]; hi[2] = par[1];
    }
  }
}

struct Box {
  double lo[3], hi[3];
  void reset() { for (int i = 0; i < 3; ++i) { lo[i] = INFINITY; hi[i] = -INFINITY; } }
  void grow(const Box& o) {
    for (int i = 0; i < 3; ++i) { lo[i] = std::min(lo[i], o.lo[i]); hi[i] = std::max(hi[i], o.hi[i]); }
  }
};

Box world_box(const double* pf, int type, double slack, double z_min = 0.0) {
  Box b;
  b.reset();
  if (type == ODW_PRIM_TRIANGLE) {   // v0, e1, e2 in global coordinates
    for (int i = 0; i < 3; ++i) {
      const double a = pf[i], c1 = pf[i] + pf[3 + i], c2 = pf[i] + pf[6 + i];
      const double s = slack + 1e-9 * (std::fabs(a) + std::fabs(c1) + std::fabs(c2));
      b.lo[i] = std::min(a, std::min(c1, c2)) - s;
      b.hi[i] = std::max(a, std::max(c1, c2)) + s;
    }
    return b;
  }
  double lo[3], hi[3];
  local_bounds(type, pf + 12, lo, hi, z_min);
  for (int c = 0; c < 8; ++c) {
    const double l[3] = {(c & 1) ? hi[0] : lo[0], (c & 2) ? hi[1] : lo[1], (c & 4) ? hi[2] : lo[2]};
    // global = R^T (local - t)
    const double d[3] = {l[0] - pf[3], l[1] - pf[7], l[2] - pf[11]};
    const double g[3] = {pf[0] * d[0] + pf[4] * d[1] + pf[8] * d[2],
                         pf[1] * d[0] + pf[5] * d[1] + pf[9] * d[2],
                         pf[2] * d[0] + pf[6] * d[1] + pf[10] * d[2]};
    for (int i = 0; i < 3; ++i) { b.lo[i] = std::min(b.lo[i], g[i]); b.hi[i] = std::max(b.hi[i], g[i]); }
  }
  for (int i = 0; i < 3; ++i) {
    const double s = slack + 1e-9 * (std::fabs(b.lo[i]) + std::fabs(b.hi[i]));
    b.lo[i] -= s;
    b.hi[i] += s;
  }
  return b;
}

// BVH node, 64 bytes = one cache line: the boxes of BOTH children in float32
// (rounded outward), so one fetch decides where to go next.  child >= 0: inner
// node index; count > 0: leaf = `count` primitives from bvh_prims[child].
struct BvhNode {
  float lo0[3], hi0[3], lo1[3], hi1[3];
  int32_t child0, child1, count0, count1;
};
static_assert(sizeof(BvhNode) == 64, "BvhNode must be one 64-byte line");

float round_down(double v) {
  float f = (float)v;
  return (double)f > v ? std::nextafterf(f, -INFINITY) : f;
}
float round_up(double v) {
  float f = (float)v;
  return (double)f < v ? std::nextafterf(f, INFINITY) : f;
}

constexpr int kBvhLeaf = 8;   // largest leaf the SAH may form (measured: 8 >= 4 > 2 > 1 on meshes; round 5, mesh kernel at 1e6 facets: 8 / 6 / 4 / 3 / 2 / 1 = 7.70 / 7.73 / 7.84 / 7.95 / 8.16 / 9.04 ms -- candidates per segment 18 -> 8, node visits 11.7 -> 14.7)
constexpr int kBvhSweepMax = 256;        // nodes with more primitives use binned SAH
// the walk's leaf word, -2 - (first | count << 24), holds 24 bits of `first`: the leaf order must stay below 1 << 24 entries
inline bool bvh_order_fits(size_t entries) { return entries < ((size_t)1 << 24); }

// Surface-area-heuristic build (full sweep on the three axes).  Measured on
// hugeArray: 33 node visits and 3.0 primitive tests per segment against 57 /
// 5.8 with median splits.
struct BvhBuilder {
  const std::vector<Box>& boxes;
  std::vector<int> order;       // leaf primitive order
  std::vector<BvhNode> nodes;
  int max_depth = 0;

  // The heuristic goes on wherever the levels that are left still hold a median-split subtree of the node's primitives
  // down to leaves of kBvhLeaf; below that, median splits keep the tree within the traversal stack (round 5: against
  // medians from a fixed depth on, ball lens of 1e6 facets under the mesh kernel: 12.8 -> 7.2 candidate facets per
  // segment, 6.02 -> 5.77 ms per 1e7 rays, build 0.8 -> 1.1 s; full sweeps only up to kBvhSweepMax primitives).
  explicit BvhBuilder(const std::vector<Box>& b) : boxes(b) {}
  bool sah_ok(int depth, int m) const {
    const int need = (int)std::ceil(std::log2(std::max(1.0, (double)m / kBvhLeaf)));
    return depth + need + 2 <= ODW_BVH_STACK - 3;
  }

  static double area(const Box& b) {
    const double ex = b.hi[0] - b.lo[0], ey = b.hi[1] - b.lo[1], ez = b.hi[2] - b.lo[2];
    return 2.0 * (ex * ey + ey * ez + ez * ex);
  }

  struct Ref { int32_t child, count; Box box; };

  // builds the subtree over ids; returns either a leaf ref or an inner node ref
  Ref build(std::vector<int>& ids, int depth) {
    max_depth = std::max(max_depth, depth);
    Box bb;
    bb.reset();
    for (int i : ids) bb.grow(boxes[i]);
    const int m = (int)ids.size();
    auto make_leaf = [&]() {
      Ref r;
      r.child = (int32_t)order.size();
      r.count = m;
      r.box = bb;
      for (int i : ids) order.push_back(i);
      return r;
    };
    if (m <= 1) return make_leaf();
    const bool sah = sah_ok(depth, m);
    if (!sah && m <= kBvhLeaf) return make_leaf();
    if (m > kBvhSweepMax || !sah) return build_big(ids, depth, bb);
    // SAH sweep
    double best_cost = INFINITY;
    int best_axis = -1, best_split = 0;
    std::vector<int> sorted(ids), best_sorted;
    std::vector<double> right_area(m);
    for (int a = 0; a < 3; ++a) {
      std::sort(sorted.begin(), sorted.end(), [&](int x, int y) {
        const double cx = boxes[x].lo[a] + boxes[x].hi[a], cy = boxes[y].lo[a] + boxes[y].hi[a];
        return cx < cy || (cx == cy && x < y);
      });
      Box r;
      r.reset();
      for (int i = m - 1; i > 0; --i) { r.grow(boxes[sorted[i]]); right_area[i] = area(r); }
      Box l;
      l.reset();
      for (int i = 1; i < m; ++i) {
        l.grow(boxes[sorted[i - 1]]);
        const double cost = area(l) * i + right_area[i] * (m - i);
        if (cost < best_cost) { best_cost = cost; best_axis = a; best_split = i; best_sorted = sorted; }
      }
    }
    // leaf if splitting does not pay (traversal step ~ 1 primitive test) and it is small
    const double leaf_cost = area(bb) * m;
    if (m <= kBvhLeaf && best_cost + area(bb) >= leaf_cost) return make_leaf();
    // (no cost compares below infinity -- boxes whose area overflows --: median splits, never one leaf of up to
    //  kBvhSweepMax primitives, which the 7-bit count of a leaf word could not hold)
    if (best_axis < 0) return build_big(ids, depth, bb);
    std::vector<int> left(best_sorted.begin(), best_sorted.begin() + best_split);
    std::vector<int> right(best_sorted.begin() + best_split, best_sorted.end());
    return inner(left, right, depth, bb);
  }

  // big nodes (meshes): binned SAH over 32 bins of the centroid range, O(m) per
  // node; where sah_ok() says no: median splits, which bound the remaining
  // depth by log2(m / kBvhLeaf)
  Ref build_big(std::vector<int>& ids, int depth, const Box& bb) {
    const int m = (int)ids.size();
    Box cb;
    cb.reset();
    for (int i : ids)
      for (int a = 0; a < 3; ++a) {
        const double c = boxes[i].lo[a] + boxes[i].hi[a];
        cb.lo[a] = std::min(cb.lo[a], c);
        cb.hi[a] = std::max(cb.hi[a], c);
      }
    int axis = 0;
    for (int a = 1; a < 3; ++a) if (cb.hi[a] - cb.lo[a] > cb.hi[axis] - cb.lo[axis]) axis = a;
    auto centroid = [&](int i, int a) { return boxes[i].lo[a] + boxes[i].hi[a]; };
    std::vector<int> left, right;
    bool split_done = false;
    if (sah_ok(depth, m) && cb.hi[axis] > cb.lo[axis]) {
      constexpr int kBins = 32;
      double best_cost = INFINITY;
      int best_axis = -1, best_bin = 0;
      for (int a = 0; a < 3; ++a) {
        const double ext = cb.hi[a] - cb.lo[a];
        if (!(ext > 0)) continue;
        Box bins[kBins];
        int cnt[kBins] = {0};
        for (auto& b : bins) b.reset();
        for (int i : ids) {
          const int k = std::min(kBins - 1, (int)((centroid(i, a) - cb.lo[a]) / ext * kBins));
          bins[k].grow(boxes[i]);
          ++cnt[k];
        }
        double ra[kBins];
        int rc[kBins];
        Box r;
        r.reset();
        int c = 0;
        for (int k = kBins - 1; k > 0; --k) { r.grow(bins[k]); c += cnt[k]; ra[k] = c ? area(r) : 0.0; rc[k] = c; }
        Box l;
        l.reset();
        c = 0;
        for (int k = 1; k < kBins; ++k) {
          l.grow(bins[k - 1]);
          c += cnt[k - 1];
          if (c == 0 || rc[k] == 0) continue;
          const double cost = area(l) * c + ra[k] * rc[k];
          if (cost < best_cost) { best_cost = cost; best_axis = a; best_bin = k; }
        }
      }
      if (best_axis >= 0) {
        const double ext = cb.hi[best_axis] - cb.lo[best_axis];
        for (int i : ids) {
          const int k = std::min(kBins - 1, (int)((centroid(i, best_axis) - cb.lo[best_axis]) / ext * kBins));
          (k < best_bin ? left : right).push_back(i);
        }
        split_done = !left.empty() && !right.empty();
      }
    }
    if (!split_done) {   // median split along the widest centroid axis
      std::vector<int> sorted(ids);
      std::nth_element(sorted.begin(), sorted.begin() + m / 2, sorted.end(), [&](int x, int y) {
        const double cx = centroid(x, axis), cy = centroid(y, axis);
        return cx < cy || (cx == cy && x < y);
      });
      left.assign(sorted.begin(), sorted.begin() + m / 2);
      right.assign(sorted.begin() + m / 2, sorted.end());
    }
    return inner(left, right, depth, bb);
  }

  Ref inner(std::vector<int>& left, std::vector<int>& right, int depth, const Box& bb) {
    const int id = (int)nodes.size();
    nodes.emplace_back();
    const Ref l = build(left, depth + 1);
    const Ref r = build(right, depth + 1);
    BvhNode& nd = nodes[id];
    for (int k = 0; k < 3; ++k) {
      nd.lo0[k] = round_down(l.box.lo[k]); nd.hi0[k] = round_up(l.box.hi[k]);
      nd.lo1[k] = round_down(r.box.lo[k]); nd.hi1[k] = round_up(r.box.hi[k]);
    }
    nd.child0 = l.child; nd.count0 = l.count;
    nd.child1 = r.child; nd.count1 = r.count;
    Ref out;
    out.child = id;
    out.count = 0;
    out.box = bb;
    return out;
  }
};

// ---- eight-wide tree of the mesh kernel (odw_mesh.hip) --------------------------------------
// The binary tree above, collapsed: a wide node takes up to eight descendants of a binary node (the one with the
// largest box is opened next; one whose subtree is too high for the levels that remain goes first -- that bounds
// the depth, and with one stack entry per level the traversal stack, at kWideMaxDepth + 1).  The children's boxes
// are stored as 8-bit offsets from the node's corner in units of a power of two per axis (rounded outward);
// children sit in the slot whose sign pattern (x, y, z: away from / towards the corner) fits the direction from
// the node's centre to theirs best, so that `slot XOR ray octant` orders them roughly front to back without a
// sort.  Inner children are consecutive nodes (slot order), the facets of leaf children consecutive leaf
// records (slot order, <= 15 per leaf).
// Node = 32 words (128 bytes, 20 used):
//   0..2 corner (float)            3  exponent bytes x | y << 8 | z << 16 (biased: scale = 2^(e - 127))
//   4    first inner child         5  first leaf record
//   6    inner slots | leaf slots << 8          7  facets per leaf slot (4 bits each)
//   8..13 near corner offsets: x of slots 0-3, x of 4-7, y, y, z, z     14..19 far corner offsets, the same way
//   20..23 the solid every primitive below a slot belongs to (16 bits per slot, 0xffff: several or none): a ray that
//          has just left a convex solid drops the slots of that solid before it looks at their boxes' order
//   24..31 per slot, the cone of the outward normals of the facets below it, where they all belong to ONE STRICTLY
//          CONVEX solid: bytes 0..2 an axis a = round(127 u) (signed), byte 3 a threshold T + 3 <= 126 (signed); no cone:
//          0, 0, 0, 127.  A ray that travels INSIDE that solid (it entered through one of its facets, odw_mesh.hip `inside`)
//          can only leave through facets it meets from behind, d . n > 0; the kernel drops a slot when
//          v_dot4(word, [round(127 d), 127]) < 0, i.e. round(127 d) . a < -127 (T + 3): then d . a < -(T + 1.5) whatever the
//          rounding of d did (|round(127 d) - 127 d| <= 0.5 per axis, |a|_1 <= 220: 110 of the 190 to spare), and with
//          T = ceil(|a| sin(widest angle between a and a normal + asin(cone_margin))) every facet below the slot has
//          d . n < -cone_margin -- the whole neighbourhood of the facet the ray starts on, for one.  cone_margin
//          (WideBvh::margin) is what keeps the rule exact: the start point lies on its facet up to the closed-edge slack, so
//          it is above the plane of a dropped facet by less than `above`, and the plane would be met at
//          t < above / margin <= dist_tol, where consider() rejects it anyway.
constexpr int kWideWords = 32;
constexpr int kWideMaxDepth = 11;

struct WideBvh {
  struct Ref { int32_t child, count; float lo[3], hi[3]; };     // count > 0: leaf of `count` primitives from order[child]
  const std::vector<BvhNode>& bn;
  const std::vector<int>& order;
  const std::vector<int>& solid_of;           // solid id of every primitive
  const float* out_normal = nullptr;          // 3 per primitive: outward unit normal of the facets of convex solids, NaN for the rest
  double margin = 1.0;                        // >= 0.5: no cones
  std::vector<int> span_lo, span_hi;          // per binary node: its primitives are order[span_lo .. span_hi)
  std::vector<int> height;
  std::vector<int> solid_below;               // per binary node: the one solid of its primitives, -1 several, -2 not asked yet
  std::vector<uint32_t> nodes;
  std::vector<int> leaf_prim;                 // primitive of every leaf record
  std::vector<float> leaf_center;             // 3 per record: the centre its group is expressed around
  int depth = 0;
  bool ok = true;

  WideBvh(const std::vector<BvhNode>& n, const std::vector<int>& o, const std::vector<int>& so)
      : bn(n), order(o), solid_of(so), height(n.size(), -1), solid_below(n.size(), -2) {}

  int ref_solid(const Ref& r) {
    if (r.count == 0) return node_solid(r.child);
    int s = solid_of[order[(size_t)r.child]];
    for (int k = 1; k < r.count; ++k)
      if (solid_of[order[(size_t)r.child + k]] != s) return -1;
    return s;
  }
  int node_solid(int n) {
    if (solid_below[n] != -2) return solid_below[n];
    const BvhNode& nd = bn[n];
    int s = -3;                                 // nothing seen yet
    for (const Ref& r : {ref0(nd), ref1(nd)}) {
      if (far_box(r.lo)) continue;
      const int c = ref_solid(r);
      s = s == -3 ? c : (s == c ? s : -1);
    }
    return solid_below[n] = s == -3 ? -1 : s;
  }

  // (leaves are written to `order` in the order the builder meets them: a subtree's primitives are one run of it)
  void node_span(int n, int& lo, int& hi) {
    if (span_lo.empty()) { span_lo.assign(bn.size(), -1); span_hi.assign(bn.size(), -1); }
    if (span_lo[n] < 0) {
      int l = INT32_MAX, h = 0;
      const BvhNode& nd = bn[n];
      for (const Ref& r : {ref0(nd), ref1(nd)}) {
        if (far_box(r.lo)) continue;
        int a, b;
        if (r.count > 0) { a = r.child; b = r.child + r.count; } else node_span(r.child, a, b);
        l = std::min(l, a); h = std::max(h, b);
      }
      span_lo[n] = l == INT32_MAX ? 0 : l; span_hi[n] = h;
    }
    lo = span_lo[n]; hi = span_hi[n];
  }
  // the cone word of a slot (see the node layout above)
  uint32_t cone_word(const Ref& r) {
    constexpr uint32_t none = 0x7f000000u;
    if (!out_normal || !(margin < 0.5)) return none;
    int lo, hi;
    if (r.count > 0) { lo = r.child; hi = r.child + r.count; } else node_span(r.child, lo, hi);
    double sum[3] = {0.0, 0.0, 0.0};
    for (int k = lo; k < hi; ++k) {
      const float* nv = out_normal + 3 * (size_t)order[(size_t)k];
      if (!(nv[0] == nv[0])) return none;
      for (int a = 0; a < 3; ++a) sum[a] += (double)nv[a];
    }
    const double len = std::sqrt(sum[0] * sum[0] + sum[1] * sum[1] + sum[2] * sum[2]);
    if (!(len > 1e-6 * (double)(hi - lo)) || hi <= lo) return none;
    int ax[3];
    double al = 0.0;
    for (int a = 0; a < 3; ++a) { ax[a] = (int)std::lround(127.0 * sum[a] / len); al += (double)ax[a] * ax[a]; }
    al = std::sqrt(al);
    if (!(al > 100.0)) return none;
    double cmin = 1.0;
    for (int k = lo; k < hi; ++k) {
      const float* nv = out_normal + 3 * (size_t)order[(size_t)k];
      const double nl = std::sqrt((double)nv[0] * nv[0] + (double)nv[1] * nv[1] + (double)nv[2] * nv[2]);
      cmin = std::min(cmin, ((double)nv[0] * ax[0] + (double)nv[1] * ax[1] + (double)nv[2] * ax[2]) / (al * nl));
    }
    // (1e-5: the normals are float32 copies of unit vectors, the ray's direction is rounded to float32 in the kernel)
    const double theta = std::acos(std::max(-1.0, std::min(1.0, cmin))) + std::asin(margin) + 1e-5;
    if (!(theta < 1.5)) return none;
    const double t = std::ceil(al * std::sin(theta));
    if (!(t + 3.0 <= 126.0)) return none;                      // (cones that wide drop next to nothing)
    return (uint32_t)(ax[0] & 0xff) | ((uint32_t)(ax[1] & 0xff) << 8) | ((uint32_t)(ax[2] & 0xff) << 16) | ((uint32_t)(t + 3.0) << 24);
  }

  static bool far_box(const float* lo) { return lo[0] >= 3.0e38f; }        // the child a wrapper root does not have
  static Ref ref0(const BvhNode& nd) { Ref r{nd.child0, nd.count0, {nd.lo0[0], nd.lo0[1], nd.lo0[2]}, {nd.hi0[0], nd.hi0[1], nd.hi0[2]}}; return r; }
  static Ref ref1(const BvhNode& nd) { Ref r{nd.child1, nd.count1, {nd.lo1[0], nd.lo1[1], nd.lo1[2]}, {nd.hi1[0], nd.hi1[1], nd.hi1[2]}}; return r; }

  int node_height(int n) {
    if (height[n] >= 0) return height[n];
    const BvhNode& nd = bn[n];
    int h = 0;
    if (nd.count0 == 0 && !far_box(nd.lo0)) h = std::max(h, node_height(nd.child0));
    if (nd.count1 == 0 && !far_box(nd.lo1)) h = std::max(h, node_height(nd.child1));
    return height[n] = h + 1;
  }
  static double area(const Ref& r) {
    const double ex = (double)r.hi[0] - r.lo[0], ey = (double)r.hi[1] - r.lo[1], ez = (double)r.hi[2] - r.lo[2];
    return 2.0 * (ex * ey + ey * ez + ez * ex);
  }

  void build() {
    if (bn.empty()) { ok = false; return; }
    if (node_height(0) > 3 * (kWideMaxDepth + 1)) { ok = false; return; }
    nodes.assign(kWideWords, 0u);
    fill(0, 0, 0);
  }

  void fill(size_t index, int n, int d) {
    depth = std::max(depth, d);
    if (d > kWideMaxDepth) { ok = false; return; }
    std::vector<Ref> cand;
    for (const Ref& r : {ref0(bn[n]), ref1(bn[n])})
      if (!far_box(r.lo)) cand.push_back(r);
    const int allowed = 3 * (kWideMaxDepth - d);             // binary height a child's subtree may have
    while (cand.size() < 8) {
      int pick = -1;
      int tallest = allowed;
      for (size_t k = 0; k < cand.size(); ++k)
        if (cand[k].count == 0 && node_height(cand[k].child) > tallest) { tallest = node_height(cand[k].child); pick = (int)k; }
      if (pick < 0) {
        double best = -1.0;
        for (size_t k = 0; k < cand.size(); ++k)
          if (cand[k].count == 0 && area(cand[k]) > best) { best = area(cand[k]); pick = (int)k; }
      }
      if (pick < 0) break;                                     // leaves only
      const BvhNode& nd = bn[cand[pick].child];
      cand[pick] = ref0(nd);
      cand.push_back(ref1(nd));
    }
    // the node's box and the slots
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (const Ref& r : cand)
      for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], r.lo[a]); hi[a] = std::max(hi[a], r.hi[a]); }
    int slot_of[8], cand_in[8];
    for (int k = 0; k < 8; ++k) { slot_of[k] = -1; cand_in[k] = -1; }
    {
      struct Pair { double cost; int c, s; };
      std::vector<Pair> pairs;
      for (size_t c = 0; c < cand.size(); ++c)
        for (int sl = 0; sl < 8; ++sl) {
          double cost = 0.0;
          for (int a = 0; a < 3; ++a) {
            const double v = 0.5 * ((double)cand[c].lo[a] + cand[c].hi[a]) - 0.5 * ((double)lo[a] + hi[a]);
            cost += ((sl >> a) & 1) ? v : -v;
          }
          pairs.push_back({cost, (int)c, sl});
        }
      std::stable_sort(pairs.begin(), pairs.end(), [](const Pair& x, const Pair& y) { return x.cost > y.cost; });
      for (const Pair& pr : pairs)
        if (slot_of[pr.c] < 0 && cand_in[pr.s] < 0) { slot_of[pr.c] = pr.s; cand_in[pr.s] = pr.c; }
    }
    uint32_t w[kWideWords] = {0};
    uint32_t ebyte[3];
    double scale[3];
    for (int a = 0; a < 3; ++a) {
      std::memcpy(&w[a], &lo[a], 4);
      const double ext = (double)hi[a] - (double)lo[a];
      int e = -100;
      if (ext > 0) {
        int ex2;
        std::frexp(ext / 255.0, &ex2);                        // ext / 255 = m 2^ex2, 0.5 <= m < 1: 2^ex2 >= ext / 255
        e = ex2;
      }
      e = std::max(-126, std::min(127, e));
      while (std::ldexp(255.0, e) < ext && e < 127) ++e;
      ebyte[a] = (uint32_t)(e + 127);
      scale[a] = std::ldexp(1.0, e);
    }
    w[3] = ebyte[0] | (ebyte[1] << 8) | (ebyte[2] << 16);
    uint32_t imask = 0, lmask = 0, counts = 0;
    const uint32_t child_base = (uint32_t)(nodes.size() / kWideWords);
    const uint32_t leaf_base = (uint32_t)leaf_prim.size();
    int n_inner = 0;
    float glo[3] = {INFINITY, INFINITY, INFINITY}, ghi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int sl = 0; sl < 8; ++sl) {
      const int c = cand_in[sl];
      if (c < 0) { w[24 + sl] = 0x7f000000u; continue; }
      const Ref& r = cand[c];
      if (r.count == 0) { imask |= 1u << sl; ++n_inner; }
      else {
        if (r.count > 15) { ok = false; return; }
        lmask |= 1u << sl;
        counts |= (uint32_t)r.count << (4 * sl);
        for (int a = 0; a < 3; ++a) { glo[a] = std::min(glo[a], r.lo[a]); ghi[a] = std::max(ghi[a], r.hi[a]); }
      }
      {
        const int so = ref_solid(r);
        w[20 + (sl >> 1)] |= (uint32_t)((so >= 0 && so < 0xffff) ? so : 0xffff) << (16 * (sl & 1));
        w[24 + sl] = (so >= 0 && so < 0xffff) ? cone_word(r) : 0x7f000000u;
      }
      for (int a = 0; a < 3; ++a) {
        const double ql = std::floor(((double)r.lo[a] - (double)lo[a]) / scale[a]);
        const double qh = std::ceil(((double)r.hi[a] - (double)lo[a]) / scale[a]);
        const uint32_t bl = (uint32_t)std::max(0.0, std::min(255.0, ql)), bh = (uint32_t)std::max(0.0, std::min(255.0, qh));
        if (qh > 255.0) { ok = false; return; }                // (cannot happen: 255 scale >= extent)
        w[8 + 2 * a + (sl >> 2)] |= bl << (8 * (sl & 3));
        w[14 + 2 * a + (sl >> 2)] |= bh << (8 * (sl & 3));
      }
    }
    {
      int total = 0;
      for (int sl = 0; sl < 8; ++sl) total += (int)((counts >> (4 * sl)) & 15u);
      if (total > 64) { ok = false; return; }                  // (the kernel's candidate mask)
    }
    w[4] = child_base;
    w[5] = leaf_base;
    w[6] = imask | (lmask << 8);
    w[7] = counts;
    std::memcpy(&nodes[index * kWideWords], w, sizeof w);
    // leaf records of this node, slot order
    const float gc[3] = {0.5f * glo[0] + 0.5f * ghi[0], 0.5f * glo[1] + 0.5f * ghi[1], 0.5f * glo[2] + 0.5f * ghi[2]};
    for (int sl = 0; sl < 8; ++sl) {
      const int c = cand_in[sl];
      if (c < 0 || cand[c].count == 0) continue;
      for (int k = 0; k < cand[c].count; ++k) {
        leaf_prim.push_back(order[(size_t)cand[c].child + k]);
        leaf_center.insert(leaf_center.end(), gc, gc + 3);
      }
    }
    // inner children: consecutive nodes, slot order
    nodes.resize(nodes.size() + (size_t)n_inner * kWideWords, 0u);
    int rank = 0;
    for (int sl = 0; sl < 8; ++sl) {
      const int c = cand_in[sl];
      if (c < 0 || cand[c].count != 0) continue;
      const int child = cand[c].child;
      fill((size_t)child_base + rank, child, d + 1);
      if (!ok) return;
      ++rank;
    }
  }
};

// ---- what the builders hand back ---------------------------------------------------------------------------------
// The values are those of odw_build_check's `structure`.  A scene with a grid has the trees too (launches with
// stochastic surfaces or segment rows take them); one of kAccelFlat has neither.
enum AccelKind { kAccelFlat = 0, kAccelGrid = 1, kAccelTree = 2, kAccelWide = 3 };
inline AccelKind accel_kind(bool grid, bool tree, bool wide) {
  return grid ? kAccelGrid : !tree ? kAccelFlat : wide ? kAccelWide : kAccelTree;
}

struct SceneAccel {
  // the rectilinear grid (grid.nx = 0: none): the numbers as the kernel reads them -- the three addresses are the
  // uploader's to set -- and the tables
  DeviceGrid grid = {};
  std::vector<double> planes;               // x, y, z planes, one run after the other
  std::vector<uint32_t> cells;
  std::vector<double> sphere_recs;          // the items: 48-byte records where every primitive is an untrimmed sphere ...
  std::vector<uint32_t> item_prim;          // ... primitive numbers otherwise
  const void* items() const { return grid.spheres ? (const void*)sphere_recs.data() : (const void*)item_prim.data(); }
  size_t item_bytes() const { return grid.spheres ? sphere_recs.size() * sizeof(double) : item_prim.size() * sizeof(uint32_t); }
  // the binary tree (nodes empty: none) ...
  std::vector<BvhNode> nodes;
  std::vector<int> order;                   // leaf primitive order
  int max_depth = 0;
  // ... and the mesh kernel's eight-wide tree over it (leaf_recs empty: none)
  std::vector<uint32_t> wide_nodes;
  std::vector<float> leaf_recs;
  double wide_lo[3] = {0, 0, 0}, wide_hi[3] = {0, 0, 0};   // node 0 as the kernel decodes it

  AccelKind kind() const { return accel_kind(grid.nx > 0, !nodes.empty(), !leaf_recs.empty()); }
};

// what the environment says at every build (ODW_MESH_KERNEL, ODW_MESH_CONES, ODW_MESH_CONE_STATS: read by the caller)
struct BuildOptions {
  bool mesh_kernel = true;                  // the eight-wide tree for scenes with facets
  bool cones = true;                        // normal cones in its nodes
  bool cone_stats = false;                  // diagnostics on stderr: how many slots carry a cone
  bool force_tree = false;                  // a binary tree also for a scene the flat loop takes (spectral launches)
};

// ---- rectilinear grid for big analytic scenes (odw_grid.hip) ---------------------------------
// Planes per axis: one in the middle of every gap between the primitives' boxes (projected on the
// axis) -- a Draft array gets one element per cell --, then slabs wider than twice the width an
// even division into ~cbrt(n) cells per axis would give are cut evenly.  Cell lists (CSR): every
// primitive whose box touches the cell.  The walk is exact whatever the planes are; they only
// decide how many cells a ray crosses and how many primitives it tests per cell.
constexpr int kGridMaxAxis = 128;             // cells per axis (8 bits each in the walk's cell word)
constexpr uint32_t kGridMaxCellItems = 255;   // 8-bit count in the cell word
constexpr size_t kGridLdsBudget = 144 * 1024; // of the CU's 160 KB, one block per CU

// A is left without a grid (nx = 0) where the scene does not take one: the trees serve it
void build_grid(const HostScene& hs, const std::vector<Box>& boxes, SceneAccel& A) {
  DeviceGrid& G = A.grid;
  const std::vector<char>& dead = hs.dead;
  const int n = (int)boxes.size();
  std::vector<int> live;
  for (int p = 0; p < n; ++p)
    if (!dead[p]) live.push_back(p);
  if (live.empty()) return;
  Box all;
  all.reset();
  for (int p : live) all.grow(boxes[p]);
  double ext[3], vol = 1.0;
  for (int a = 0; a < 3; ++a) { ext[a] = std::max(all.hi[a] - all.lo[a], 1e-9); vol *= ext[a]; }
  const double per_len = std::cbrt((double)live.size() / vol);     // cells per unit length for ~1 primitive per cell
  std::vector<double> planes[3];
  for (int a = 0; a < 3; ++a) {
    std::vector<std::pair<double, double>> iv;
    for (int p : live) iv.emplace_back(boxes[p].lo[a], boxes[p].hi[a]);
    std::sort(iv.begin(), iv.end());
    const double pad = 1e-6 * (1.0 + ext[a]);
    std::vector<double> b{all.lo[a] - pad};
    double cover = iv[0].second;
    for (size_t k = 1; k < iv.size(); ++k) {
      if (iv[k].first > cover) b.push_back(0.5 * (cover + iv[k].first));
      cover = std::max(cover, iv[k].second);
    }
    b.push_back(all.hi[a] + pad);
    const double target = 1.0 / std::max(per_len, 1e-12);          // width of a cell of the even division
    std::vector<double> cut{b[0]};
    for (size_t k = 1; k < b.size(); ++k) {
      const double wdt = b[k] - b[k - 1];
      const int parts = wdt > 2.0 * target ? (int)std::min<double>(kGridMaxAxis, std::floor(wdt / target + 0.5)) : 1;
      for (int j = 1; j <= parts; ++j) cut.push_back(j == parts ? b[k] : b[k - 1] + wdt * j / parts);
    }
    if ((int)cut.size() - 1 > kGridMaxAxis) {                     // too fine: even division
      cut.clear();
      for (int j = 0; j <= kGridMaxAxis; ++j) cut.push_back(b.front() + (b.back() - b.front()) * j / kGridMaxAxis);
      cut.back() = b.back();
    }
    planes[a] = cut;
  }
  const int nx = (int)planes[0].size() - 1, ny = (int)planes[1].size() - 1, nz = (int)planes[2].size() - 1;
  const size_t ncell = (size_t)nx * ny * nz;
  if (ncell > (1u << 21)) return;
  // cell ranges of every primitive (closed boxes: a box that ends on a plane is listed on both sides)
  auto range = [&](int a, double lo, double hi, int& i0, int& i1) {
    const std::vector<double>& b = planes[a];
    const int m = (int)b.size() - 1;
    i0 = (int)(std::upper_bound(b.begin(), b.end(), lo) - b.begin()) - 1;     // last plane <= lo
    if (i0 > 0 && b[i0] == lo) --i0;
    i1 = (int)(std::lower_bound(b.begin(), b.end(), hi) - b.begin()) - 1;     // slab whose upper plane >= hi
    if (i1 + 1 < m && b[i1 + 1] == hi) ++i1;
    i0 = std::max(0, std::min(m - 1, i0));
    i1 = std::max(i0, std::min(m - 1, i1));
  };
  std::vector<uint32_t> count(ncell, 0);
  std::vector<int> r(6 * (size_t)live.size());
  for (size_t k = 0; k < live.size(); ++k) {
    const Box& bx = boxes[live[k]];
    int* q = &r[6 * k];
    range(0, bx.lo[0], bx.hi[0], q[0], q[1]);
    range(1, bx.lo[1], bx.hi[1], q[2], q[3]);
    range(2, bx.lo[2], bx.hi[2], q[4], q[5]);
    for (int z = q[4]; z <= q[5]; ++z)
      for (int y = q[2]; y <= q[3]; ++y)
        for (int x = q[0]; x <= q[1]; ++x) ++count[x + (size_t)nx * (y + (size_t)ny * z)];
  }
  size_t total = 0;
  std::vector<uint32_t> first(ncell);
  for (size_t c = 0; c < ncell; ++c) {
    if (count[c] > kGridMaxCellItems) return;              // crowded beyond the cell word: BVH kernels
    first[c] = (uint32_t)total;
    total += count[c];
  }
  if (total >= (1u << 24)) return;
  std::vector<uint32_t> item_prim(std::max<size_t>(total, 1)), fill(ncell, 0);
  for (size_t k = 0; k < live.size(); ++k) {
    const int* q = &r[6 * k];
    for (int z = q[4]; z <= q[5]; ++z)
      for (int y = q[2]; y <= q[3]; ++y)
        for (int x = q[0]; x <= q[1]; ++x) {
          const size_t c = x + (size_t)nx * (y + (size_t)ny * z);
          item_prim[first[c] + fill[c]++] = (uint32_t)live[k];
        }
  }
  std::vector<uint32_t> cells(ncell);
  for (size_t c = 0; c < ncell; ++c) cells[c] = first[c] | (count[c] << 24);
  bool spheres = true;
  for (int p : live) {
    const int32_t* pi = &hs.prim_i32[4 * (size_t)p];
    if (pi[0] != ODW_PRIM_SPHERE || ((pi[3] >> 24) & 0xff) != 0) { spheres = false; break; }
  }
  std::vector<double> bounds;
  for (int a = 0; a < 3; ++a) bounds.insert(bounds.end(), planes[a].begin(), planes[a].end());
  size_t item_bytes;
  std::vector<double> recs;
  if (spheres) {
    // 48-byte records: centre (global; prim_f64 12..15 = R, cx, cy, cz as the flat kernel reads them),
    // radius, {primitive, group | solid << 8}, the primitive's flag word
    recs.resize(std::max<size_t>(total, 1) * 6, 0.0);
    for (size_t k = 0; k < total; ++k) {
      const uint32_t p = item_prim[k];
      const double* par = hs.prim_f64.data() + 16 * (size_t)p + 12;
      const int32_t* pi = &hs.prim_i32[4 * (size_t)p];
      double* o = &recs[6 * k];
      o[0] = par[1]; o[1] = par[2]; o[2] = par[3]; o[3] = par[0];
      const uint64_t bits = (uint64_t)p | ((uint64_t)(uint32_t)((pi[1] & 0xff) | ((pi[2] >> ODW_SOLID_SHIFT) << 8)) << 32);
      std::memcpy(&o[4], &bits, sizeof bits);
      const uint64_t flag_word = (uint64_t)(uint32_t)pi[2];          // (flags | facemask << 8 | solid << 16, for the interaction)
      std::memcpy(&o[5], &flag_word, sizeof flag_word);
    }
    item_bytes = recs.size() * sizeof(double);
  } else {
    item_prim.resize((item_prim.size() + 1) & ~(size_t)1, 0u);      // whole doubles (the LDS copy moves 8 bytes at a time)
    item_bytes = item_prim.size() * sizeof(uint32_t);
  }
  // the kernel's LDS image (odw_grid_kernel, same arithmetic): planes | per-wave words | ray rings | cells | items
  const size_t nbp = bounds.size();
  const size_t word_off = 2 * nbp;
  const size_t ring_off = (word_off + (size_t)ODW_GRID_WAVES * ODW_GRID_WAVE_WORDS + 1) / 2;
  const size_t cell_off = 2 * (ring_off + (size_t)ODW_GRID_WAVES * ODW_GRID_RING_DOUBLES);
  const size_t fixed = cell_off * sizeof(uint32_t);
  const size_t staged = (((cell_off + ncell + 3) & ~(size_t)3) / 2) * sizeof(double) + item_bytes;
  A.planes = std::move(bounds);
  A.cells = std::move(cells);
  A.sphere_recs = std::move(recs);
  if (!spheres) A.item_prim = std::move(item_prim);
  G.nx = nx; G.ny = ny; G.nz = nz;
  G.n_items = (int32_t)total;
  G.spheres = spheres ? 1 : 0;
  G.in_lds = staged + 16 <= kGridLdsBudget ? 1 : 0;
  G.lds_bytes = (uint32_t)((G.in_lds ? staged : fixed) + 16);
}

// the primitives' boxes for the tolerance dist_tol; into hs: the 64-byte headers, the dead primitives and
// ODW_FLAG_ISOLATED in the flag words
void compute_boxes(HostScene& hs, double dist_tol, std::vector<Box>& boxes) {
  const int n = hs.n_prims;
  std::vector<char>& dead = hs.dead;
  // boxes contain every point the tolerance rules may accept
  const double slack = 2.0 * dist_tol;
  boxes.assign(n, Box());
  std::vector<double>& flat = hs.prim_hdr;
  flat.assign((size_t)std::max(1, n) * 8, 0.0);   // 64-byte headers
  for (int p = 0; p < n; ++p)
    boxes[p] = world_box(hs.prim_f64.data() + 16 * (size_t)p, hs.prim_i32[4 * p], slack,
                         hs.prim_i32[4 * p] == ODW_PRIM_ASPHERE ? hs.asph[ODW_ASPH_ROW * (size_t)p + 10] : 0.0);
  // A face that exists only inside other primitives (operands of a Common, the base of a Cut for
  // its tool) lies in their boxes too: the box of a lens cap is the lens, not the sphere.
  // Primitives without faces (pure operands) and faces that cannot exist get a box no ray meets.
  std::vector<Box> full = boxes;
  dead.assign(n, 0);
  // A trimming list of several clauses bounds the face by the UNION over its clauses of (own box ^ that clause's
  // must-be-inside operands): a literal of one clause alone does not bound it.  One clause: the cut as it always was.
  for (int p = 0; p < n; ++p) {
    const int cw = hs.prim_i32[4 * p + 3], off = cw & 0xffffff, cnt = (cw >> 24) & 0xff;
    const int end = std::min(off + cnt, (int)hs.cond.size());
    Box u;
    u.reset();
    int clauses = 0;
    for (int c0 = off; c0 < end;) {
      int c1 = c0 + 1;
      while (c1 < end && !cond_opens(hs.cond[c1])) ++c1;
      Box b = full[p];
      for (int c = c0; c < c1; ++c) {
        if (hs.cond[c] >= 0) continue;                     // must be OUTSIDE that one: no bound
        const Box& o = full[cond_operand(hs.cond[c])];
        for (int a = 0; a < 3; ++a) {
          b.lo[a] = std::max(b.lo[a], o.lo[a]);
          b.hi[a] = std::min(b.hi[a], o.hi[a]);
        }
      }
      if (clauses++ == 0) boxes[p] = b;                        // (an empty first clause stays empty unless another grows it)
      if (b.lo[0] <= b.hi[0] && b.lo[1] <= b.hi[1] && b.lo[2] <= b.hi[2]) u.grow(b);
      c0 = c1;
    }
    if (clauses > 1 && u.lo[0] <= u.hi[0]) boxes[p] = u;
    const int facemask = (hs.prim_i32[4 * p + 2] >> ODW_FACEMASK_SHIFT) & 0xff;
    dead[p] = facemask == 0 || boxes[p].lo[0] > boxes[p].hi[0] || boxes[p].lo[1] > boxes[p].hi[1] ||
              boxes[p].lo[2] > boxes[p].hi[2];
    if (dead[p])
      for (int a = 0; a < 3; ++a) boxes[p].lo[a] = boxes[p].hi[a] = 1e30;
  }
  // ODW_FLAG_ISOLATED (odw_device.h): solids whose box keeps clear of every other solid's
  {
    std::map<int, Box> solid_box;
    for (int p = 0; p < n; ++p) {
      hs.prim_i32[4 * p + 2] &= ~ODW_FLAG_ISOLATED;
      if (dead[p]) continue;
      const int sid = hs.prim_i32[4 * p + 2] >> ODW_SOLID_SHIFT;
      auto it = solid_box.find(sid);
      if (it == solid_box.end()) { solid_box[sid] = boxes[p]; continue; }
      for (int a = 0; a < 3; ++a) {
        it->second.lo[a] = std::min(it->second.lo[a], boxes[p].lo[a]);
        it->second.hi[a] = std::max(it->second.hi[a], boxes[p].hi[a]);
      }
    }
    const double gap = 2.0 * slack;                             // 4 distTol
    if (solid_box.size() <= 64 && solid_box.count(0x7fff) == 0)  // (0x7fff: solid ids that did not fit the word)
      for (int p = 0; p < n; ++p) {
        if (dead[p]) continue;
        const int sid = hs.prim_i32[4 * p + 2] >> ODW_SOLID_SHIFT;
        const Box& mine = solid_box[sid];
        bool alone = true;
        for (const auto& other : solid_box) {
          if (other.first == sid) continue;
          bool apart = false;
          for (int a = 0; a < 3; ++a)
            apart |= mine.lo[a] - other.second.hi[a] > gap || other.second.lo[a] - mine.hi[a] > gap;
          if (!apart) { alone = false; break; }
        }
        if (alone) hs.prim_i32[4 * p + 2] |= ODW_FLAG_ISOLATED;
      }
  }
  for (int p = 0; p < n; ++p) {
    double* h = flat.data() + 8 * (size_t)p;
    for (int a = 0; a < 3; ++a) { h[a] = boxes[p].lo[a]; h[3 + a] = boxes[p].hi[a]; }
    std::memcpy(h + 6, &hs.prim_i32[4 * (size_t)p], 4 * sizeof(int32_t));
  }
}

// ---- the value image of a scene-compiled kernel ------------------------------------------------
// A compiled kernel (odw_spec.hip) knows its scene's structure; every float64 VALUE its unrolled loop reads comes from
// one dense block of doubles, laid out for exactly that structure and read at compile-time offsets:
//   [0..3]   limits: distTol, maxRayLength + distTol, 2 distTol, 0
//   groups:  group_f64 (4 per group) | group_gdir (3 per group) | grating type and order (the group_i32 row: 2 doubles)
//   per primitive: the frame entries that are neither 0 nor +-1 (xf_pattern), in index order | its 4 parameters |
//                  with a box of its own (box_of[p] == p, some face): centre xyz, half extent xyz |
//                  with a face: the constants intersect_prim derives from parameters and tolerance (spec_image_build)
//   behind the doubles, one word of 64 bits that is not one: bit s = solid s is isolated (compute_boxes:
//            ODW_FLAG_ISOLATED).  Isolation depends on the boxes' values, so it is a value like them: the header never
//            holds it, and in a batch every scene's image carries its own (which is why the word lies in the per-scene
//            part and not in the limits section, read from the kernel arguments for every scene of a batch)
// The layout depends on the structure only, the values on the scene's numbers and the limits.

// zero / +-1 pattern of a frame's 12 entries (odw_kernels.hip: xf_comb): bits 0-11 entry != 0, 12-23 entry == +1,
// 24-35 entry == -1 (rotation part only)
inline unsigned long long xf_pattern(const double* m) {
  unsigned long long w = 0;
  for (int i = 0; i < 12; ++i) {
    if (m[i] != 0.0) w |= 1ull << i;
    if (i % 4 != 3 && m[i] == 1.0) w |= 1ull << (12 + i);
    if (i % 4 != 3 && m[i] == -1.0) w |= 1ull << (24 + i);
  }
  return w;
}
// the entries of a frame the image stores
inline unsigned xf_stored(unsigned long long xf) { return (unsigned)(xf & ~(xf >> 12) & ~(xf >> 24) & 0xfffull); }

// primitives with the same box: equal sets {p} + {q : p must lie inside q} (compute_boxes cuts p's box by
// the boxes of those q), one set per clause of a trimming list of several (compute_boxes: the union over the
// clauses of such cuts -- equal sets of sets, equal boxes).  box_of = the first such primitive, box_shared =
// another one refers to it.  (dead here: no face -- an empty box is a matter of values)
inline void spec_box_sharing(const HostScene& hs, std::vector<int>& box_of, std::vector<int>& box_shared) {
  const int n = hs.n_prims;
  box_of.assign(n, 0);
  box_shared.assign(n, 0);
  std::vector<std::vector<std::vector<int>>> inside(n);
  std::vector<char> dead(n);
  for (int p = 0; p < n; ++p) {
    const int cw = hs.prim_i32[4 * p + 3], off = cw & 0xffffff, cnt = (cw >> 24) & 0xff;
    const int end = std::min(off + cnt, (int)hs.cond.size());
    dead[p] = (((hs.prim_i32[4 * p + 2] & ~ODW_FLAG_ISOLATED) >> ODW_FACEMASK_SHIFT) & 0xff) == 0;
    inside[p].push_back({p});
    for (int c = off; c < end; ++c) {
      if (c != off && cond_opens(hs.cond[c])) inside[p].push_back({p});
      if (hs.cond[c] < 0) inside[p].back().push_back(cond_operand(hs.cond[c]));
    }
    for (std::vector<int>& set : inside[p]) {
      std::sort(set.begin(), set.end());
      set.erase(std::unique(set.begin(), set.end()), set.end());
    }
    std::sort(inside[p].begin(), inside[p].end());
  }
  for (int p = 0; p < n; ++p) {
    box_of[p] = p;
    // (the sets are equal, but compute_boxes cuts with the operands' FULL boxes only: p's box is
    //  box(p) ^ box(q1) ^ ..., the same expression for both when the sets agree)
    for (int q = 0; q < p; ++q)
      if (!dead[q] && !dead[p] && hs.prim_i32[4 * q + 1] == hs.prim_i32[4 * p + 1] && inside[q] == inside[p]) {
        box_of[p] = q;
        box_shared[q] = 1;
        break;
      }
  }
}

constexpr int kSpecImageLimits = 4;       // doubles of the limits section (it travels in the kernel arguments always)
// A launch's kernel arguments hold 4 KB: TraceParams, the image's pointer, the image, and the arguments the compiler
// adds (256 bytes; twice that is left).  A larger image stays in device memory.
constexpr size_t kSpecArgBytes = 4096 - 512;

struct SpecLayout {
  int n = 0, ng = 0, size = 0;
  int gf = 0, gd = 0, gi = 0;                       // group_f64, group_gdir, group_i32 rows
  int iso = 0;                                      // the mask of isolated solids (one word), behind the plain layout's last double
  std::vector<int> frame, par, box, der;            // per primitive (box, der: -1 = none)
  std::vector<int> box_of, box_shared;
  std::vector<int> dc;                              // spectral variant: per group, its six dispersion coefficients (-1: none); else empty
  std::vector<int> cc, cn;                          // coated variant: per group, its (index, thickness) pairs (-1: none) and their number; else empty
  int words() const { return std::max(size, iso + 1); }     // the image as a kernel reads it: the doubles and the mask word
  bool fits(size_t params_bytes) const { return ((params_bytes + 7) & ~(size_t)7) + 8 + (size_t)words() * 8 <= kSpecArgBytes; }
};

inline int spec_derived_count(int type) {
  switch (type) {
    case ODW_PRIM_BOX: return 3;
    case ODW_PRIM_CYLINDER: case ODW_PRIM_CONE: case ODW_PRIM_PARABOLOID: case ODW_PRIM_TORUS: return 4;
    case ODW_PRIM_CONICOID: case ODW_PRIM_ASPHERE: return 3;
    default: return 0;
  }
}

// disp_kind (spectral variant of the compiled kernel): six coefficient words per dispersive group, behind everything
// else -- the offsets of every other piece are those of the plain layout
// coat_n (coated variant of the FRESNEL kernel; never together with disp_kind): two words per layer of a coated group, in
// the same place.  Null, or no layer anywhere: the plain layout
inline SpecLayout spec_image_layout(const HostScene& hs, const int32_t* disp_kind = nullptr, const int32_t* coat_n = nullptr) {
  SpecLayout L;
  const int n = L.n = hs.n_prims, ng = L.ng = hs.n_groups;
  spec_box_sharing(hs, L.box_of, L.box_shared);
  int at = kSpecImageLimits;
  L.gf = at; at += 4 * ng;
  L.gd = at; at += 3 * ng;
  L.gi = at; at += 2 * ng;
  L.frame.assign(n, 0); L.par.assign(n, 0); L.box.assign(n, -1); L.der.assign(n, -1);
  for (int p = 0; p < n; ++p) {
    const bool faces = (((hs.prim_i32[4 * p + 2]) >> ODW_FACEMASK_SHIFT) & 0xff) != 0;
    L.frame[p] = at; at += __builtin_popcount(xf_stored(xf_pattern(&hs.prim_f64[16 * (size_t)p])));
    // (an asphere's row of the table -- coefficients, bounds -- lies behind its parameters)
    L.par[p] = at; at += hs.prim_i32[4 * p] == ODW_PRIM_ASPHERE ? 4 + ODW_ASPH_ROW : 4;
    if (faces && L.box_of[p] == p) { L.box[p] = at; at += 6; }
    const int nd = faces ? spec_derived_count(hs.prim_i32[4 * p]) : 0;
    if (nd) { L.der[p] = at; at += nd; }
  }
  // (the doubles of the plain layout end here, and `size` with them; the mask word stands behind them, in front of a
  //  spectral variant's coefficients, whose layout holds it inside its size: words() in every case)
  L.iso = at;
  if (disp_kind) {
    at += 1;
    L.dc.assign(std::max(1, ng), -1);
    for (int g = 0; g < ng; ++g)
      if (disp_kind[g]) { L.dc[g] = at; at += ODW_DISP_COEFS; }
  }
  bool coated = false;
  for (int g = 0; coat_n && !disp_kind && g < ng; ++g) coated |= coat_n[g] > 0;
  if (coated) {
    at += 1;
    L.cc.assign(std::max(1, ng), -1);
    L.cn.assign(std::max(1, ng), 0);
    for (int g = 0; g < ng; ++g)
      if (coat_n[g] > 0) { L.cc[g] = at; L.cn[g] = coat_n[g]; at += 2 * coat_n[g]; }
  }
  L.size = at;
  return L;
}

// Centre and half extent of the interval [lo, hi] (lo <= hi, finite) as the compiled kernels' box screen reads them:
// c near the middle (its rounding does not matter), h >= 0 rounded outward until c - h <= lo and c + h >= hi hold in
// float64 -- the screened interval contains the box, slack included.
inline void box_centre_half(double lo, double hi, double& c, double& h) {
#pragma clang fp contract(off)
  c = 0.5 * lo + 0.5 * hi;
  h = std::max(hi - c, c - lo);
  if (!(h >= 0.0)) h = 0.0;
  while (c - h > lo || c + h < hi) h = std::nextafter(h, INFINITY);
}

// The isolated solids of hs as the compiled kernels read them: bit s = the primitives of solid s carry
// ODW_FLAG_ISOLATED (compute_boxes sets it on every primitive of a solid that has a box, or on none).  Solid ids of 64
// and more -- 0x7fff, the id of solids that did not fit the flag word, among them -- have no bit: never isolated here.
inline uint64_t spec_isolated_mask(const HostScene& hs) {
  uint64_t mask = 0;
  for (int p = 0; p < hs.n_prims; ++p) {
    const int32_t w = hs.prim_i32[4 * (size_t)p + 2];
    const int sid = w >> ODW_SOLID_SHIFT;
    if ((w & ODW_FLAG_ISOLATED) && sid >= 0 && sid < 64) mask |= 1ull << sid;
  }
  return mask;
}

// The image of hs (boxes built: compute_boxes) for the limits lim: its doubles, img[0 .. L.size), or -- whole, what a
// launch hands its kernel -- img[0 .. L.words()) with the mask of isolated solids at L.iso.  Every derived constant is the
// sequence of IEEE operations intersect_prim performs on the device for it (odw_kernels.hip, compiled with
// -ffp-contract=on): std::fma where a product and a sum of ONE expression fuse there, plain operations elsewhere --
// and nothing else fuses here.
// coat: the context's table of layers, [group][ODW_COAT_LAYERS][2], for a layout with coated groups
inline void spec_image_build(const HostScene& hs, const DeviceLimits& lim, const SpecLayout& L, double* img,
                             const double* disp_coef = nullptr, bool whole = false, const double* coat = nullptr) {
#pragma clang fp contract(off)
  const double tol = lim.dist_tol;
  std::fill(img, img + (whole ? L.words() : L.size), 0.0);
  if (disp_coef)
    for (int g = 0; g < (int)L.dc.size() && g < L.ng; ++g)
      if (L.dc[g] >= 0) std::memcpy(&img[L.dc[g]], disp_coef + ODW_DISP_COEFS * g, ODW_DISP_COEFS * sizeof(double));
  if (coat)
    for (int g = 0; g < (int)L.cc.size() && g < L.ng; ++g)
      if (L.cc[g] >= 0) std::memcpy(&img[L.cc[g]], coat + 2 * ODW_COAT_LAYERS * (size_t)g, 2 * (size_t)L.cn[g] * sizeof(double));
  img[0] = tol;
  img[1] = lim.max_ray_length + tol;
  img[2] = 2.0 * tol;
  for (int g = 0; g < L.ng; ++g) {
    for (int k = 0; k < 4; ++k) img[L.gf + 4 * g + k] = hs.group_f64[4 * (size_t)g + k];
    for (int k = 0; k < 3; ++k) img[L.gd + 3 * g + k] = hs.group_gdir[3 * (size_t)g + k];
    std::memcpy(&img[L.gi + 2 * g], &hs.group_i32[4 * (size_t)g], 4 * sizeof(int32_t));
  }
  if (whole) {
    const uint64_t iso = spec_isolated_mask(hs);
    std::memcpy(&img[L.iso], &iso, sizeof iso);
  }
  for (int p = 0; p < L.n; ++p) {
    const double* pf = &hs.prim_f64[16 * (size_t)p];
    const double* par = pf + 12;
    const unsigned stored = xf_stored(xf_pattern(pf));
    int at = L.frame[p];
    for (int i = 0; i < 12; ++i)
      if ((stored >> i) & 1u) img[at++] = pf[i];
    for (int k = 0; k < 4; ++k) img[L.par[p] + k] = par[k];
    if (hs.prim_i32[4 * p] == ODW_PRIM_ASPHERE)
      for (int k = 0; k < ODW_ASPH_ROW; ++k) img[L.par[p] + 4 + k] = hs.asph[ODW_ASPH_ROW * (size_t)p + k];
    if (L.box[p] >= 0) {
      // centre and half extent of the box, the half extent rounded outward: [c - h, c + h] holds [lo, hi] in float64
      const double* b = &hs.prim_hdr[8 * (size_t)p];
      for (int a = 0; a < 3; ++a) box_centre_half(b[a], b[3 + a], img[L.box[p] + a], img[L.box[p] + 3 + a]);
    }
    if (L.der[p] < 0) continue;
    double* d = img + L.der[p];
    const int type = hs.prim_i32[4 * p];
    if (type == ODW_PRIM_BOX) {
      for (int a = 0; a < 3; ++a) d[a] = par[a] + tol;                    // the face rectangles' far edges
    } else if (type == ODW_PRIM_TORUS) {
      const double R1 = par[0], R2 = par[1];
      d[0] = std::fma(R1 + R2, 1.0000001, 1e-9);                          // bound
      d[1] = std::fma(R2, 1.0000001, 1e-9);                               // zs
      d[2] = std::fma(R1 - R2, 0.9999999, -1e-9);                         // rin
      d[3] = d[2] * d[2];
    } else if (type == ODW_PRIM_CONICOID) {
      d[0] = par[2] + tol;                                                // the z window's upper end
      d[1] = (par[3] + tol) * (par[3] + tol);                             // the cap's disc
      d[2] = 1.0 + par[1];                                                // the z^2 coefficient
    } else if (type == ODW_PRIM_ASPHERE) {
      d[0] = par[2] + tol;                                                // the clip region's cap
      const double wt = std::fmin(tol, 1e-3 * par[3]);                    // (the bounds M, L hold that far out, no farther)
      d[1] = (par[3] + wt) * (par[3] + wt);                               // the clip region's cylinder
      d[2] = par[3] * par[3];                                             // the wall
    } else {
      const bool parab = type == ODW_PRIM_PARABOLOID;
      const double R1 = parab ? 0.0 : par[0];
      const double R2 = (type == ODW_PRIM_CYLINDER) ? par[0] : (parab ? par[2] : par[1]);
      const double H = (type == ODW_PRIM_CONE) ? par[2] : par[1];
      d[0] = H + tol;
      d[1] = R1 * R1 * (1.0 - 1e-9);                                      // the cylinder's side test
      d[2] = (R1 + tol) * (R1 + tol);
      d[3] = (R2 + tol) * (R2 + tol);
    }
  }
}

// A scene the flat loop would take but for its rare quadrics (paraboloids, ellipsoids, conicoids, aspheres: build_accel gives it a grid and a
// tree, since the generic flat kernel leaves their code out): a kernel compiled against it needs neither
bool flat_but_for_rare_quadrics(const HostScene& hs, int flat_limit) {
  bool rare = false;
  for (int p = 0; p < hs.n_prims; ++p) {
    const int t = hs.prim_i32[4 * p];
    if (t == ODW_PRIM_TRIANGLE) return false;
    rare |= t == ODW_PRIM_PARABOLOID || t == ODW_PRIM_ELLIPSOID || t == ODW_PRIM_CONICOID || t == ODW_PRIM_ASPHERE;
  }
  return rare && hs.n_prims <= flat_limit;
}

// The structures a scene is traced with: none for analytic scenes of up to flat_limit primitives (the flat kernels),
// else the grid where the scene takes one, and the trees.  hs and boxes as compute_boxes(hs, dist_tol, boxes) left them.
int build_accel(const HostScene& hs, std::vector<Box> boxes, double dist_tol, int flat_limit, const BuildOptions& opt,
                SceneAccel& A, std::string& error) {
  A = SceneAccel();
  const int n = hs.n_prims;
  const std::vector<char>& dead = hs.dead;
  bool has_triangles = false, has_paraboloids = false, has_ellipsoids = false;
  for (int p = 0; p < n; ++p) {
    has_triangles |= hs.prim_i32[4 * p] == ODW_PRIM_TRIANGLE;
    has_paraboloids |= hs.prim_i32[4 * p] == ODW_PRIM_PARABOLOID;
    // (conicoids and aspheres go where ellipsoids go: known to the binary tree and the grid kernel's item branch)
    has_ellipsoids |= hs.prim_i32[4 * p] == ODW_PRIM_ELLIPSOID || hs.prim_i32[4 * p] == ODW_PRIM_CONICOID ||
                      hs.prim_i32[4 * p] == ODW_PRIM_ASPHERE;
  }
  // (triangles are only known to the BVH kernels, paraboloids to the BVH and grid kernels, ellipsoids to the binary
  //  tree and the grid kernel: beside facets they take the binary tree, not the mesh kernel's eight-wide one)
  if (n <= flat_limit && !has_triangles && !has_paraboloids && !has_ellipsoids && !opt.force_tree) return ODW_OK;
  if (!has_triangles && !opt.force_tree) build_grid(hs, boxes, A);
  // float32 traversal boxes: enlarge by what float rounding of the ray origin
  // and of the slab arithmetic can cost (see ray_box_f32 in odw_kernels.hip)
  for (int p = 0; p < n; ++p)
    for (int a = 0; a < 3; ++a) {
      const double s = 1e-4 + 4e-7 * (std::fabs(boxes[p].lo[a]) + std::fabs(boxes[p].hi[a]));
      boxes[p].lo[a] -= s;
      boxes[p].hi[a] += s;
    }
  BvhBuilder b(boxes);
  std::vector<int> ids;
  ids.reserve(n);
  for (int i = 0; i < n; ++i)
    if (!dead[i]) ids.push_back(i);
  if (ids.empty() && n > 0) ids.push_back(0);   // (a far-away box: the tree needs one leaf)
  if (!bvh_order_fits(ids.size())) {
    A = SceneAccel();
    return refuse(error, ODW_ERR_UNSUPPORTED, "more than 16777215 (2^24 - 1) primitives in the tree: a leaf word holds 24 bits of its first primitive");
  }
  b.nodes.reserve((size_t)n);
  const BvhBuilder::Ref root = b.build(ids, 0);
  if (root.count > 0) {   // everything in one leaf: wrap it into a root node
    BvhNode nd;
    for (int k = 0; k < 3; ++k) {
      nd.lo0[k] = round_down(root.box.lo[k]); nd.hi0[k] = round_up(root.box.hi[k]);
      // the second child does not exist.  Its box must be one no ray meets: an inverted box
      // (lo = +inf, hi = -inf) passes the slab test for every ray (min = -inf, max = +inf on
      // each axis) and would send the traversal back to node 0 for ever; a point far away fails
      // it for every direction
      nd.lo1[k] = 3.0e38f; nd.hi1[k] = 3.0e38f;
    }
    nd.child0 = root.child; nd.count0 = root.count;
    nd.child1 = 0; nd.count1 = 0;
    b.nodes.insert(b.nodes.begin(), nd);
  }
  if (b.max_depth + 2 > ODW_BVH_STACK) {
    A = SceneAccel();
    return refuse(error, ODW_ERR_UNSUPPORTED, "BVH deeper than the LDS stack");
  }
  // the mesh kernel's eight-wide tree and leaf records (odw_mesh.hip: ODW_LEAF_WORDS): the facet relative to the centre
  // of the leaf group of its node, in float32, with the bounds the conservative filter needs
  std::vector<float> recs;
  const bool mesh_kernel = opt.mesh_kernel;
  std::vector<int> prim_solid((size_t)n);
  for (int p = 0; p < n; ++p) prim_solid[p] = hs.prim_i32[4 * (size_t)p + 2] >> ODW_SOLID_SHIFT;
  WideBvh wide(b.nodes, b.order, prim_solid);
  std::vector<float> out_normal;
  if (has_triangles && mesh_kernel && !has_ellipsoids) {
    // normal cones for rays inside STRICTLY convex tessellated solids (ODW_FLAG_STRICTLY_CONVEX; node words 24..31;
    // ODW_MESH_CONES=0: none).  The margin: a ray that starts on a facet whose edges are all closed is out of that facet's
    // area by 1e-9 of its edges at most; every point of a facet lies on or below the plane of every other facet up to
    // rounding (what the flag says: 1e-13 of the mesh's size per edge, taken a hundred times wider here); the point itself
    // is rounded (~1e-13 of the coordinates): above a dropped facet's plane by less than `above`, met at t < above / margin.
    const bool cones_off = !opt.cones;
    double size = 0.0, reach = 0.0;
    out_normal.assign(3 * (size_t)n, std::numeric_limits<float>::quiet_NaN());
    bool any = false;
    for (int p = 0; p < n && !cones_off; ++p) {
      const int32_t* pi = &hs.prim_i32[4 * (size_t)p];
      if (pi[0] != ODW_PRIM_TRIANGLE || !(pi[2] & ODW_FLAG_CONVEX) || !(pi[2] & ODW_FLAG_STRICTLY_CONVEX)) continue;
      const double* pf = hs.prim_f64.data() + 16 * (size_t)p;
      const double sg = (pi[2] & ODW_FLAG_FLIP_NORMAL) ? -1.0 : 1.0;
      for (int a = 0; a < 3; ++a) {
        out_normal[3 * (size_t)p + a] = (float)(sg * pf[9 + a]);
        size = std::max(size, std::fabs(pf[3 + a]) + std::fabs(pf[6 + a]));
        reach = std::max(reach, std::max(std::fabs(boxes[p].lo[a]), std::fabs(boxes[p].hi[a])));
      }
      any = true;
    }
    if (any) {
      // (size: the longest facet edge, and more; the mesh is at most the extent of all such facets together: reach both ways)
      const double above = 1e-9 * size + 1e-11 * 2.0 * reach + 1e-12 * reach;
      wide.margin = std::max(0.02, 2.0 * above / std::max(dist_tol, 1e-300));
      wide.out_normal = out_normal.data();
    }
    wide.build();
    if (wide.ok) {
      recs.assign(std::max<size_t>(wide.leaf_prim.size(), 1) * ODW_LEAF_WORDS, 0.0f);
      for (size_t j = 0; j < wide.leaf_prim.size(); ++j) {
        const int p = wide.leaf_prim[j];
        float* r = &recs[j * ODW_LEAF_WORDS];
        const float* c = &wide.leaf_center[3 * j];
        const double* pf = hs.prim_f64.data() + 16 * (size_t)p;
        const int32_t* pi = &hs.prim_i32[4 * (size_t)p];
        uint32_t gs = (uint32_t)(pi[1] & 0xff) | ((uint32_t)((pi[2] >> ODW_SOLID_SHIFT) & 0x7fff) << 8);
        float smax = 0.0f, err = 0.0f;
        if (pi[0] == ODW_PRIM_TRIANGLE) {
          double l1[2] = {0.0, 0.0};
          float e1[3], e2[3];
          for (int a = 0; a < 3; ++a) {
            r[a] = (float)(pf[a] - (double)c[a]);
            e1[a] = (float)pf[3 + a];
            e2[a] = (float)pf[6 + a];
            l1[0] += std::fabs(pf[3 + a]);
            l1[1] += std::fabs(pf[6 + a]);
          }
          r[3] = e1[0]; r[4] = e1[1]; r[5] = e1[2]; r[6] = e2[0]; r[7] = e2[1]; r[8] = e2[2];
          smax = round_up(std::max(0.0, std::max(pf[12], std::max(pf[13], pf[14]))));
          err = round_up(4e-6 * std::max(l1[0], l1[1]));
        } else {
          gs |= 0x80000000u;
        }
        std::memcpy(&r[9], &gs, 4);
        r[10] = smax;
        r[11] = err;
        std::memcpy(&r[12], &p, 4);
        r[13] = c[0]; r[14] = c[1]; r[15] = c[2];
      }
      if (opt.cone_stats) {                            // (diagnostics: how many slots carry a cone)
        size_t slots = 0, cones = 0;
        for (size_t k = 0; k + kWideWords <= wide.nodes.size(); k += kWideWords)
          for (int sl = 0; sl < 8; ++sl)
            if ((wide.nodes[k + 6] | (wide.nodes[k + 6] >> 8)) & (1u << sl)) { ++slots; cones += (wide.nodes[k + 24 + sl] >> 24) != 127u; }
        fprintf(stderr, "[odw mesh cones] margin %.4g, %zu of %zu slots carry a cone\n", wide.margin, cones, slots);
      }
      for (int a = 0; a < 3; ++a) {       // node 0 as the kernel decodes it: corner + 255 units of its scale
        float corner, unit;
        const uint32_t eb = ((wide.nodes[3] >> (8 * a)) & 0xffu) << 23;
        std::memcpy(&corner, &wide.nodes[a], 4);
        std::memcpy(&unit, &eb, 4);
        A.wide_lo[a] = (double)corner;
        A.wide_hi[a] = (double)corner + 255.0 * (double)unit;
      }
      A.wide_nodes = std::move(wide.nodes);
      A.leaf_recs = std::move(recs);
    }
  }
  A.nodes = std::move(b.nodes);
  A.order = std::move(b.order);
  A.max_depth = b.max_depth;
  return ODW_OK;
}

}  // namespace
