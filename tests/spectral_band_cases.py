"""Band edges, probe wavelengths and numpy's band planes for the spectral detector maps (tests/test_spectral_bands.py,
tests/test_gpu_spectral_bands.py).

The band of a wavelength among edges e_0 < ... < e_K is numpy.histogram's: e_b <= wl < e_(b+1), wl == e_K in band K - 1,
nothing outside [e_0, e_K].  `band_of` says so with numpy.searchsorted; tests/test_spectral_bands.py holds it against
numpy.histogram itself.  The detector bin of a row is power_scene.detector_bins, its weight power_scene.quanta."""
import numpy as np

import power_scene

LINE_EDGES = np.array([450.0, 540.0, 620.0, 700.0])      # F (486.1), d (587.6), C (656.3): one line per band


def edges(k):
  """k uneven bands over the visible: e_j = 400 + 350 (j / k)^1.7, nudged by a fixed irrational-looking amount so that no
  edge is a round number"""
  j = np.arange(k + 1, dtype=np.float64)
  e = 400.0 + 350.0 * (j / k) ** 1.7 + 0.0137 * np.sin(1.0 + 3.0 * j)
  assert np.all(np.diff(e) > 0)
  return e


EDGE_SETS = {k: edges(k) for k in (1, 3, 7, 64)}


def band_of(e, wl):
  """int32 band of every wavelength, -1: none"""
  e = np.asarray(e, np.float64)
  wl = np.asarray(wl, np.float64)
  b = np.searchsorted(e, wl, 'right') - 1
  b = np.where(wl == e[-1], len(e) - 2, b)
  b = np.where((wl < e[0]) | (wl > e[-1]) | np.isnan(wl), -1, b)
  return b.astype(np.int32)


def probes(e, n_uniform=0, seed=11):
  """every edge, its two float64 neighbours, values below e_0 and above e_K, e_K itself once more, then n_uniform draws
  between e_0 and e_K"""
  e = np.asarray(e, np.float64)
  fixed = np.concatenate([e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf),
                          [e[0] - 30.0, e[0] * 0.5, e[-1] + 25.0, e[-1] * 1.1, e[-1]]])
  rs = np.random.RandomState(seed)
  return np.concatenate([fixed, rs.uniform(e[0], e[-1], n_uniform)])


def wavelengths(e, n, seed=11):
  """n wavelengths for a launch: the probes (repeated where n is small: the first n of them), the rest uniform"""
  p = probes(e)
  if n <= len(p):
    return p[:n].copy()
  return probes(e, n - len(p), seed)


def band_planes(rows, wl, e, det):
  """(band count planes (K, nx, ny), band power planes in quanta, binned hits whose wavelength lies in no band) of hit rows
  with the wavelength of every row, with numpy"""
  k = len(e) - 1
  ix, iy, inside = power_scene.detector_bins(rows['point'], det)
  if det.get('group', -1) >= 0:
    grp = ((rows['tag'] >> np.uint64(48)) & np.uint64(0x7FFF)).astype(np.int64)
    inside = inside & (grp == det['group'])
  b = band_of(e, wl)
  sel = inside & (b >= 0)
  counts = np.zeros((k, det['nx'], det['ny']), dtype=np.uint64)
  power = np.zeros_like(counts)
  np.add.at(counts, (b[sel], ix[sel], iy[sel]), np.uint64(1))
  np.add.at(power, (b[sel], ix[sel], iy[sel]), power_scene.quanta(rows['power'][sel]))
  return counts, power, int((inside & (b < 0)).sum())


def ray_of(rows):
  return (rows['tag'] & np.uint64(0xFFFFFFFFFFFF)).astype(np.int64)
