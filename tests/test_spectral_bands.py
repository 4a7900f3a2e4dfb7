"""Spectral detector maps on the host: the band rule, the edge checks, the interface and the compiled header.

The band of a wavelength is numpy.histogram's bin of it among the detector's band edges.  The helper the GPU tests build
their expected planes with (spectral_band_cases.band_of: numpy.searchsorted) is held against numpy.histogram and
numpy.histogramdd here, and the library's host-side odw_band_index against the helper -- equal, not close."""
import numpy as np
import pytest

import spectral_band_cases as bc
import spectral_cases as sp
from freecad.optics_design_workbench_amd import _native

pytestmark = pytest.mark.usefixtures('native_lib')


def _uneven():
  return np.array([380.0, 380.5, 455.25, 600.0, 601.0, 790.125])


def _sets():
  return list(bc.EDGE_SETS.items()) + [(5, _uneven())]


@pytest.mark.parametrize('k,e', _sets(), ids=lambda v: str(v) if isinstance(v, int) else '')
def test_helper_against_numpy_histogram(k, e):
  """every edge, one ulp on either side of every edge, below e_0, above e_K, exactly e_K, and a uniform draw: the counts per
  band of the helper's indices are numpy.histogram's, and wavelength by wavelength the index is the one numpy.histogram
  gives that wavelength alone"""
  assert len(e) == k + 1
  wl = bc.probes(e, 2000)
  b = bc.band_of(e, wl)
  assert b.dtype == np.int32 and b.min() == -1 and b.max() == k - 1
  assert np.array_equal(np.bincount(b[b >= 0], minlength=k), np.histogram(wl, bins=e)[0])
  for w, bw in zip(wl[:3 * (k + 1) + 5], b):
    h = np.histogram([w], bins=e)[0]
    assert h.sum() == (1 if bw >= 0 else 0) and (bw < 0 or h[bw] == 1), (w, bw)
  # the named cases
  assert np.array_equal(bc.band_of(e, e), np.r_[np.arange(k), k - 1])                         # on every edge; e_K folds into K - 1
  assert np.array_equal(bc.band_of(e, np.nextafter(e, -np.inf)), np.r_[-1, np.arange(k)])     # one ulp below
  assert np.array_equal(bc.band_of(e, np.nextafter(e, np.inf)), np.r_[np.arange(k), -1])      # one ulp above
  assert bc.band_of(e, [np.nan])[0] == -1


def test_helper_planes_against_numpy_histogramdd():
  """the helper's band planes of made-up rows are numpy.histogramdd over (wavelength, x, y) with the detector's edges"""
  import power_scene
  det = power_scene.DETECTOR
  rs = np.random.RandomState(5)
  n = 4000
  rows = np.zeros(n, dtype=_native.HIT_DTYPE)
  rows['point'] = rs.uniform(-24.0, 24.0, (n, 3))
  rows['power'] = rs.uniform(0.0, 1.0, n)
  e = bc.EDGE_SETS[7]
  wl = bc.wavelengths(e, n)
  counts, power, outside = bc.band_planes(rows, wl, e, det)
  r = rows['point'] - np.asarray(det['origin'])
  xe = np.linspace(det['x_lo'], det['x_hi'], det['nx'] + 1)
  ye = np.linspace(det['y_lo'], det['y_hi'], det['ny'] + 1)
  ix, iy, inside = power_scene.detector_bins(rows['point'], det)
  # (histogramdd closes the last bin of every axis on the right; the detector does not: no point lies on x_hi / y_hi here)
  assert not np.any(r[:, 0] == det['x_hi']) and not np.any(r[:, 1] == det['y_hi'])
  want, _ = np.histogramdd(np.stack([wl, r[:, 0], r[:, 1]], axis=1), bins=(e, xe, ye))
  assert np.array_equal(counts, want.astype(np.uint64)) and counts.sum() > 1000
  wantp, _ = np.histogramdd(np.stack([wl, r[:, 0], r[:, 1]], axis=1), bins=(e, xe, ye), weights=power_scene.quanta(rows['power']).astype(np.float64))
  assert np.array_equal(power, wantp.astype(np.uint64))          # (sums below 2^53: exact in float64)
  assert outside == int((inside & (bc.band_of(e, wl) < 0)).sum()) > 0


@pytest.mark.parametrize('k,e', _sets(), ids=lambda v: str(v) if isinstance(v, int) else '')
def test_band_index_on_the_host(k, e):
  wl = np.r_[bc.probes(e, 3000), np.nan, np.inf, -np.inf, 0.0, -500.0]
  got = _native.band_index(e, wl)
  assert got.dtype == np.int32 and np.array_equal(got, bc.band_of(e, wl))
  from freecad.optics_design_workbench_amd.simulation.tracer import Tracer
  assert np.array_equal(Tracer.bandIndex(e, wl), got)
  assert _native.band_index(e, np.empty(0)).shape == (0,)


def test_edges_are_refused_by_name():
  """odw_set_detector_bands' check of the edges, reached without a context (a null context checks and sets nothing)"""
  _native.band_edges_check([450.0, 540.0])
  _native.band_edges_check(bc.EDGE_SETS[64])
  for bad, what in (([450.0, np.nan, 600.0], r'band edge 1 \(nan nm\) is not finite'),
                    ([450.0, np.inf], r'band edge 1 \(inf nm\) is not finite'),
                    ([0.0, 500.0], r'band edge 0 \(0 nm\) is not positive'),
                    ([-1.0, 500.0], r'band edge 0 \(-1 nm\) is not positive'),
                    ([450.0, 540.0, 540.0], r'band edge 2 \(540 nm\) is not above its predecessor'),
                    ([450.0, 540.0, 500.0], r'band edge 2 \(500 nm\) is not above its predecessor'),
                    ([500.0], 'band edges: at least two edges'),
                    (np.linspace(400.0, 700.0, 67), '66 bands: a detector takes at most ODW_BAND_MAX = 64'),
                    (bc.edges(65), '65 bands: a detector takes at most ODW_BAND_MAX = 64')):
    with pytest.raises(_native.NativeError, match='odw_set_detector_bands: ' + what):
      _native.band_edges_check(bad)
    with pytest.raises(_native.NativeError, match='odw_band_index: ' + what):
      _native.band_index(bad, [500.0])


def test_symbols_and_abi():
  new = ('odw_set_detector_bands', 'odw_fetch_band_histogram', 'odw_fetch_band_power_histogram', 'odw_device_band_histogram',
         'odw_band_index', 'odw_compiled_bands_info', 'odw_compile_check_bands')
  header = open(_native._HEADER).read()
  for name in new:
    assert name in _native.SYMBOLS and hasattr(_native.lib(), name)
    assert f'int {name}(' in header, name
  assert _native.lib().odw_abi_version() == _native.ABI_VERSION
  assert f'#define ODW_ABI_VERSION {_native.ABI_VERSION}\n' in header
  assert '#define ODW_TRACE_BAND_HISTOGRAM 0x10 ' in header and _native.TRACE_BAND_HISTOGRAM == 0x10
  assert '#define ODW_BAND_MAX 64 ' in header and _native.BAND_MAX == 64
  # the flag is a bit of its own beside the others
  flags = [_native.TRACE_RECORD_HITS, _native.TRACE_HISTOGRAM, _native.TRACE_RECORD_SEGMENTS, _native.TRACE_POWER_HISTOGRAM,
           _native.TRACE_BAND_HISTOGRAM]
  assert sum(flags) == 31 and all(f & (f - 1) == 0 for f in flags)


def test_compiled_bands_header():
  """the compiled kernel's variant for band planes: its header is the CHROMA header with ODW_SPEC_BANDS defined behind
  ODW_SPEC_CHROMA (and img_fits counted for the longer third argument) and compiles for gfx950, with and without the power
  plane; without bands the CHROMA header is what it is without this feature: no line of it knows about bands"""
  sc, lim, src = sp.scene()
  chroma, n0 = _native.compile_check_chroma(sc, lim, source=src)
  assert 'BANDS' not in chroma and 'bands' not in chroma and n0 > 10000
  h, n = _native.compile_check_bands(sc, lim, source=src)
  assert n > n0                                               # (the band search and its atomics are in the code)
  assert '#define ODW_SPEC_CHROMA true\n#define ODW_SPEC_BANDS true\n' in h
  # ... and that line is the only difference (the bench's value image fits the kernel arguments either way)
  assert h.replace('#define ODW_SPEC_BANDS true\n', '') == chroma
  hp, npw = _native.compile_check_bands(sc, lim, source=src, power=True)
  assert hp == h + '#define ODW_SPEC_POWER true\n' and npw > n
  # the header of every other launch stays what it is
  plain, _ = _native.compile_check(sc, lim, 'structure', source=src)
  assert 'BANDS' not in plain and 'CHROMA' not in plain
