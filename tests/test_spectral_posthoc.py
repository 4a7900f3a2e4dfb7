"""Post-hoc band histograms without a device: the host mirror `Hits.histogram(bands=)` against numpy, and the native entry
points that answer without a GPU (tests/test_gpu_spectral_posthoc.py holds the kernel).

The host mirror splits the hits of one plane by the `initWavelength` column, numpy.histogram's rule on the band edges
(spectral_band_cases.band_of); every comparison of counts is an integer equality."""
import ctypes as C
import os

import numpy as np
import pytest

import spectral_band_cases as bc
from freecad.optics_design_workbench_amd import _native
from freecad.optics_design_workbench_amd.jupyter_utils import BandHistograms, Hits
from freecad.optics_design_workbench_amd.jupyter_utils.histogram import bandOf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1025


def _hits(k, wavelengths=True):
  """1025 rows on a slightly tilted plane, powers in (0, 1], the probe wavelengths of edge set k"""
  rs = np.random.RandomState(5)
  xy = rs.normal(0.0, 3.0, (N, 2))
  pts = np.stack([xy[:, 0], xy[:, 1], 40.0 + 1e-3 * xy[:, 0]], axis=1)
  dirs = np.tile([0.0, 0.0, 1.0], (N, 1)) + 0.01 * rs.normal(0, 1, (N, 3))
  d = dict(points=pts, directions=dirs, powers=rs.uniform(0.1, 1.0, N), isEntering=np.ones(N, dtype=np.int64))
  if wavelengths:
    d['initWavelength'] = bc.wavelengths(bc.EDGE_SETS[k], N)
  return d


def _coords(h, x, y):
  a, b = x - h._origin[0], y - h._origin[1]
  return (np.arctan2(a, b), np.sqrt(a**2 + b**2)) if h._binCoords == 'polar' else (a, b)


@pytest.mark.parametrize('kwargs', [dict(), dict(bins=(3, 5)), dict(binCoords='polar', bins=[np.linspace(-np.pi, np.pi, 7), 8]),
                                    dict(weights='powers', bins=12)], ids=['default', '3x5', 'polar', 'powers'])
@pytest.mark.parametrize('k', [1, 7, 64])
def test_host_bands_against_numpy(k, kwargs):
  e = bc.EDGE_SETS[k]
  d = _hits(k)
  wl = d['initWavelength']
  assert set(e) <= set(wl) and (bc.band_of(e, wl) < 0).sum() >= 6
  hits = Hits(d)
  got = hits.histogram(bands=e, **kwargs)
  plain = hits.histogram(**kwargs)
  assert isinstance(got, BandHistograms) and len(got) == k == len(got.bands) and got[0] is got.bands[0]
  assert np.array_equal(got.edges, e)
  # the total is the call without bands
  for name in ('hist', 'binX', 'binY', '_origin'):
    assert np.array_equal(getattr(got.total, name), getattr(plain, name)), name
  x, y, _, _ = hits._flat('points', got.total._planeNormal, got.total._xInPlaneVec)
  a, b = _coords(got.total, x, y)
  band = bc.band_of(e, wl)
  assert np.array_equal(band, bandOf(e, wl))
  w = d['powers'] if 'weights' in kwargs else None
  grid = [got.total.binX, got.total.binY]
  for j in range(k):
    s = band == j
    want = np.histogram2d(a[s], b[s], bins=grid, weights=None if w is None else w[s])[0]
    assert np.array_equal(got[j].hist, want), j
    assert np.array_equal(got[j].binX, plain.binX) and np.array_equal(got[j].binY, plain.binY)
    assert np.array_equal(got[j]._origin, plain._origin) and got[j]._binCoords == plain._binCoords
  # bin by bin: bands + rows in no band = total (counts)
  none = np.histogram2d(a[band < 0], b[band < 0], bins=grid)[0]
  counts = np.histogram2d(a, b, bins=grid)[0]
  per_band = [np.histogram2d(a[band == j], b[band == j], bins=grid)[0] for j in range(k)]
  assert np.array_equal(sum(per_band) + none, counts)
  assert got.noBand == int(none.sum()) > 0
  if w is None:
    assert np.array_equal(sum(h.hist for h in got.bands) + none, got.total.hist)
    assert int(got.total.hist.sum()) - int(sum(h.hist.sum() for h in got.bands)) == got.noBand


def test_host_refusals():
  e = bc.EDGE_SETS[7]
  with pytest.raises(KeyError, match='StoreHitInitWavelength'):
    Hits(_hits(7, wavelengths=False)).histogram(bands=e)
  hits = Hits(_hits(7))
  for bad in ([500.0], [500.0, 500.0], [600.0, 500.0], [0.0, 500.0], [400.0, np.inf], [400.0, np.nan, 700.0], bc.edges(65)):
    with pytest.raises(ValueError, match='bands'):
      hits.histogram(bands=bad)
  # without the keyword nothing changes
  assert type(hits.histogram()).__name__ == 'Histogram'


# ---- native calls that need no device ---------------------------------------------------------------------------------
def test_symbols(native_lib):
  with open(os.path.join(ROOT, 'include', 'odw_trace.h')) as f:
    header = f.read()
  for name in ('odw_hits_bin_bands', 'odw_hits_bin_bands_info'):
    assert f'int {name}(' in header and name in _native.SYMBOLS
    assert getattr(native_lib, name) is not None
  assert 'enum { ODW_ROW_WL_SPECTRUM = 1, ODW_ROW_WL_TABLE = 2 };' in header
  assert (_native.ROW_WL_SPECTRUM, _native.ROW_WL_TABLE) == (1, 2)


def test_null_context_is_refused(native_lib):
  pd, pu = C.POINTER(C.c_double), C.POINTER(C.c_uint64)
  f = native_lib.odw_hits_bin_bands
  f.argtypes = [C.c_void_p, C.c_int32, pd, pd, C.c_int32, pd, C.c_int32, pd, C.c_int32, C.c_int32, C.c_uint64, C.c_uint64,
                C.c_uint64, pd, pu, pu, pu]
  origin, ea, eb, be = np.zeros(2), np.linspace(-1, 1, 4), np.linspace(-1, 1, 4), bc.EDGE_SETS[7]
  counts, none = np.zeros(9 * 8, dtype=np.uint64), C.c_uint64(0)
  rc = f(None, 0, origin.ctypes.data_as(pd), ea.ctypes.data_as(pd), 4, eb.ctypes.data_as(pd), 4, be.ctypes.data_as(pd), len(be),
         _native.ROW_WL_SPECTRUM, 1, 0, 0, None, counts.ctypes.data_as(pu), None, C.byref(none))
  assert rc == 1                                    # ODW_ERR_INVALID
  assert b'odw_hits_bin_bands' in native_lib.odw_last_error(None)


def _info(lib, n_a, n_b, n_band_edges, power=0):
  f = lib.odw_hits_bin_bands_info
  f.argtypes = [C.c_int32] * 4 + [C.POINTER(C.c_int32)] * 2
  c, p = C.c_int32(-1), C.c_int32(-1)
  rc = f(n_a, n_b, n_band_edges, power, C.byref(c), C.byref(p))
  return rc, c.value, p.value


def test_route_info_without_a_device(native_lib, monkeypatch):
  monkeypatch.delenv('ODW_BIN_BANDS_HBM', raising=False)
  assert _info(native_lib, 11, 11, 8) == (0, 1, 0)             # 8 planes of 100 bins: the LDS window
  assert _info(native_lib, 31, 31, 65) == (0, 0, 0)            # 65 planes of 900 bins: HBM atomics
  assert _info(native_lib, 11, 11, 8, power=1) == (0, 1, 0)    # (the power planes: HBM either way)
  # the border: (K + 1) * nbins = 8192 words still fit
  assert _info(native_lib, 65, 65, 2)[1] == 1 and _info(native_lib, 65, 66, 2)[1] == 0
  rc, _, _ = _info(native_lib, 11, 11, 67)                     # K = 66
  assert rc == 1
  rc, _, _ = _info(native_lib, 11, 11, 66)                     # K = 65: one more than ODW_BAND_MAX
  assert rc == 1 and b'65 bands' in native_lib.odw_last_error(None)
  assert _info(native_lib, 11, 11, 1)[0] == 1 and _info(native_lib, 1, 11, 8)[0] == 1
  monkeypatch.setenv('ODW_BIN_BANDS_HBM', '1')
  assert _info(native_lib, 11, 11, 8) == (0, 0, 0)
