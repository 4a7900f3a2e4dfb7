"""Post-hoc band histograms on the device: `DeviceHits.histogram(bands=)` -> `odw_hits_bin_bands` -> ph_bin_bands_kernel.

Expected planes come from numpy alone: the launch's own rows (`tr.hits()`), the wavelength of a row from its ray number
(the launch's table, or `Tracer.rayWavelengths`), its band from spectral_band_cases.band_of, its bin from
numpy.histogram2d over the returned histogram's own plane, origin and edges (those are held equal to the host `Hits` by
tests/test_gpu_device_hits.py), its weight from power_scene.quanta.  Every comparison of counts is an integer equality."""
import ctypes as C

import numpy as np
import pytest

import power_scene
import spectral_band_cases as bc
import spectral_cases as sp
from freecad.optics_design_workbench_amd import _native
from freecad.optics_design_workbench_amd.jupyter_utils import BandHistograms
from test_gpu_spectral import SEED, SOURCE, THREE_LINES
from test_gpu_spectral_bands import DENSITY, GEN_EDGES

pytestmark = pytest.mark.gpu
N, FIRST = 1025, 1000
GROUP_MASK = np.uint64(0x7FFF)


def _tracer(compile='off'):
  from freecad.optics_design_workbench_amd.simulation.tracer import Tracer
  tr = Tracer(0)
  tr.compileScene(compile)
  return tr


def _launch(tr, o, d, wl, first=FIRST):
  tr.setDetector(None)
  tr.reserveHits(max(len(o), 64) * 8)
  tr.reset()
  tr.traceRays(o, d, first=first, wavelengths=wl, histogram=False)
  tr.sync()
  assert tr.counters()['hits_dropped'] == 0
  return tr.hits()


def _in_lds(lib, n_a, n_b, n_band_edges):
  f = lib.odw_hits_bin_bands_info
  f.argtypes = [C.c_int32] * 4 + [C.POINTER(C.c_int32)] * 2
  c, p = C.c_int32(-1), C.c_int32(-1)
  assert f(n_a, n_b, n_band_edges, 0, C.byref(c), C.byref(p)) == 0
  return bool(c.value)


def _bin_of(edges, v):
  """numpy.histogramdd's rule: searchsorted(edges, v, 'right') - 1, the last edge closed; -1: outside"""
  i = np.searchsorted(edges, v, 'right') - 1
  i = np.where(v == edges[-1], len(edges) - 2, i)
  return np.where((v >= edges[0]) & (v <= edges[-1]), i, -1)


def _expected(rows, wl_rows, e, H, key='points'):
  """(band counts (K, na, nb), total counts, band quanta, total quanta, binned rows in no band) of `rows` over the plane,
  origin and edges of the histogram H, with numpy; the projection sums its three products left to right, as the kernel
  says it does (csrc/odw_posthoc.hip: ph_project_kernel)"""
  ex = np.asarray(H._xInPlaneVec, dtype=np.float64)
  ey = np.cross(H._planeNormal, H._xInPlaneVec)
  ex, ey = ex / np.linalg.norm(ex), ey / np.linalg.norm(ey)
  p = rows['point'] if key == 'points' else rows['direction']
  x = p[:, 0] * ex[0] + p[:, 1] * ex[1] + p[:, 2] * ex[2]
  y = p[:, 0] * ey[0] + p[:, 1] * ey[1] + p[:, 2] * ey[2]
  a, b = x - H._origin[0], y - H._origin[1]
  if H._binCoords == 'polar':
    a, b = np.arctan2(a, b), np.sqrt(a * a + b * b)
  k = len(e) - 1
  band = bc.band_of(e, wl_rows)
  grid = [H.binX, H.binY]
  counts = np.array([np.histogram2d(a[band == j], b[band == j], bins=grid)[0] for j in range(k)]).astype(np.uint64)
  total = np.histogram2d(a, b, bins=grid)[0].astype(np.uint64)
  ia, ib = _bin_of(H.binX, a), _bin_of(H.binY, b)
  inside = (ia >= 0) & (ib >= 0)
  q = power_scene.quanta(rows['power'])
  qt = np.zeros(total.shape, dtype=np.uint64)
  np.add.at(qt, (ia[inside], ib[inside]), q[inside])
  qb = np.zeros(counts.shape, dtype=np.uint64)
  s = inside & (band >= 0)
  np.add.at(qb, (band[s], ia[s], ib[s]), q[s])
  return counts, total, qb, qt, int((inside & (band < 0)).sum())


def _same_histogram(a, b, plane=True):
  for name in ('hist', 'binX', 'binY', '_origin') + (('_planeNormal', '_xInPlaneVec') if plane else ()):
    assert np.array_equal(getattr(a, name), getattr(b, name)), name
  assert a._binCoords == b._binCoords
  assert (a.powerQuanta is None) == (b.powerQuanta is None)
  if a.powerQuanta is not None:
    assert np.array_equal(a.powerQuanta, b.powerQuanta)


def _check(got, rows, wl_rows, e, weighted, key='points'):
  """a BandHistograms against numpy on the rows it binned -> (band counts or quanta, noBand)"""
  k = len(e) - 1
  assert isinstance(got, BandHistograms) and len(got) == k and np.array_equal(got.edges, e)
  counts, total, qb, qt, none = _expected(rows, wl_rows, e, got.total, key)
  for h in got.bands:
    assert np.array_equal(h.binX, got.total.binX) and np.array_equal(h.binY, got.total.binY)
    assert np.array_equal(h._origin, got.total._origin) and h._binCoords == got.total._binCoords
  assert got.noBand == none
  if weighted:
    assert np.array_equal(got.total.powerQuanta, qt)
    for j in range(k):
      assert got[j].powerQuanta.dtype == np.uint64 and np.array_equal(got[j].powerQuanta, qb[j]), j
      assert np.array_equal(got[j].hist, qb[j].astype(np.float64) * 2.0 ** -32)
    return qb, none
  assert np.array_equal(got.total.hist, total.astype(np.float64))
  for j in range(k):
    assert got[j].powerQuanta is None and np.array_equal(got[j].hist, counts[j].astype(np.float64)), j
  # bin by bin: the bands and the rows in no band add up to the total
  assert np.array_equal(total - counts.sum(0), got.total.hist.astype(np.uint64) - sum(h.hist for h in got.bands).astype(np.uint64))
  assert int(total.sum()) - int(counts.sum()) == none
  return counts, none


# 70 edges a side: 4761 bins -- with two planes (K = 1) already beyond the LDS window's 8192 words
_BIG = [np.linspace(-260.0, 260.0, 70), np.linspace(-30.0, 30.0, 70)]
BINNINGS = {
    'bins10': dict(bins=10),
    '3x5': dict(bins=(3, 5)),
    'arrays': dict(bins=_BIG),
    'polar6': dict(binCoords='polar', bins=[np.linspace(-np.pi, np.pi, 6), np.geomspace(1e-3, 300.0, 9)]),      # the tables
    'polar12': dict(binCoords='polar', bins=[np.linspace(-np.pi, np.pi, 12), np.linspace(0.0, 300.0, 7)]),     # atan2, the search
}
_SIZES = {'bins10': (11, 11), '3x5': (4, 6), 'arrays': (70, 70), 'polar6': (6, 9), 'polar12': (12, 7)}
_ROWS = {}              # k -> the rows of the first compile mode (both modes: the same rows bit for bit)


# ---- 1. explicit wavelengths -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('compile', ['off', 'structure'])
@pytest.mark.parametrize('k', [1, 7, 64])
def test_explicit_wavelengths(native_lib, monkeypatch, compile, k):
  """1025 rays (first = 1000) whose wavelengths sit on every band edge, one ulp either side of it, below e_0, above e_K and
  on e_K: five binnings, with and without weights='powers', all groups and one named group; both count routes; launches
  of the first 1, 63, 64 and 65 rays"""
  monkeypatch.delenv('ODW_BIN_BANDS_HBM', raising=False)
  monkeypatch.delenv('ODW_BIN_PLAIN', raising=False)
  sc, lim, _ = sp.scene()
  o, d = sp.all_rays(N)
  e = bc.EDGE_SETS[k]
  wl = bc.wavelengths(e, N)
  # both routes are among the sizes
  routes = {name: _in_lds(native_lib, na, nb, k + 1) for name, (na, nb) in _SIZES.items()}
  assert routes['bins10'] and routes['3x5'] and not routes['arrays']
  assert _in_lds(native_lib, 11, 11, 8) and not _in_lds(native_lib, 31, 31, 65)
  tr = _tracer(compile)
  try:
    tr.setScene(sc)
    tr.setLimits(lim)
    rows = _launch(tr, o, d, wl)
    assert tr.hitProvenance()[0] == 'table' and tr.hitProvenance()[1] == FIRST
    if k in _ROWS:
      for col in ('point', 'direction', 'power', 'tag'):
        assert np.array_equal(rows[col], _ROWS[k][col]), col
    _ROWS.setdefault(k, rows)
    ray = bc.ray_of(rows)
    assert ray.min() >= FIRST and ray.max() < FIRST + N
    grp = ((rows['tag'] >> np.uint64(48)) & GROUP_MASK).astype(np.int64)
    detectors = sc.group_index('Detectors_')
    for group in (None, 'Detectors_'):
      mine = rows if group is None else rows[grp == detectors]
      w_rows = wl[bc.ray_of(mine) - FIRST]
      assert len(mine) > 300
      dh = tr.deviceHits(group)
      assert len(dh) == len(mine)
      for name, kw in BINNINGS.items():
        for weighted in (False, True):
          kw2 = dict(kw, weights='powers') if weighted else kw
          got = dh.histogram(bands=e, **kw2)
          _same_histogram(got.total, dh.histogram(**kw2))              # the plain call: plane, origin, edges, counts
          planes, none = _check(got, mine, w_rows, e, weighted)
          assert got.total.hist.shape == (_SIZES[name][0] - 1, _SIZES[name][1] - 1)
          if name in ('bins10', '3x5'):
            assert none > 0 and planes.sum() > 300
          if name == 'bins10' and not weighted:
            # the other route for the same call
            monkeypatch.setenv('ODW_BIN_BANDS_HBM', '1')
            assert not _in_lds(native_lib, 11, 11, k + 1)
            forced = dh.histogram(bands=e, **kw2)
            monkeypatch.delenv('ODW_BIN_BANDS_HBM')
            _same_histogram(forced.total, got.total)
            assert forced.noBand == got.noBand
            for a, b in zip(forced.bands, got.bands):
              _same_histogram(a, b)
      # directions, and the polar tables switched off
      got = dh.histogram(bands=e, key='directions', bins=(4, 3))
      _same_histogram(got.total, dh.histogram(key='directions', bins=(4, 3)))
      _check(got, mine, w_rows, e, False, key='directions')
      got = dh.histogram(bands=e, radius=40.0, bins=8)
      _same_histogram(got.total, dh.histogram(radius=40.0, bins=8))
      _check(got, mine, w_rows, e, False)
    # array weights: the device route does not take them
    with pytest.raises(TypeError):
      tr.deviceHits().histogram(bands=e, weights=np.ones(len(rows)))
    # launches of the first m rays give the planes of those rays (a fixed plane: one ray's hits span none)
    plane = dict(planeNormal=np.array([0.0, 0.0, -1.0]), xInPlaneVec=np.array([1.0, 0.0, 0.0]), origin=np.zeros(2), bins=_BIG)
    for m in (1, 63, 64, 65):
      part = _launch(tr, o[:m], d[:m], wl[:m])
      first = rows[bc.ray_of(rows) < FIRST + m]
      assert len(part) == len(first) > 0 and np.array_equal(part['tag'], first['tag'])
      got = tr.deviceHits().histogram(bands=e, weights='powers', **plane)
      _check(got, part, wl[bc.ray_of(part) - FIRST], e, True)
      got = tr.deviceHits().histogram(bands=e, **dict(plane, bins=(3, 5)))
      _check(got, part, wl[bc.ray_of(part) - FIRST], e, False)
  finally:
    tr.close()


# ---- 2. generated rays ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('compile', ['off', 'structure'])
@pytest.mark.parametrize('spectrum', ['density', 'lines'])
def test_generated_rays(native_lib, monkeypatch, compile, spectrum):
  """20000 rays of a point source under a SpectralDensity / under three lines: the planes against numpy with
  Tracer.rayWavelengths; two launches of 10000 rays into one hit list give the same planes; a wrong seed gives other band
  planes under the same total"""
  monkeypatch.delenv('ODW_BIN_BANDS_HBM', raising=False)
  n, first = 20000, 5 << 20
  props = DENSITY if spectrum == 'density' else dict(Spectrum=THREE_LINES)
  e = GEN_EDGES if spectrum == 'density' else bc.LINE_EDGES
  k = len(e) - 1
  sc, lim, src = sp.scene(source=dict(SOURCE, **props))
  tr = _tracer(compile)
  try:
    tr.setScene(sc)
    tr.setLimits(lim)
    tr.setSource(src)
    tr.setDetector(None)
    tr.reserveHits(n * 8)

    def launch(parts):
      tr.reset()
      for a, m in parts:
        tr.trace(a, m, SEED, histogram=False)
      tr.sync()

    launch([(first, n)])
    assert tr.hitProvenance() == ('seed', SEED)
    rows = tr.hits()
    assert tr.counters()['hits_dropped'] == 0 and len(rows) > 1000
    w_rows = tr.rayWavelengths(bc.ray_of(rows).astype(np.uint64), SEED)
    results = {}
    for name, kw in (('lds', dict(bins=10)), ('hbm', dict(bins=[np.linspace(-20.0, 20.0, 70), np.linspace(-20.0, 20.0, 70)])),
                     ('polar', BINNINGS['polar6'])):
      for weighted in (False, True):
        kw2 = dict(kw, weights='powers') if weighted else kw
        dh = tr.deviceHits()
        got = dh.histogram(bands=e, **kw2)
        _same_histogram(got.total, dh.histogram(**kw2))
        planes, none = _check(got, rows, w_rows, e, weighted)
        results[name, weighted] = (got, planes)
        if name == 'lds':
          assert all(planes[b].any() for b in range(k)) and (none > 0) == (spectrum == 'density')
    assert _in_lds(native_lib, 11, 11, k + 1) and not _in_lds(native_lib, 70, 70, k + 1)
    # a wrong seed: other wavelengths, so other band planes -- under the same total
    dh = tr.deviceHits()
    wrong = dh.histogram(bands=e, bins=10, wavelengths={'seed': SEED + 1})
    _same_histogram(wrong.total, results['lds', False][0].total)
    assert any(not np.array_equal(a.hist, b.hist) for a, b in zip(wrong.bands, results['lds', False][0].bands))
    _check(wrong, rows, tr.rayWavelengths(bc.ray_of(rows).astype(np.uint64), SEED + 1), e, False)
    # the same seed named explicitly: the noted provenance's planes
    named = tr.deviceHits().histogram(bands=e, bins=10, wavelengths={'seed': SEED})
    for a, b in zip(named.bands, results['lds', False][0].bands):
      _same_histogram(a, b)
    # two launches appended to one hit list
    launch([(first, n // 2), (first + n // 2, n - n // 2)])
    assert tr.hitProvenance() == ('seed', SEED)
    for name, kw in (('lds', dict(bins=10)), ('hbm', dict(bins=[np.linspace(-20.0, 20.0, 70), np.linspace(-20.0, 20.0, 70)]))):
      both = tr.deviceHits().histogram(bands=e, weights='powers', **kw)
      _same_histogram(both.total, results[name, True][0].total)
      assert both.noBand == results[name, True][0].noBand
      for a, b in zip(both.bands, results[name, True][0].bands):
        _same_histogram(a, b)
  finally:
    tr.close()


# ---- 3. provenance -----------------------------------------------------------------------------------------------------
def test_provenance_refusals(native_lib):
  sc, lim, src = sp.scene(source=dict(SOURCE, Spectrum=THREE_LINES))
  o, d = sp.all_rays(N)
  e = bc.EDGE_SETS[7]
  wl = bc.wavelengths(e, N)
  tr = _tracer('off')
  try:
    tr.setScene(sc)
    tr.setLimits(lim)
    tr.setDetector(None)
    tr.reserveHits(1 << 16)
    tr.setWavelength(550.0)
    # nothing recorded yet
    assert tr.hitProvenance() is None
    # a monochromatic launch
    tr.reset()
    tr.traceRays(o, d, first=FIRST, histogram=False)
    tr.sync()
    assert tr.hitProvenance()[0] == 'mono'
    with pytest.raises(ValueError, match='monochromatic.*wavelengths='):
      tr.deviceHits().histogram(bands=e)
    assert type(tr.deviceHits().histogram()).__name__ == 'Histogram'            # (without the keyword nothing changes)
    # ... into which a spectral launch is appended
    tr.traceRays(o, d, first=FIRST + N, wavelengths=wl, histogram=False)
    tr.sync()
    assert tr.hitProvenance()[0] == 'mixed'
    with pytest.raises(ValueError, match='monochromatic and spectral.*wavelengths='):
      tr.deviceHits().histogram(bands=e)
    # contiguous tables extend each other, a gap mixes
    tr.reset()
    assert tr.hitProvenance() is None
    tr.traceRays(o[:500], d[:500], first=FIRST, wavelengths=wl[:500], histogram=False)
    tr.traceRays(o[500:], d[500:], first=FIRST + 500, wavelengths=wl[500:], histogram=False)
    tr.sync()
    prov = tr.hitProvenance()
    assert prov[0] == 'table' and prov[1] == FIRST and np.array_equal(prov[2], wl)
    rows = tr.hits()
    got = tr.deviceHits().histogram(bands=e, bins=10)
    _check(got, rows, wl[bc.ray_of(rows) - FIRST], e, False)
    tr.traceRays(o[:10], d[:10], first=FIRST + N + 7, wavelengths=wl[:10], histogram=False)
    tr.sync()
    with pytest.raises(ValueError, match='not contiguous'):
      tr.deviceHits().histogram(bands=e)
    # a table that does not cover a row's ray: refused by the library, with the count
    tr.resetHits()
    assert tr.hitProvenance() is None
    tr.traceRays(o, d, first=FIRST, wavelengths=wl, histogram=False)
    tr.sync()
    rows = tr.hits()
    short = int((bc.ray_of(rows) < FIRST + 5).sum()) + int((bc.ray_of(rows) >= FIRST + N - 3).sum())
    assert short > 0
    with pytest.raises(_native.NativeError, match=f'odw_hits_bin_bands: {short} selected row'):
      tr.deviceHits().histogram(bands=e, bins=10, wavelengths=(FIRST + 5, wl[5:N - 3]))
    with pytest.raises(_native.NativeError, match='not positive and finite'):
      tr.deviceHits().histogram(bands=e, bins=10, wavelengths=(FIRST, np.where(np.arange(N) == 17, np.nan, wl)))
    with pytest.raises(_native.NativeError, match='wavelength table is needed'):
      tr.deviceHits().histogram(bands=e, bins=10, wavelengths=(FIRST, np.zeros(0)))
    with pytest.raises(ValueError, match='bands'):
      tr.deviceHits().histogram(bands=[500.0, 400.0])
    # explicit rays know no spectrum: the seed route is refused by name
    with pytest.raises(_native.NativeError, match='no spectrum bound'):
      tr.deviceHits().histogram(bands=e, bins=10, wavelengths={'seed': SEED})
    # two seeds in one list; a spectral list with a monochromatic launch behind it
    tr.setSource(src)
    tr.reset()
    tr.trace(0, 2000, SEED, histogram=False)
    tr.trace(2000, 2000, SEED + 1, histogram=False)
    tr.sync()
    with pytest.raises(ValueError, match='two seeds.*wavelengths='):
      tr.deviceHits().histogram(bands=bc.LINE_EDGES)
    tr.reset()
    tr.trace(0, 2000, SEED, histogram=False)
    tr.setSpectrum(None)
    tr.trace(2000, 2000, SEED, histogram=False)
    tr.sync()
    with pytest.raises(ValueError, match='monochromatic and spectral'):
      tr.deviceHits().histogram(bands=bc.LINE_EDGES)
  finally:
    tr.close()


@pytest.mark.parametrize('k', [1, 7, 64])
def test_loaded_rows_need_their_wavelengths(native_lib, k):
  """rows put back with loadHits(HIT_DTYPE rows) carry their ray numbers but no provenance: ValueError without
  `wavelengths=`, the planes of the launch with it"""
  sc, lim, _ = sp.scene()
  o, d = sp.all_rays(N)
  e = bc.EDGE_SETS[k]
  wl = bc.wavelengths(e, N)
  tr = _tracer('off')
  try:
    tr.setScene(sc)
    tr.setLimits(lim)
    rows = _launch(tr, o, d, wl)
    planes = np.array([h.hist for h in tr.deviceHits().histogram(bands=e, bins=10).bands]).astype(np.uint64)
    assert planes.sum() > 300
    dh = tr.loadHits(rows)
    assert tr.hitProvenance() is None and len(dh) == len(rows)
    with pytest.raises(ValueError, match='wavelengths='):
      dh.histogram(bands=e, bins=10)
    got = dh.histogram(bands=e, bins=10, wavelengths=(FIRST, wl))
    counts, _ = _check(got, rows, wl[bc.ray_of(rows) - FIRST], e, False)
    assert np.array_equal(counts, planes)
  finally:
    tr.close()


# ---- 4. a run ---------------------------------------------------------------------------------------------------------
def test_a_run_is_binned_by_band_in_hbm(native_lib, tmp_path):
  """runSimulation('true') of a three-line source: `raw.loadHits('*').histogram(bands=)` bins the rows the run kept in HBM
  (provenance: the run's seed; the archive carries the source's spectrum) -- the planes of the host mirror on the arrays
  read back from the files (initWavelength); each line fills exactly its band"""
  from freecad.optics_design_workbench_amd.simulation import results_store, runSimulation
  doc, src = sp.document(source=dict(SOURCE, Spectrum=THREE_LINES), EndAfterRays='2e4', RaysPerIteration=1000.0,
                         StoreHitInitWavelength=True)
  for g in doc.Objects:
    if g.Name == 'Detectors_':
      g._props['RecordHits'] = True
  try:
    store = runSimulation(doc, 'true', seed=SEED, compileScene='off', raysPerLaunch=5000,
                          resultsPath=str(tmp_path / 'bench.OpticsDesign'))
    raw = results_store.RawFolder(store.runFolderPath())
    lazy = raw.loadHits('*')
    assert isinstance(lazy, results_store.RunHits)
    dev = lazy.deviceHits()
    assert dev is not None and len(dev) > 1000
    assert dev._tr.hitProvenance() == ('seed', SEED)
    got = lazy.histogram(bands=bc.LINE_EDGES, bins=10)
    assert lazy._loaded is None                                        # (nothing was read back)
    assert isinstance(got, BandHistograms) and len(got) == 3
    host = raw.loadHits('*', device=False)
    assert type(host) is results_store.Hits and len(host) == len(dev)
    want = host.histogram(bands=bc.LINE_EDGES, bins=10)
    _same_histogram(got.total, want.total, plane=False)            # counts, edges, origin
    assert got.noBand == want.noBand == 0
    lam = np.asarray(host.hits['initWavelength'])
    for b, line in enumerate(sp.LINES):
      _same_histogram(got[b], want[b], plane=False)
      assert int(got[b].hist.sum()) == int((lam == line).sum()) > 100
    # once the arrays were read, the same object answers from them
    lazy.hits
    again = lazy.histogram(bands=bc.LINE_EDGES, bins=10)
    for a, b in zip(again.bands, want.bands):
      _same_histogram(a, b, plane=False)
  finally:
    results_store.releaseDeviceRuns()
