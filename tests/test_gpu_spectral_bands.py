"""Spectral detector maps on the device: per-band count and power planes of spectral launches.

A detector with band edges keeps, behind its count plane and its power plane, one more of each per band; a binned hit of a
spectral launch is counted (and weighed) in the band its ray's wavelength falls into by numpy.histogram's rule.  Expected
planes come from numpy alone: spectral_band_cases.band_planes over hit rows -- the oracle's rows per line where every line
falls into one band, else the launch's own rows with the wavelength of a row taken from its ray number -- binned by
power_scene.detector_bins and weighed by power_scene.quanta.  Every comparison is an integer equality.

`compile='off'`: the binary tree's BANDS kernels; `'structure'`: the compiled kernel's BANDS variant
(`compiledInfo()['bands']` says which)."""
import numpy as np
import pytest

import power_scene
import spectral_band_cases as bc
import spectral_cases as sp
from freecad.optics_design_workbench_amd import _native
from test_gpu_spectral import SEED, SOURCE, THREE_LINES, bench  # noqa: F401  (the bench launch: a fixture)

pytestmark = pytest.mark.gpu
DET = power_scene.DETECTOR
NB = DET['nx'] * DET['ny']


def _tracer(compile='off'):
  from freecad.optics_design_workbench_amd.simulation.tracer import Tracer
  tr = Tracer(0)
  tr.compileScene(compile)
  return tr


def _explicit(tr, sc, lim, o, d, wl, edges, power=True, first=0, setup=True):
  """one traceRays launch with a wavelength per ray -> (counters, rows, total counts, total power or None, band counts or
  None, band power or None)"""
  if setup:
    tr.setScene(sc)
    tr.setLimits(lim)
  tr.setDetector(DET, power=power, bands=edges)
  tr.reserveHits(max(len(o), 64) * 8)
  tr.reset()
  tr.traceRays(o, d, first=first, wavelengths=wl)
  tr.sync()
  return (tr.counters(), tr.hits(), tr.histogram(), tr.powerHistogramRaw() if power else None,
          tr.bandHistogram() if edges is not None else None, tr.bandPowerHistogramRaw() if edges is not None and power else None)


# ---- 1. explicit wavelengths, lines -----------------------------------------------------------------------------------
_LINE_PLANES = {}


@pytest.mark.parametrize('compile', ['off', 'structure'])
def test_lines_against_the_oracle(bench, compile):
  """the bench launch of test_gpu_spectral.py (5000 rays, F / d / C round-robin) with edges [450, 540, 620, 700]: band b holds
  numpy's planes of the oracle's rows of line b on the constant-index scene"""
  sc, lim, o, d, wl, per_line = bench
  e = bc.LINE_EDGES
  assert np.array_equal(bc.band_of(e, sp.LINES), [0, 1, 2])
  tr = _tracer(compile)
  try:
    cnt, rows, hist, raw, bands, bpow = _explicit(tr, sc, lim, o, d, wl, e)
    info = tr.compiledInfo()
    plain = _explicit(tr, sc, lim, o, d, wl, None, setup=False)
  finally:
    tr.close()
  assert info['mode'] == info['bands'] == (1 if compile == 'structure' else 0), info
  assert bands.shape == bpow.shape == (3, DET['nx'], DET['ny']) and bands.dtype == bpow.dtype == np.uint64
  for b, line in enumerate(sp.LINES):
    c, p, _ = power_scene.planes(per_line[line][1]['hits'], DET)
    assert c.sum() > 100
    assert np.array_equal(bands[b], c), line
    assert np.array_equal(bpow[b], p), line
  assert np.array_equal(bands.sum(0), hist) and np.array_equal(bpow.sum(0), raw)
  # the total planes, the rows and the counters are those of the same launch without bands
  assert plain[0] == cnt and np.array_equal(plain[2], hist) and np.array_equal(plain[3], raw) and hist.any()
  for col in ('point', 'direction', 'power', 'tag'):
    assert np.array_equal(rows[col], plain[1][col]), col
  for other in _LINE_PLANES.values():                  # both compile modes: the same planes bit for bit
    assert np.array_equal(bands, other[0]) and np.array_equal(bpow, other[1])
  _LINE_PLANES[compile] = (bands, bpow)


# ---- 2. explicit wavelengths, continuum and edges ---------------------------------------------------------------------
@pytest.mark.parametrize('compile', ['off', 'structure'])
@pytest.mark.parametrize('k', [1, 7, 64])
def test_continuum_and_edges_against_own_rows(native_lib, compile, k):
  """1025 rays whose wavelengths sit on every edge, one ulp on either side of it, below e_0, above e_K, on e_K, and between
  the edges: the band planes are numpy's planes of the launch's own rows (the wavelength of a row from its ray number);
  what the total plane holds beyond the bands' sum are the binned hits whose wavelength lies in no band; launches of the
  first 1, 63, 64 and 65 rays give the planes of those rays"""
  sc, lim, _ = sp.scene()
  n = 1025
  o, d = sp.all_rays(n)
  e = bc.EDGE_SETS[k]
  wl = bc.wavelengths(e, n)
  assert set(e) <= set(wl) and (bc.band_of(e, wl) < 0).sum() >= 6
  tr = _tracer(compile)
  try:
    cnt, rows, hist, raw, bands, bpow = _explicit(tr, sc, lim, o, d, wl, e)
    assert tr.compiledInfo()['bands'] == (1 if compile == 'structure' else 0)
    assert cnt['hits_dropped'] == 0 and cnt['traced_rays'] == n
    w_rows = wl[bc.ray_of(rows)]
    want_c, want_p, outside = bc.band_planes(rows, w_rows, e, DET)
    tot_c, tot_p, _ = power_scene.planes(rows, DET)
    assert np.array_equal(hist, tot_c) and np.array_equal(raw, tot_p)
    assert np.array_equal(bands, want_c) and np.array_equal(bpow, want_p)
    assert bands.sum() > 300 and len(np.unique(bpow)) > 20
    assert outside > 0 and int(hist.sum()) - int(bands.sum()) == outside
    assert np.array_equal(hist - bands.sum(0), tot_c - want_c.sum(0))
    for m in (1, 63, 64, 65):
      _, part, h2, r2, b2, p2 = _explicit(tr, sc, lim, o[:m], d[:m], wl[:m], e, setup=False)
      first = rows[bc.ray_of(rows) < m]
      c, p, _ = bc.band_planes(first, wl[bc.ray_of(first)], e, DET)
      assert len(part) == len(first) > 0
      assert np.array_equal(b2, c) and np.array_equal(p2, p), m
      assert np.array_equal(h2, power_scene.planes(first, DET)[0]), m
  finally:
    tr.close()


# ---- 3. generated rays --------------------------------------------------------------------------------------------------
GEN_EDGES = np.array([470.0, 500.25, 560.0, 610.5, 680.0])
DENSITY = dict(SpectralDensity='exp(-(wavelength-550)^2/(2*40^2)) + 0.2', SpectrumDomain='450, 700', SpectrumResolution='1e3')


def _device_words(view):
  import ctypes as C
  hip = C.CDLL('libamdhip64.so')
  hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
  cai = view.__cuda_array_interface__
  out = np.zeros(cai['shape'][0], dtype=np.int64)
  assert hip.hipMemcpy(out.ctypes.data, cai['data'][0], out.nbytes, 2) == 0          # (2: hipMemcpyDeviceToHost)
  return out


@pytest.mark.parametrize('compile', ['off', 'structure'])
@pytest.mark.parametrize('spectrum', ['density', 'lines'])
def test_generated_rays(native_lib, compile, spectrum):
  """a point source under a SpectralDensity / under Spectrum lines, 20000 rays: the planes against numpy on the launch's own
  rows with Tracer.rayWavelengths; the halves add up to the whole bit for bit; the results block is
  [16 | counts | power | K band counts | K band power]"""
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

    def launch(a, m, power=True):
      tr.setDetector(DET, power=power, bands=e)
      tr.reserveHits(n * 8)
      tr.reset()
      tr.trace(a, m, SEED)
      tr.sync()
      return tr.histogram(), tr.powerHistogramRaw() if power else None, tr.bandHistogram(), tr.bandPowerHistogramRaw() if power else None

    hist, raw, bands, bpow = launch(first, n)
    rows, cnt = tr.hits(), tr.counters()
    assert tr.compiledInfo()['bands'] == (1 if compile == 'structure' else 0)
    wl = tr.rayWavelengths(first + np.arange(n, dtype=np.uint64), SEED)
    want_c, want_p, outside = bc.band_planes(rows, wl[bc.ray_of(rows) - first], e, DET)
    assert cnt['hits_dropped'] == 0 and want_c.sum() > 1000
    assert np.array_equal(bands, want_c) and np.array_equal(bpow, want_p)
    assert np.array_equal(hist, power_scene.planes(rows, DET)[0])
    assert int(hist.sum()) - int(bands.sum()) == outside and (outside > 0) == (spectrum == 'density')
    assert all(bands[b].any() for b in range(k))
    # the block: [16 counter words | counts | power | K band counts | K band power], band-major
    view, off = tr.resultsView()
    block = _device_words(view)
    assert off == 16 and block.shape == (16 + NB * 2 * (1 + k),)
    u = block[off:].astype(np.uint64)
    assert np.array_equal(u[:NB].reshape(hist.shape), hist) and np.array_equal(u[NB:2 * NB].reshape(hist.shape), raw)
    assert np.array_equal(u[2 * NB:(2 + k) * NB].reshape(bands.shape), bands)
    assert np.array_equal(u[(2 + k) * NB:].reshape(bands.shape), bpow)
    bview = tr.bandHistogramView().__cuda_array_interface__
    assert bview['shape'] == (2 * k * NB,) and bview['data'][0] == view.__cuda_array_interface__['data'][0] + 8 * (off + 2 * NB)
    # two launches of the halves add up to the single launch
    parts = [launch(first, n // 2), launch(first + n // 2, n - n // 2)]
    for whole, a, b in zip((hist, raw, bands, bpow), *parts):
      assert np.array_equal(a + b, whole)
    # without the power plane: [16 | counts | K band counts]
    h1, _, b1, _ = launch(first, n, power=False)
    view, off = tr.resultsView()
    block = _device_words(view)
    assert block.shape == (16 + NB * (1 + k),)
    assert np.array_equal(h1, hist) and np.array_equal(b1, bands)
    assert np.array_equal(block[off + NB:].astype(np.uint64).reshape(bands.shape), bands)
    with pytest.raises(ValueError, match='no power plane'):
      tr.bandPowerHistogramRaw()
    tr.setDetector(DET, power=True, bands=e)
    real = tr.bandPowerHistogram()
    assert real.dtype == np.float64 and real.shape == bands.shape and not real.any()       # (setting bands zeroes their planes)
  finally:
    tr.close()


# ---- 4. Fresnel and coating routes ------------------------------------------------------------------------------------
@pytest.mark.parametrize('route', ['fresnel', 'coat'])
def test_fresnel_and_coating_routes(bench, route):
  """the bench with Fresnel 'Loss' on the singlet -- and a one-layer coating on it -- : the tree's fresnel / coat CHROMA
  kernels with BANDS.  Band power planes against numpy on the launch's own rows; band counts those of the launch without
  Fresnel ('Loss' takes power away, it moves no ray)"""
  sc, lim, o, d, wl, per_line = bench
  e = bc.LINE_EDGES
  tr = _tracer('structure')              # (spectral + Fresnel: the tree, whatever the mode)
  try:
    base = _explicit(tr, sc, lim, o, d, wl, e)
    tr.setFresnel(['Loss', '', '', ''])
    if route == 'coat':
      tr.setCoating([[(1.38, 99.6)], [], [], []])
    cnt, rows, hist, raw, bands, bpow = _explicit(tr, sc, lim, o, d, wl, e, setup=False)
    info = tr.compiledInfo()
  finally:
    tr.close()
  assert info['fresnel'] == 0, info
  want_c, want_p, outside = bc.band_planes(rows, wl[bc.ray_of(rows)], e, DET)
  assert outside == 0 and np.array_equal(bands, want_c) and np.array_equal(bpow, want_p)
  assert np.array_equal(bands, base[4]) and np.array_equal(hist, base[2]) and bands.any()
  assert np.array_equal(bpow.sum(0), raw)
  # the loss is in the planes: less power than without Fresnel wherever the singlet's rays land, never more
  assert np.all(bpow <= base[5]) and int(bpow.sum()) < int(base[5].sum())
  if route == 'coat':
    _COATED['coat'] = bpow
  else:
    _COATED['bare'] = bpow
  if len(_COATED) == 2:                  # a quarter-wave MgF2 layer reflects less than the bare glass
    assert int(_COATED['coat'].sum()) > int(_COATED['bare'].sum())


_COATED = {}


# ---- 5. the band index on the device ----------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [1, 3, 5, 7, 64])
def test_band_index_on_the_device(native_lib, k):
  e = bc.EDGE_SETS[k] if k in bc.EDGE_SETS else np.array([380.0, 380.5, 455.25, 600.0, 601.0, 790.125])
  wl = np.r_[bc.probes(e, 3000), np.nan, np.inf, -np.inf, 0.0, -500.0]
  host = _native.band_index(e, wl)
  assert np.array_equal(host, bc.band_of(e, wl))
  assert np.array_equal(_native.band_index(e, wl, device=True), host)


# ---- 6. refusals --------------------------------------------------------------------------------------------------------
def test_refusals(bench):
  sc, lim, o, d, wl, per_line = bench
  o, d, wl = o[:200], d[:200], wl[:200]
  e = bc.LINE_EDGES
  tr = _tracer()
  try:
    tr.setScene(sc)
    tr.setLimits(lim)
    with pytest.raises(_native.NativeError, match='odw_set_detector_bands: bands need a detector'):
      tr.setDetector(None, bands=e)
    for bad, what in (([450.0, np.nan], 'band edge 1 .* is not finite'), ([-5.0, 500.0], 'band edge 0 .* is not positive'),
                      ([450.0, 450.0], 'band edge 1 .* is not above its predecessor'),
                      (bc.edges(65), '65 bands: a detector takes at most ODW_BAND_MAX = 64')):
      with pytest.raises(_native.NativeError, match='odw_set_detector_bands: ' + what):
        tr.setDetector(DET, bands=bad)
    tr.setDetector(DET, power=True, bands=e)
    tr.reserveHits(len(o) * 8)
    tr.reserveSegments(len(o) * 8)
    tr.reset()
    with pytest.raises(_native.NativeError, match='band planes: the launch is monochromatic'):
      tr.traceRays(o, d)
    with pytest.raises(_native.NativeError, match='band planes: a launch with ODW_TRACE_RECORD_SEGMENTS'):
      tr.traceRays(o, d, wavelengths=wl, record_segments=True)
    # launches that ask for no histogram are none of the bands' business
    tr.traceRays(o, d, histogram=False)
    tr.traceRays(o, d, wavelengths=wl, record_segments=True, histogram=False)
    tr.sync()
    assert not tr.bandHistogram().any()
    # ... and the context goes on
    tr.reset()
    tr.traceRays(o, d, wavelengths=wl)
    tr.sync()
    assert tr.bandHistogram().any() and np.array_equal(tr.bandHistogram().sum(0), tr.histogram())
    # setDetector without bands has none
    tr.setDetector(DET)
    with pytest.raises(ValueError, match='no bands'):
      tr.bandHistogram()
    with pytest.raises(ValueError, match='no bands'):
      tr.bandHistogramView()
    view, off = tr.resultsView()
    assert view.__cuda_array_interface__['shape'] == (off + NB,)
    tr.reset()
    tr.traceRays(o, d)                   # (monochromatic again, as ever)
    tr.sync()
    assert tr.histogram().any()
  finally:
    tr.close()


def test_refusal_of_a_batch(native_lib):
  """bands and batches: refused by name, and the batch runs once the bands are gone"""
  import os
  from conftest import SCENES
  from freecad.optics_design_workbench_amd import scenes
  from freecad.optics_design_workbench_amd.scene import open_fcstd
  doc = open_fcstd(os.path.join(SCENES, 'GettingStarted.FCStd'))
  batch = []
  for radius in (9.6, 10.0):
    doc.Sphere.Radius = radius
    batch.append(scenes.bakeProject(doc))
  m = 2000
  tr = _tracer()
  try:
    tr.setLimits(batch[0].limits)
    tr.setSource(batch[0].source)
    tr.setSceneBatch([b.scene for b in batch])
    tr.setDetector(DET, bands=bc.LINE_EDGES)
    tr.reset()
    with pytest.raises(_native.NativeError, match='odw_trace_batch: a batch with detector bands set'):
      tr.traceBatch(0, m, SEED, 2 * m)
    tr.setDetector(DET)
    tr.traceBatch(0, m, SEED, 2 * m)
    tr.sync()
    assert tr.counters()['traced_rays'] == 2 * m
  finally:
    tr.close()


# ---- 7. off means off -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('compile', ['off', 'structure'])
def test_off_means_off(bench, compile):
  """bands never set: a spectral launch with the power plane leaves the device words behind that plane as they are.  The
  block is made longer than the detector needs by a larger detector set first (it never shrinks); the words behind the
  power plane are given a pattern through the HIP runtime, and read back after the launch"""
  import ctypes as C
  sc, lim, o, d, wl, per_line = bench
  hip = C.CDLL('libamdhip64.so')
  hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
  tr = _tracer(compile)
  try:
    tr.setScene(sc)
    tr.setLimits(lim)
    tr.setDetector(dict(DET, nx=4 * DET['nx'], ny=2 * DET['ny']))               # 8 NB bins: the block holds 16 + 8 NB words
    tr.setDetector(DET, power=True)
    view, off = tr.resultsView()
    cai = view.__cuda_array_interface__
    assert cai['shape'] == (off + 2 * NB,)
    behind = cai['data'][0] + 8 * (off + 2 * NB)
    pattern = (np.arange(6 * NB, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) | np.uint64(1)
    assert hip.hipMemcpy(behind, pattern.ctypes.data, pattern.nbytes, 1) == 0     # (1: hipMemcpyHostToDevice)
    tr.reserveHits(len(o) * 8)
    tr.reset()
    tr.traceRays(o, d, wavelengths=wl)
    tr.sync()
    assert tr.compiledInfo()['bands'] == 0 and tr.compiledInfo()['chroma'] == (1 if compile == 'structure' else 0)
    view2, _ = tr.resultsView()
    assert view2.__cuda_array_interface__['data'][0] == cai['data'][0]            # (the block has not moved)
    after = np.zeros_like(pattern)
    assert hip.hipMemcpy(after.ctypes.data, behind, after.nbytes, 2) == 0
    assert np.array_equal(after, pattern)
    assert tr.histogram().any() and tr.powerHistogramRaw().any()
    with pytest.raises(ValueError, match='no bands'):
      tr.bandHistogram()
  finally:
    tr.close()
