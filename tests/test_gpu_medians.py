"""The medians the post-hoc histograms are centred on, and their fallbacks, against `numpy.median` of the projected
coordinates (tests/median_cases.py; the cases themselves are held by tests/test_median_cases.py):

  * the per-segment chain (`ph_select_stats`, csrc/odw_posthoc.hip) on synthetic clouds -- counts around the kernels'
    block and wave sizes, clouds piled up on one value, two values half and half, ranges that overflow or are
    subnormal, heavy tails, and 2^21 + 7 rows that take the sort (`ph_sorted_stats`);
  * the batched chain (csrc/odw_posthoc_batch.hip) on a spot swept through its focus, where thousands of rows tie on
    the median value: step by step the piled scene is sorted (`phb_read_project`), the enqueued chain reports it
    (PHB_SLOW_X / PHB_SLOW_Y) and `DeviceHitsBatch.measured()` hands it to the caller;
  * `parameterSweep` through the focus: `finishGroup` measures the reported scene segment by segment.

Origins are compared to the bit (the arithmetic is the same on both sides), counts count for count."""
import time

import numpy as np
import pytest

import median_cases as mc

pytestmark = pytest.mark.gpu

PLANE = dict(planeNormal=mc.PLANE_NORMAL, xInPlaneVec=mc.X_IN_PLANE)
# cartesian edges for the focus family: one edge on the median, the rest from below the focused spot's width (1e-13)
# to above the defocused ones' (1e-3)
_HALF = np.geomspace(1e-15, 1e-2, 18)
FOCUS_EDGES = np.r_[-_HALF[::-1], 0.0, _HALF]
CART = dict(binCoords='cartesian', bins=[FOCUS_EDGES, FOCUS_EDGES])


@pytest.fixture(scope='module')
def tracer(native_lib):
  from freecad.optics_design_workbench_amd.simulation.tracer import Tracer
  tr = Tracer(0)
  yield tr
  tr.close()


@pytest.fixture(scope='module', params=['off', 'structure'])
def batchTracer(native_lib, request):
  from freecad.optics_design_workbench_amd.simulation.tracer import Tracer
  tr = Tracer(0)
  tr.compileScene(request.param)
  tr.wanted = request.param
  yield tr
  tr.close()


# ---- a. the per-segment chain ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', mc.NAMES)
def test_per_segment_median_and_counts_equal_numpy(tracer, name):
  """(the cases run in the order of median_cases.NAMES on one tracer: a tiny cloud follows the 2^21 + 7 rows, and what
  a case leaves in the library's buffers must not show in the next)"""
  c = mc.case(name)
  hits = mc.rows(c.X, c.Y)
  x, y = mc.project(hits['points'], **PLANE)
  origin = mc.medians(x, y)
  edges = mc.edgesAbout(x, y)
  want = mc.histogram2d(x, y, origin, edges)
  t0 = time.perf_counter()
  dh = tracer.loadHits(hits)
  assert len(dh) == len(x)
  H = dh.histogram(bins=[edges, edges], **PLANE)
  t1 = time.perf_counter()
  print(f'{name}: m = {len(x)}, origin {H._origin}, load + select + median + bin {t1 - t0:.3f} s')
  assert np.array_equal(H._origin, origin), (name, H._origin, origin)          # (the sign of a zero: by value)
  assert np.array_equal(H.hist, want), (name, np.argwhere(H.hist != want)[:5])
  assert want.sum() == len(x)
  # a second selection of the same rows: the same answer
  H2 = tracer.deviceHits().histogram(bins=[edges, edges], **PLANE)
  assert np.array_equal(H2._origin, origin) and np.array_equal(H2.hist, want)


# ---- b. the batched chain on the focus family ----------------------------------------------------------------------------
def _traceFamily(tr, prs, n=mc.FOCUS_RAYS):
  """one batch launch of the scenes -> every segment's rows on the host"""
  cap = n + 1024
  tr.setLimits(prs[0].limits)
  tr.setSource(prs[0].source)
  tr.setSceneBatch([pr.scene for pr in prs])
  tr.setDetector(None)
  tr.reset()
  tr.traceBatch(0, n, mc.FOCUS_SEED, cap)
  tr.sync()
  assert tr.counters()['hits_dropped'] == 0
  assert tr.compiledInfo()['mode'] == (1 if tr.wanted == 'structure' else 0)
  rows = []
  for k in range(len(prs)):
    tr.batchSelect(k)
    rows.append(tr.hits())
  tr.batchSelect(None)
  return rows


def _projected(rows, ex, ey):
  return [(mc.dot3(r['point'], ex[k]), mc.dot3(r['point'], ey[k])) for k, r in enumerate(rows)]


def _ties(xy):
  return [(mc.tiesAtMiddle(x), mc.tiesAtMiddle(y)) for x, y in xy]


def _segmentAnswers(tr, k):
  """polar histogram and moments of DeviceHits on segment k alone"""
  from freecad.optics_design_workbench_amd.simulation import sweep
  tr.batchSelect(k)
  h = tr.deviceHits()
  return h.histogram(**sweep.calcFwhm.batchedBins), h.moments()


def _sameHistogram(got, want):
  return (np.array_equal(got.hist, want.hist) and np.array_equal(got._origin, want._origin) and
          np.array_equal(got._planeNormal, want._planeNormal) and np.array_equal(got._xInPlaneVec, want._xInPlaneVec))


@pytest.mark.parametrize('family', ['disc', 'halfDisc'])
def test_batched_medians_step_by_step_equal_numpy(batchTracer, family):
  """DeviceHitsBatch driven step by step: every scene is served -- the piled one through the sort of
  `phb_read_project`, `phb_origins_kernel` clears its flags before the bin"""
  from freecad.optics_design_workbench_amd.simulation import sweep
  from freecad.optics_design_workbench_amd.simulation.device_hits import DeviceHitsBatch
  tr = batchTracer
  prs = mc.focusProjects(halfDisc=family == 'halfDisc')
  rows = _traceFamily(tr, prs)
  S = len(prs)
  b = DeviceHitsBatch(tr, S)
  assert b.rows == [mc.FOCUS_RAYS] * S and all(b.ordered)
  boxes = b.histograms(**CART)
  polar = b.histograms(**sweep.calcFwhm.batchedBins)
  moments = b.moments()
  ex, ey, skip = b._axes()
  assert not skip.any()
  xy = _projected(rows, ex, ey)
  ties = _ties(xy)
  print(f'{family} ({tr.wanted}): rows tied on the middle rank per scene (X, Y): {ties}')
  for k in range(S):
    if family == 'disc' and k == 0:
      assert min(ties[k]) > mc.K_PHB_CAND, ties[k]          # the pile is real, on the device's own rows
    else:
      assert max(ties[k]) < mc.K_PHB_CAND, (k, ties[k])
  for k, (x, y) in enumerate(xy):
    origin = mc.medians(x, y)
    assert boxes[k] is not None and polar[k] is not None and moments[k] is not None, k
    assert np.array_equal(boxes[k]._origin, origin) and np.array_equal(polar[k]._origin, origin), (k, boxes[k]._origin, origin)
    want = mc.histogram2d(x, y, origin, FOCUS_EDGES)
    assert np.array_equal(boxes[k].hist, want), (k, np.argwhere(boxes[k].hist != want)[:5])
    assert want.sum() > 0.99 * len(x)
  for k in range(S):
    H, (mean, var) = _segmentAnswers(tr, k)
    assert _sameHistogram(polar[k], H), k
    assert np.array_equal(moments[k][0], mean) and np.array_equal(moments[k][1], var), k
  tr.batchSelect(None)


def _chain(tr, S, request):
  """the enqueued chain -> (batch, ex, ey) with the axes of every scene's plane (before `measured` drops any)"""
  from freecad.optics_design_workbench_amd.simulation.device_hits import DeviceHitsBatch
  b = DeviceHitsBatch.begin(tr, S)
  assert b.sampled(wait=True)
  b.searchPlanes()
  ex, ey, skip = b._axes()
  assert not skip.any() and all(b.ordered)
  b.enqueueMeasure(**request)
  assert b.measured(wait=True)
  return b, ex, ey


@pytest.mark.parametrize('binCoords', ['cartesian', 'polar'])
def test_enqueued_chain_reports_the_piled_scene_and_serves_the_others(batchTracer, binCoords):
  """begin / sampled / searchPlanes / enqueueMeasure / measured: the scene whose median candidates outnumber kPhbCand
  is flagged and handed to the caller (its plane dropped, None from histograms() and moments()), the others are
  numpy's -- and the same as in a batch without the piled scene"""
  from freecad.optics_design_workbench_amd.simulation import sweep
  tr = batchTracer
  request = CART if binCoords == 'cartesian' else sweep.calcFwhm.batchedBins
  prs = mc.focusProjects()
  S = len(prs)
  rows = _traceFamily(tr, prs)
  b, ex, ey = _chain(tr, S, request)
  xy = _projected(rows, ex, ey)
  ties = _ties(xy)
  assert min(ties[0]) > mc.K_PHB_CAND and max(max(t) for t in ties[1:]) < mc.K_PHB_CAND, ties
  counts, origins, flags = b._binned
  assert flags[0] != 0 and not flags[1:].any(), flags
  assert not b.detached()
  hists, moments = b.histograms(**request), b.moments()
  assert [h is None for h in hists] == [True] + [False] * (S - 1)
  assert [m is None for m in moments] == [True] + [False] * (S - 1)
  for k in range(1, S):
    x, y = xy[k]
    origin = mc.medians(x, y)
    assert np.array_equal(origins[k], origin) and np.array_equal(hists[k]._origin, origin), (k, origins[k], origin)
    if binCoords == 'cartesian':
      want = mc.histogram2d(x, y, origin, FOCUS_EDGES)
      assert np.array_equal(hists[k].hist, want), (k, np.argwhere(hists[k].hist != want)[:5])
  alone = [_segmentAnswers(tr, k) for k in range(1, S)]
  tr.batchSelect(None)
  for k in range(1, S):
    H, (mean, var) = alone[k - 1]
    if binCoords == 'polar':
      assert _sameHistogram(hists[k], H), k
    assert np.array_equal(moments[k][0], mean) and np.array_equal(moments[k][1], var), k
  # the same scenes without the piled one: nothing of it shows in their answers, and no flag is carried over.  (The
  # per-segment histograms above went through the device's edge buffers with the polar edges: a chain that bins other
  # edges behind them must upload its own again -- it once kept "its" edges cached and binned by the stale ones.)
  _traceFamily(tr, prs[1:])
  b2, _, _ = _chain(tr, S - 1, request)
  assert not b2._binned[2].any() and b2.detached()
  assert np.array_equal(b2._binned[1], origins[1:]) and np.array_equal(b2._binned[0], counts[1:])
  for k, (h2, m2) in enumerate(zip(b2.histograms(**request), b2.moments()), start=1):
    assert _sameHistogram(h2, hists[k]), k
    assert np.array_equal(m2[0], moments[k][0]) and np.array_equal(m2[1], moments[k][1]), k


@pytest.mark.parametrize('n', [1, 2, 3, 64, 65])
def test_batched_medians_of_tiny_segments_equal_numpy(batchTracer, n):
  """m in {1, 2, 3, 64, 65}: one block projects, `phb_rank_bins` scans a near-empty histogram, k_lo = k_hi = 0 at m = 1"""
  from freecad.optics_design_workbench_amd.simulation.device_hits import DeviceHitsBatch
  tr = batchTracer
  prs = mc.focusProjects(dzs=(1e-3, -1e-3, 1e-9))
  rows = _traceFamily(tr, prs, n)
  assert [len(r) for r in rows] == [n] * 3
  b = DeviceHitsBatch(tr, 3)
  boxes = b.histograms(**CART)
  ex, ey, _ = b._axes()
  xy = _projected(rows, ex, ey)
  for k, (x, y) in enumerate(xy):
    origin = mc.medians(x, y)
    assert np.array_equal(boxes[k]._origin, origin), (n, k, boxes[k]._origin, origin)
    assert np.array_equal(boxes[k].hist, mc.histogram2d(x, y, origin, FOCUS_EDGES)), (n, k)
  c, ex2, ey2 = _chain(tr, 3, CART)
  assert np.array_equal(ex2, ex) and np.array_equal(ey2, ey)
  assert not c._binned[2].any() and c.detached()
  for k, (x, y) in enumerate(xy):
    assert np.array_equal(c._binned[1][k], mc.medians(x, y)), (n, k)
    assert np.array_equal(c.histograms(**CART)[k].hist, boxes[k].hist), (n, k)


# ---- c. the sweep's hand-over ----------------------------------------------------------------------------------------------
def test_sweep_through_the_focus_measures_the_reported_scene_by_itself(native_lib, tracer):
  """parameterSweep with batch launches against one launch per value, through the exact focus: `finishGroup` meets a
  scene the chain reported and measures it segment by segment -- nothing dropped, nothing binned about a stale origin"""
  from freecad.optics_design_workbench_amd import scenes
  from freecad.optics_design_workbench_amd.simulation import sweep
  from freecad.optics_design_workbench_amd.simulation.tracer import Tracer
  doc = mc.focusDocument()
  # 22 values on four contexts go out in groups of 2, 4, 4, 3, 3, 3, 3: the focus in the middle of a group of four
  # (index 3) and of a group of three (index 11)
  dz = np.r_[np.linspace(-1e-3, -1e-4, 11), np.linspace(1e-4, 1e-3, 11)]
  dz[3] = dz[11] = 0.0

  def inner(hits):
    """rows within 5e-5 of the median, through a per-segment cartesian histogram: other edges than the chain's polar
    ones pass through the device between two groups of one context"""
    return float(hits.histogram(**CART).hist[3:-3, 3:-3].sum())

  def window(hits):
    return inner(hits)
  # the same figure with a batched form: a histogram the chain did not bin, asked of the batch after `measured` -- the
  # reported scene must come back None (and go segment by segment), not binned about the origin the chain never found
  window.batched = lambda batch: [None if H is None else float(H.hist[3:-3, 3:-3].sum()) for H in batch.histograms(**CART)]
  res = {}
  for batch in (0, 4):
    with Tracer(0) as tr:
      res[batch] = sweep.parameterSweep(doc, mc.setDz, dz, rays=mc.FOCUS_RAYS, seed=mc.FOCUS_SEED, tracer=tr, batch=batch,
                                        measure=dict(fwhm=sweep.calcFwhm, rms=sweep.rmsSpot, rows=len, inner=inner,
                                                     window=window))
  print('rms through the focus:', res[4].columns['rms'][[2, 3, 4, 10, 11, 12]])
  for col in ('fwhm', 'rms', 'rows', 'inner', 'window'):
    assert np.array_equal(res[4].columns[col], res[0].columns[col], equal_nan=col == 'fwhm'), (col, res[4].columns[col], res[0].columns[col])
  for batch in (0, 4):
    assert np.array_equal(res[batch].columns['rows'], np.full(len(dz), mc.FOCUS_RAYS))
    rms = res[batch].columns['rms']
    assert np.isfinite(rms).all()
    assert np.all(rms[dz == 0] < 1e-12), rms[dz == 0]
    assert np.all(rms[dz != 0] > 1e-6)
    inside = res[batch].columns['inner']
    assert np.all(inside[dz == 0] == mc.FOCUS_RAYS) and 0 < inside[0] < mc.FOCUS_RAYS and 0 < inside[-1] < mc.FOCUS_RAYS
    assert np.array_equal(res[batch].columns['window'], inside)
    assert res[batch].tracedRays == len(dz) * mc.FOCUS_RAYS
  # a defocused value's rms is that of a launch of its own
  for k in (2, 4, 12):
    mc.setDz(doc, dz[k])
    pr = scenes.bakeProject(doc)
    tracer.setScene(pr.scene)
    tracer.setSource(pr.source)
    tracer.setLimits(pr.limits)
    tracer.setDetector(None)
    tracer.reserveHits(mc.FOCUS_RAYS + 1024)
    tracer.reset()
    tracer.trace(0, mc.FOCUS_RAYS, mc.FOCUS_SEED, histogram=False)
    tracer.sync()
    assert sweep.rmsSpot(tracer.deviceHits()) == res[4].columns['rms'][k], k
