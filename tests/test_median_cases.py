"""The clouds of tests/median_cases.py are what they claim to be -- held with numpy alone (synthetic clouds) and on
the CPU oracle's rows (the focus family), so that tests/test_gpu_medians.py cannot pass because a case silently stopped
being the case."""
import numpy as np
import pytest

import median_cases as mc


@pytest.mark.parametrize('name', mc.NAMES)
def test_synthetic_cases_are_what_they_claim(name):
  c = mc.case(name)
  assert len(c.X) == len(c.Y)
  for v, claims in ((c.X, c.claimsX), (c.Y, c.claimsY)):
    assert not np.isnan(v).any()
    assert len(v) == claims['m']
    ties = mc.tiesAtMiddle(v)
    if 'ties' in claims:
      assert ties == claims['ties'], (name, ties)
    if 'ties_above' in claims:
      assert ties > claims['ties_above'], (name, ties)
    if 'ties_below' in claims:
      assert ties < claims['ties_below'], (name, ties)
    lo, hi = mc.middle(v)
    if 'middle' in claims:
      assert (lo, hi) == claims['middle'], (name, lo, hi)
      if claims['middle'][0] != claims['middle'][1]:
        assert lo != hi and len(v) % 2 == 0
        if 'width' not in claims:       # two values, half and half: the middle ranks are the extrema (coarse bins 0 and 4095)
          assert lo == v.min() and hi == v.max()
    with np.errstate(over='ignore'):
      width = v.max() - v.min()
    want = claims.get('width')
    if want == 'subnormal':
      assert 0 < width < np.finfo(np.float64).tiny
      with np.errstate(over='ignore', under='ignore'):
        assert np.isinf(4096.0 / width) and width / 4096.0 == 0.0
    elif want is not None:
      assert width == want, (name, width)          # (0, inf, or 2e300: everything but the outliers in one bin)
    else:
      assert np.isfinite(width)
    if claims.get('signed_zeros'):
      zeros = v[v == 0]
      assert np.signbit(zeros).any() and not np.signbit(zeros).all() and lo == 0 and hi == 0


def test_the_cases_cover_what_the_kernels_branch_on():
  ms = [mc.case(n).claimsX['m'] for n in mc.NAMES]
  assert set(mc.COUNTS) <= set(ms)
  big = mc.case('sort-route+normal-big')
  assert len(big.X) == mc.BIG > mc.K_PH_SEL_MAX and mc.tiesAtMiddle(big.X) == mc.K_PH_SEL_MAX + 5
  assert big.X.min() < 0.75 < big.X.max()
  # a tiny case follows the large one
  at = mc.NAMES.index('sort-route+normal-big')
  assert mc.case(mc.NAMES[at + 1]).claimsX['m'] == 1
  # every edge array has an edge on the median and finite ends that bracket the cloud
  for c in mc.cases():
    x, y = mc.project(mc.rows(c.X, c.Y)['points'], mc.PLANE_NORMAL, mc.X_IN_PLANE)
    assert np.array_equal(x, c.X) and np.array_equal(y, c.Y)          # (by value: -0.0 projects to +0.0)
    e = mc.edgesAbout(x, y)
    o = mc.medians(x, y)
    assert np.isfinite(e).all() and 0.0 in e and np.all(np.diff(e) > 0)
    assert mc.histogram2d(x, y, o, e).sum() == len(x), c.name


def _oracleRows(oracle, pr):
  from oracle_tracer import OracleTracer
  with OracleTracer() as tr:
    tr.setScene(pr.scene)
    tr.setSource(pr.source)
    tr.setLimits(pr.limits)
    tr.setDetector(None)
    tr.trace(0, mc.FOCUS_RAYS, mc.FOCUS_SEED, histogram=False)
    return tr.hits()


def _tiesOnHostPlane(rows):
  from freecad.optics_design_workbench_amd.jupyter_utils.hits import Hits
  h = Hits(dict(points=np.ascontiguousarray(rows['point']), directions=np.ascontiguousarray(rows['direction']),
                isEntering=(rows['tag'] >> np.uint64(63)).astype(np.int64)))
  normal, xvec = h.detectPlaneNormal()
  x, y = mc.project(h.points(), normal, xvec)
  return mc.tiesAtMiddle(x), mc.tiesAtMiddle(y), float(max(np.ptp(x), np.ptp(y)))


def test_focus_family_piles_up_at_the_focus_only(oracle):
  """200 000 rays, seed 5, on the CPU oracle: at dz = 0 the rows tied on the value at rank (m - 1) // 2 number more
  than kPhbCand = 2048 on both coordinates (measured: 10 643 and 10 690, the cloud 2.6e-13 wide); at every other dz,
  and for the half disc, fewer"""
  prs = mc.focusProjects()
  for dz, pr in zip(mc.FOCUS_DZ, prs):
    rows = _oracleRows(oracle, pr)
    assert len(rows) == mc.FOCUS_RAYS
    tx, ty, width = _tiesOnHostPlane(rows)
    print(f'focus family dz={dz:g}: ties at the middle rank X {tx} Y {ty}, width {width:.3g}')
    if dz == 0.0:
      assert tx > mc.K_PHB_CAND and ty > mc.K_PHB_CAND, (tx, ty)
    else:
      assert tx < mc.K_PHB_CAND and ty < mc.K_PHB_CAND, (dz, tx, ty)
  for dz, pr in zip(mc.HALF_DISC_DZ, mc.focusProjects(halfDisc=True)):
    rows = _oracleRows(oracle, pr)
    assert len(rows) == mc.FOCUS_RAYS
    tx, ty, width = _tiesOnHostPlane(rows)
    print(f'half disc dz={dz:g}: ties at the middle rank X {tx} Y {ty}, width {width:.3g}')
    assert tx < mc.K_PHB_CAND and ty < mc.K_PHB_CAND, (dz, tx, ty)
    # the median is not the centre: the centre of the full disc is the focus' (x, y) = (0, 0)
    p = rows['point']
    if abs(dz) >= 1e-3:
      r = np.hypot(p[:, 0], p[:, 1]).max()
      assert np.hypot(np.median(p[:, 0]), np.median(p[:, 1])) > 0.2 * r
