"""Part::Ellipsoid on the device, held to closed forms evaluated here in float64 (tests/ellipsoid_cases.py; the CPU
oracle does not know the kind): crossings, trimming against a box from both sides, the two focal properties -- mirror
from focus to focus, the aberration-free immersion lens --, a sphere written as an ellipsoid against the oracle's
sphere, and every route: the compiled kernel, the grid kernel's item branch, the binary tree, batch launches.  Every
recorded point within 1e-9 mm, powers within 1e-12, counts exact; the generic and the compiled launch of a scene agree
row for row, bit for bit."""
import numpy as np
import pytest

import ellipsoid_cases as ec
import power_scene
from freecad.optics_design_workbench_amd.freecad_elements import make

pytestmark = pytest.mark.gpu

SEED = 0x0D15EA5E
MODES = ['off', 'structure']


def _launch(sc, lim, o, d, mode='off', segments=False, det=None, power=False):
  """explicit rays through a tracer of its own -> dict(rows, counters, info, [segments, hist, power plane])"""
  from freecad.optics_design_workbench_amd.simulation.tracer import Tracer
  with Tracer(0) as tr:
    tr.compileScene(mode)
    tr.setScene(sc)
    tr.setLimits(lim)
    tr.setDetector(det, power=power)
    tr.reserveHits(len(o) * (lim.max_intersections + 1))
    if segments:
      tr.reserveSegments(len(o) * (lim.max_intersections + 1))
    tr.reset()
    tr.traceRays(o, d, record_segments=segments, histogram=det is not None)
    tr.sync()
    out = dict(rows=tr.hits(), counters=tr.counters(), info=tr.compiledInfo())
    assert out['counters']['hits_dropped'] == 0
    if segments:
      out['segments'] = tr.segments()
    if det is not None:
      out['hist'] = tr.histogram()
      out['power'] = tr.powerHistogramRaw() if power else None
  return out


def _same_rows(a, b):
  assert a['counters'] == b['counters']
  for col in ('tag', 'point', 'direction', 'power'):
    assert np.array_equal(a['rows'][col], b['rows'][col]), col


def _both(sc, lim, o, d):
  """the generic and the compiled launch: equal bit for bit -> the rows"""
  off, spec = (_launch(sc, lim, o, d, mode) for mode in MODES)
  assert off['info']['mode'] == 0 and spec['info']['mode'] == 1, (off['info'], spec['info'])
  _same_rows(off, spec)
  return off['rows']


def _held(got, want, excluded=None, cap=0.01):
  """every line that is not excluded: the expected number of points, each within TOL"""
  excluded = np.zeros(len(want), bool) if excluded is None else excluded
  assert excluded.mean() <= cap
  worst = 0.0
  for k, (g, w) in enumerate(zip(got, want)):
    if excluded[k]:
      continue
    assert len(g) == len(w), (k, g, w)
    if len(w):
      worst = max(worst, float(np.abs(g - w).max()))
  print(f'worst deviation {worst:.3e} mm over {len(want) - int(excluded.sum())} lines')
  assert worst < ec.TOL


# ---- 1 ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def scene1():
  pl = ec.PLACEMENTS[1]
  O, D, want = ec.crossing_lines()
  sc, lim = ec.vacuum(lambda d: [ec.ellipsoid(d, 'E', ec.RADII, **pl)])
  return sc, lim, ec.to_world(pl, points=O), ec.to_world(pl, dirs=D), [ec.to_world(pl, points=w) for w in want]


@pytest.mark.parametrize('pl', ec.PLACEMENTS, ids=['at-origin', 'moved'])
def test_crossings_triaxial(native_lib, pl):
  """ellipsoid (30, 20, 50): lines along the axes, chords parallel to them, lines through the centre, a line that
  clears the surface by 1e-9 mm (nothing) beside one 1e-6 mm inside (its chord), rays that start inside (one point)"""
  O, D, want = ec.crossing_lines()
  assert len(O) == 36 and sum(len(w) == 0 for w in want) == 1 and sum(len(w) == 1 for w in want) == 8
  sc, lim = ec.vacuum(lambda d: [ec.ellipsoid(d, 'E', ec.RADII, **pl)])
  o, d = ec.to_world(pl, points=O), ec.to_world(pl, dirs=D)
  rows = _both(sc, lim, o, d)
  assert len(rows) == sum(len(w) for w in want)
  _held(ec.per_ray(rows, o, d), [ec.to_world(pl, points=w) for w in want])


# ---- 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['common', 'cut'])
def test_trimmed_by_a_box(native_lib, case):
  """Common(ellipsoid, box z <= 10): the ellipsoid's face inside the box, the box's inside the ellipsoid;
  Cut(box 120^3, ellipsoid): the "outside the ellipsoid" literal on the box, the flipped face of the cavity"""
  o, d = ec.random_lines(2000)
  sc, lim = ec.common_scene() if case == 'common' else ec.cut_scene()
  want, excluded = ec.common_expected(o, d) if case == 'common' else ec.cut_expected(o, d)
  if case == 'common':
    assert sum(len(w) > 0 for w in want) == 476 and excluded.sum() == 0
  else:
    assert sum(len(w) == 4 for w in want) == 630 and all(len(w) in (2, 4) for w in want)
  _held(ec.per_ray(_both(sc, lim, o, d), o, d), want, excluded)


# ---- 3 ---------------------------------------------------------------------------------------------------------------
def test_mirror_from_focus_to_focus(native_lib):
  """an ellipsoidal cavity rx = ry = 30, rz = 50 in a mirror block, a point source at the focus (0, 0, -40) emitting
  into the whole sphere, through runSimulation: every ray passes the other focus after its first reflection (the
  path F1 -> hit -> F2 measures 2 rz = 100) and comes back through the first after the second"""
  from freecad.optics_design_workbench_amd.simulation.simulation_loop import runSimulation
  F1, F2, n = np.array([0.0, 0.0, -40.0]), np.array([0.0, 0.0, 40.0]), 4100
  from freecad.optics_design_workbench_amd.scene.placement import Placement
  doc, src = ec.document(
      [('Mirror', lambda d: [make.makeCut(d, ec.centred_box(d, 'B', *ec.CUBE), ec.ellipsoid(d, 'E', (30.0, 30.0, 50.0)))],
        dict(RecordHits=True, Reflectivity=0.9))],
      source=dict(PowerDensity='1', ThetaDomain='0, pi', placement=Placement(base=tuple(F1))),
      MaxIntersections=3.0, RaysPerIteration=float(n), EndAfterRays='4100', StoreHitInitDirection=True)
  runs = []
  for mode in MODES:
    store = runSimulation(doc, 'singletrue', device=0, compileScene=mode, seed=SEED)
    assert store.totalTracedRays == n
    runs.append(store.hits().hits)
  for col in ('points', 'directions', 'powers', 'initDirection'):
    assert np.array_equal(runs[0][col], runs[1][col]), col
  h = runs[0]
  assert len(h['points']) == 3 * n
  # a ray's rows share its initial direction; the power tells the bounce (0.9 per reflection)
  _, ray = np.unique(h['initDirection'], axis=0, return_inverse=True)
  ray = ray.ravel()
  bounce = np.rint(np.log(h['powers']) / np.log(0.9)).astype(int)
  assert np.abs(h['powers'] - 0.9**bounce).max() < ec.POWER_TOL and np.array_equal(np.bincount(ray), np.full(n, 3))
  order = np.lexsort((bounce, ray))
  pts = h['points'][order].reshape(n, 3, 3)
  assert np.array_equal(bounce[order].reshape(n, 3), np.tile([0, 1, 2], (n, 1)))
  h0, h1, h2 = pts[:, 0], pts[:, 1], pts[:, 2]
  figures = (ec.point_line_distance(F2, h0, h1).max(),
             np.abs(np.linalg.norm(h0 - F1, axis=1) + np.linalg.norm(F2 - h0, axis=1) - 100.0).max(),
             ec.point_line_distance(F1, h1, h2).max())
  print('past F2 %.3e, path %.3e, past F1 %.3e mm' % figures)
  assert max(figures) < ec.TOL
  # the whole sphere of directions was used, and every first hit lies on the cavity
  d0 = h['initDirection'][order].reshape(n, 3, 3)[:, 0]
  assert d0[:, 2].min() < -0.99 and d0[:, 2].max() > 0.99
  assert np.abs(((h0 / np.array([30.0, 30.0, 50.0]))**2).sum(1) - 1.0).max() < 1e-10


# ---- 4 ---------------------------------------------------------------------------------------------------------------
def test_aberration_free_lens(native_lib):
  """a prolate spheroid of eccentricity 1 / n: rays parallel to its axis meet at the far focus inside the glass --
  normal and Snell's law on the new surface"""
  radii, n = (np.sqrt(500.0), np.sqrt(500.0), 30.0), 4100
  sc, lim = ec.baked([('Lens', lambda d: [ec.ellipsoid(d, 'E', radii)], dict(RefractiveIndex=1.5))])
  rng = np.random.default_rng(5)
  rho, phi = 0.95 * radii[0] * np.sqrt(rng.uniform(0, 1, n)), rng.uniform(0, 2 * np.pi, n)
  o = np.stack([rho * np.cos(phi), rho * np.sin(phi), np.full(n, -100.0)], axis=1)
  d = np.tile([0.0, 0.0, 1.0], (n, 1))
  rows = _both(sc, lim, o, d)
  assert len(rows) == 2 * n
  ray = (rows['tag'] & np.uint64(0xFFFFFFFFFFFF)).astype(np.int64)
  entering = (rows['tag'] >> np.uint64(63)).astype(bool)
  assert np.array_equal(ray[entering], np.arange(n)) and np.array_equal(ray[~entering], np.arange(n))
  h0, h1 = rows['point'][entering], rows['point'][~entering]
  assert np.abs(h0[:, :2] - o[:, :2]).max() < ec.TOL and h0[:, 2].max() < 0 < h1[:, 2].min()
  worst = ec.point_line_distance([0.0, 0.0, 20.0], h0, h1).max()
  print(f'past the far focus {worst:.3e} mm')
  assert worst < ec.TOL


# ---- 5 ---------------------------------------------------------------------------------------------------------------
def test_an_ellipsoid_that_is_a_sphere(native_lib, oracle):
  """a ball lens written as Part::Ellipsoid(R, R, R) on the device against the same document with Part::Sphere(R) on
  the oracle: same tags and counters, points within 1e-9 mm, powers within 1e-12"""
  from freecad.optics_design_workbench_amd.freecad_elements import point_source
  from freecad.optics_design_workbench_amd.scene import bake
  from freecad.optics_design_workbench_amd.simulation.tracer import Tracer
  R, n = 10.0, 4100

  def project(ball):
    doc, src = ec.document([('Lens', lambda d: [ball(d)], dict(RefractiveIndex=1.5, RecordHits=True, AbsorptionLength='40.0')),
                            ('Absorber', lambda d: [make.makeBox(d, 'A', 100, 100, 1, base=(-50, -50, 60))], {})],
                           source=dict(PowerDensity='exp(-theta^2/0.05)'))
    return bake.bakeScene(doc, src), point_source.bakeSource(doc, src), bake.bakeLimits(doc, src)
  sphere = project(lambda d: make.makeSphere(d, 'S', R, base=(1.0, -0.5, 30.0)))
  ell = project(lambda d: make.makeEllipsoid(d, 'S', R, R, R, base=(1.0, -0.5, 30.0)))
  assert list(sphere[0].prim_type) == [1, 0] and list(ell[0].prim_type) == [7, 0]
  ref = oracle.trace(sphere[0], sphere[1], sphere[2], 0, n, SEED, hit_capacity=4 * n, nthreads=0)
  got = []
  for mode in MODES:
    with Tracer(0) as tr:
      tr.compileScene(mode)
      tr.setScene(ell[0])
      tr.setSource(ell[1])
      tr.setLimits(ell[2])
      tr.setDetector(None)
      tr.reserveHits(4 * n)
      tr.reset()
      tr.trace(0, n, SEED)
      tr.sync()
      assert tr.compiledInfo()['mode'] == MODES.index(mode)
      got.append(dict(rows=tr.hits(), counters=tr.counters()))
  _same_rows(got[0], got[1])
  rows, want = got[0]['rows'], ref['hits']
  assert got[0]['counters'] == ref['counters'] and len(want) > 2 * n
  assert np.array_equal(rows['tag'], want['tag'])
  figures = (np.abs(rows['point'] - want['point']).max(), np.abs(rows['direction'] - want['direction']).max(),
             np.abs(rows['power'] - want['power']).max())
  print('points %.3e mm, directions %.3e, powers %.3e' % figures)
  assert figures[0] < ec.TOL and figures[1] < ec.TOL and figures[2] < ec.POWER_TOL
  assert len(np.unique(rows['power'])) > n // 2                     # (the absorbing glass moves the power)


# ---- 6 ---------------------------------------------------------------------------------------------------------------
def test_lattice_takes_the_grid_or_the_tree(native_lib):
  """75 small ellipsoids: more than a compiled kernel takes -- the grid kernel's item branch (or the tree)"""
  from freecad.optics_design_workbench_amd import _native
  sc, lim = ec.lattice_scene()
  assert _native.build_check(sc, lim)['structure'] in ('grid', 'bvh')
  o, d = ec.random_lines(300, seed=11, span=30.0)
  want, excluded = ec.lattice_expected(o, d)
  assert sum(len(w) > 0 for w in want) > 100
  out = _launch(sc, lim, o, d, 'structure')
  assert out['info']['mode'] == 0
  _held(ec.per_ray(out['rows'], o, d), want, excluded)


def test_segment_rows_take_the_tree(native_lib, scene1):
  """record_segments: the binary-tree kernel.  The hit rows are those of the launch without segments"""
  sc, lim, o, d, want = scene1
  plain = _launch(sc, lim, o, d)
  seg = _launch(sc, lim, o, d, segments=True)
  for col in ('tag', 'point', 'direction', 'power'):
    assert np.array_equal(plain['rows'][col], seg['rows'][col]), col
  # one segment up to every recorded point and one beyond the last
  assert len(seg['segments']) == len(plain['rows']) + len(o)
  _held(ec.per_ray(seg['rows'], o, d), want)


def test_facets_beside_an_ellipsoid_take_the_binary_tree(native_lib, scene1):
  """a tessellated ball in the scene: the mesh kernel's eight-wide tree does not know the kind, the binary tree does"""
  from freecad.optics_design_workbench_amd import _native
  _, lim, o, d, want = scene1
  ball = np.array([40.0, 300.0, -200.0])
  assert ec.point_line_distance(ball, o, o + d).min() > 10.0                      # (no line of the scene meets the ball)
  sc, _ = ec.vacuum(lambda doc: [ec.ellipsoid(doc, 'E', ec.RADII, **ec.PLACEMENTS[1]),
                                 make.makeTessellated(doc, make.makeSphere(doc, 'S', 5.0, base=tuple(ball)), 16)])
  assert _native.build_check(sc, lim)['structure'] == 'bvh' and (np.asarray(sc.prim_type) == 5).sum() > 100
  o2, d2 = np.vstack([o, ball + [0.7, 0.4, -50.0]]), np.vstack([d, [0.0, 0.0, 1.0]])
  got = ec.per_ray(_launch(sc, lim, o2, d2)['rows'], o2, d2)
  _held(got[:-1], want)
  assert len(got[-1]) == 2 and np.abs(np.linalg.norm(got[-1] - ball, axis=1) - 5.0).max() < 0.2   # (through the facets)


def test_power_weighted_detector_map(native_lib, scene1):
  """setDetector(det, power=True): count plane and power plane are numpy's binning of the launch's own rows"""
  sc, lim, o, d, want = scene1
  det = dict(group=-1, origin=(3.0, -7.0, 11.0), ex=(1.0, 0.0, 0.0), ey=(0.0, 0.0, 1.0), x_lo=-25.0, x_hi=25.0, y_lo=-45.0,
             y_hi=45.0, nx=20, ny=36)
  for mode in MODES:
    out = _launch(sc, lim, o, d, mode, det=det, power=True)
    counts, power, outside = power_scene.planes(out['rows'], det)
    assert counts.sum() > 20 and outside > 0 and out['counters']['hist_overflow'] == outside
    assert np.array_equal(out['hist'], counts) and np.array_equal(out['power'], power)
  _held(ec.per_ray(out['rows'], o, d), want)


# ---- 7 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['ellipsoid', 'paraboloid'])
def test_batch_of_three_radii(native_lib, kind):
  """setSceneBatch of three values of Radius1 (the semi-axis along z): one launch of the compiled kernel's batch variant
  equals three single launches, bit for bit -- of the compiled kernel, and so (test 1 to 5) of the generic ones.
  Without a compiled kernel such a batch is refused: the generic flat kernel, which traces batches, leaves the kind out.
  The rule is the same for the other rare quadric (three focal lengths of a paraboloid)"""
  from freecad.optics_design_workbench_amd import _native
  from freecad.optics_design_workbench_amd.freecad_elements import point_source
  from freecad.optics_design_workbench_amd.scene import bake
  from freecad.optics_design_workbench_amd.simulation.tracer import Tracer
  solid = (lambda d: make.makeEllipsoid(d, 'Solid', 12.0, 9.0, 8.0, base=(0.5, 0.0, 30.0))) if kind == 'ellipsoid' else \
          (lambda d: make.makeParaboloid(d, 'Solid', 11.0, 6.0, base=(0.5, 0.0, 25.0)))
  doc, src = ec.document([('Lens', lambda d: [solid(d)], dict(RefractiveIndex=1.5)),
                          ('Absorber', lambda d: [make.makeBox(d, 'A', 100, 100, 1, base=(-50, -50, 60))], {})],
                         source=dict(PowerDensity='exp(-theta^2/0.05)'))
  prs = []
  for r1 in (11.0, 12.0, 13.7):
    if kind == 'ellipsoid':
      doc.Solid.Radius1 = r1
    else:
      doc.Solid.FocalLength = r1
    prs.append((bake.bakeScene(doc, src), point_source.bakeSource(doc, src), bake.bakeLimits(doc, src)))
  assert [float(p[0].prim_params[0][2 if kind == 'ellipsoid' else 0]) for p in prs] == [11.0, 12.0, 13.7]
  n, cap = 4100, 4100 + 1024
  singles = {}
  for mode in MODES:
    with Tracer(0) as tr:
      tr.compileScene(mode)
      singles[mode] = []
      for sc, bs, lim in prs:
        tr.setScene(sc)
        tr.setSource(bs)
        tr.setLimits(lim)
        tr.setDetector(None)
        tr.reserveHits(cap)
        tr.reset()
        tr.trace(0, n, SEED, histogram=False)
        tr.sync()
        assert tr.compiledInfo()['mode'] == MODES.index(mode)
        singles[mode].append(tr.hits())
      tr.setLimits(prs[0][2])
      tr.setSource(prs[0][1])
      if mode == 'off':
        with pytest.raises(_native.NativeError, match='unsupported'):
          tr.setSceneBatch([p[0] for p in prs])
        continue
      tr.setSceneBatch([p[0] for p in prs])
      tr.reset()
      tr.traceBatch(0, n, SEED, cap)
      tr.sync()
      assert tr.counters()['traced_rays'] == 3 * n
      for k, want in enumerate(singles[mode]):
        tr.batchSelect(k)
        got = tr.hits()
        for col in ('tag', 'point', 'direction', 'power'):
          assert np.array_equal(got[col], want[col]), (k, col)
      tr.batchSelect(None)
  for a, b in zip(singles['off'], singles['structure']):
    assert len(a) > n // 2 and all(np.array_equal(a[col], b[col]) for col in ('tag', 'point', 'direction', 'power'))
  assert not np.array_equal(singles['off'][0]['point'][:100], singles['off'][1]['point'][:100])
