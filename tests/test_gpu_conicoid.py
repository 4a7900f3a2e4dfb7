"""The conicoid (primitive kind 8) on the device, held to closed forms evaluated here in float64 (tests/conicoid_cases.py;
the CPU oracle does not know the kind): crossings for every family of the conic constant, trimming against a box in
both directions, the hyperbolic mirror from focus to focus, the aberration-free plano-hyperbolic lens, the members the
engine already has under other names (spherical cap, paraboloid, spheroid caps), and every route: the compiled kernel
with the value image's new entries, the grid kernel's item branch, the binary tree, batch launches, a lens built by
make.makeConicLens under a point source.  Every recorded point within 1e-9 mm, powers within 1e-12, counts exact; the
generic and the compiled launch of a scene agree row for row, bit for bit."""
import numpy as np
import pytest

import conicoid_cases as cc
import power_scene
from freecad.optics_design_workbench_amd.freecad_elements import make
from freecad.optics_design_workbench_amd.scene.placement import Placement

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


def _held(got, want, excluded=None):
  """every line (the reference excludes none, tests/test_conicoid.py): the expected number of points, each within TOL"""
  assert excluded is None or excluded.sum() == 0
  worst = 0.0
  for k, (g, w) in enumerate(zip(got, want)):
    assert len(g) == len(w), (k, g, w)
    if len(w):
      worst = max(worst, float(np.abs(g - w).max()))
  print(f'worst deviation {worst:.3e} mm over {len(want)} lines')
  assert worst < cc.TOL


def _by_ray(rows, n):
  """rows sorted by ray, in the order they were recorded -> (ray numbers, rows)"""
  ray = (rows['tag'] & np.uint64(0xFFFFFFFFFFFF)).astype(np.int64)
  order = np.argsort(ray, kind='stable')
  return ray[order], rows[order]


# ---- 1 ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def scene1():
  """the hyperboloid, moved and turned, with its lines and what they record"""
  pl = cc.PLACEMENTS[1]
  K, H = cc.CASES[0]
  O, D, want, excluded, _ = cc.crossing_lines(K, H)
  sc, lim = cc.vacuum(lambda d: [cc.conicoid(d, 'C', cc.R0, K, H, **pl)])
  return sc, lim, cc.to_world(pl, points=O), cc.to_world(pl, dirs=D), [cc.to_world(pl, points=w) for w in want]


@pytest.mark.parametrize('pl', cc.PLACEMENTS, ids=['at-origin', 'moved'])
@pytest.mark.parametrize('case', cc.CASES, ids=cc.IDS)
def test_crossings(native_lib, case, pl):
  """lines along and parallel to the axis, through the vertex, chords, through the rim -+ 1e-6, a line that clears the
  surface by 1e-9 mm (nothing) beside one 1e-6 mm inside (its chord), rays that start inside (one point: the cap, the
  surface); for the hyperboloid a line along an asymptote direction, one steeper, two through the absent sheet"""
  K, H = case
  O, D, want, excluded, counts = cc.crossing_lines(K, H)
  sc, lim = cc.vacuum(lambda d: [cc.conicoid(d, 'C', cc.R0, K, H, **pl)])
  o, d = cc.to_world(pl, points=O), cc.to_world(pl, dirs=D)
  rows = _both(sc, lim, o, d)
  got = cc.per_ray(rows, o, d)
  print([len(g) for g in got])
  _held(got, [cc.to_world(pl, points=w) for w in want], excluded)
  assert len(rows) == sum(len(w) for w in want)


# ---- 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', cc.TRIMS)
def test_trimmed_by_a_box(native_lib, case):
  """Cut(block, conicoid): the "outside the conicoid" literal on the box, the flipped faces of the cavity;
  Cut(conicoid, drill) and Common(conicoid, half): the conicoid's faces outside / inside the box"""
  o, d = cc.trim_lines(case)
  sc, lim = cc.trim_scene(case)
  want, excluded = cc.trim_expected(case, o, d)
  rows = _both(sc, lim, o, d)
  # every recorded point lies on the boundary of the result: its distance rule vanishes there (first order: a point
  # within 1e-9 mm of the boundary in every coordinate is within sqrt(3) 1e-9 of it)
  worst = np.abs(cc.trim_distance(case, rows['point'])).max()
  print(f'recorded points off the boundary of the result by {worst:.3e} mm at most')
  assert worst < 2 * cc.TOL
  _held(cc.per_ray(rows, o, d), want, excluded)


# ---- 3 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('side', ['convex', 'concave'])
def test_hyperbolic_mirror(native_lib, side):
  """K = -2.25, R = 10, H = 8.  Convex: 4 100 rays aimed at the inner focus from outside reflect through the outer one.
  Concave (the cavity of Cut(block, conicoid)): rays from the inner focus leave along lines through the outer one.  An
  absorber catches the reflected rays; the line from the mirror to it is the reflected ray"""
  concave = side == 'concave'
  o, d = cc.mirror_concave_rays() if concave else cc.mirror_convex_rays()
  x_ref, r_ref, _ = cc.mirror_reference(o, d, concave)
  body = (lambda doc: [make.makeCut(doc, cc.centred_box(doc, 'B', *cc.BLOCK), cc.conicoid(doc, 'C', **_rkh(cc.MIRROR)))]) if concave else \
         (lambda doc: [cc.conicoid(doc, 'C', **_rkh(cc.MIRROR))])
  # (convex: the reflected rays come down through the outer focus at z = -20; concave: they leave upwards)
  slab = (lambda doc: [make.makeBox(doc, 'A', 400, 400, 1, base=(-200, -200, 60.0 if concave else -61.0))])
  sc, lim = cc.baked([('Mirror', body, dict(RecordHits=True)), ('Absorber', slab, {})])
  rows = _both(sc, lim, o, d)
  n = len(o)
  assert len(rows) == 2 * n
  ray, rows = _by_ray(rows, n)
  assert np.array_equal(ray, np.repeat(np.arange(n), 2))
  h0, h1 = rows['point'][0::2], rows['point'][1::2]
  figures = (np.abs(h0 - x_ref).max(), cc.point_line_distance(cc.F_OUTER, h0, h1).max(), np.abs(rows['power'] - 1.0).max())
  print('mirror points %.3e mm, past the outer focus %.3e mm, powers %.3e' % figures)
  assert figures[0] < cc.TOL and figures[1] < cc.TOL and figures[2] < cc.POWER_TOL
  assert np.abs(np.abs(h1[:, 2]) - (60.0 if concave else 60.0)).max() < cc.TOL


def _rkh(spec):
  return dict(R=spec['R'], K=spec['K'], H=spec['H'])


# ---- 4 ---------------------------------------------------------------------------------------------------------------
def test_aberration_free_lens(native_lib):
  """n = 1.5, f = 40, R = f (n - 1), K = -n^2, H = 6: rays entering the cap along -z meet at (0, 0, -f) -- normal and
  Snell's law on the new surface"""
  o, d = cc.lens_rays()
  x_ref, r_ref, _ = cc.lens_reference(o, d)
  sc, lim = cc.baked([('Lens', lambda doc: [cc.conicoid(doc, 'C', **_rkh(cc.LENS))], dict(RefractiveIndex=cc.LENS['n'], RecordHits=True)),
                      ('Absorber', lambda doc: [make.makeBox(doc, 'A', 400, 400, 1, base=(-200, -200, -61.0))], {})])
  rows = _both(sc, lim, o, d)
  n = len(o)
  assert len(rows) == 3 * n
  ray, rows = _by_ray(rows, n)
  assert np.array_equal(ray, np.repeat(np.arange(n), 3))
  h0, h1, h2 = rows['point'][0::3], rows['point'][1::3], rows['point'][2::3]
  assert np.abs(h0[:, :2] - o[:, :2]).max() < cc.TOL and np.abs(h0[:, 2] - cc.LENS['H']).max() < cc.TOL
  figures = (np.abs(h1 - x_ref).max(), cc.point_line_distance([0.0, 0.0, -cc.LENS['f']], h1, h2).max())
  print('leaving points %.3e mm, past the focus %.3e mm' % figures)
  assert max(figures) < cc.TOL


# ---- 5 ---------------------------------------------------------------------------------------------------------------
def _source_launch(pr, mode, n, cap):
  from freecad.optics_design_workbench_amd.simulation.tracer import Tracer
  with Tracer(0) as tr:
    tr.compileScene(mode)
    tr.setScene(pr[0])
    tr.setSource(pr[1])
    tr.setLimits(pr[2])
    tr.setDetector(None)
    tr.reserveHits(cap)
    tr.reset()
    tr.trace(0, n, SEED)
    tr.sync()
    assert tr.compiledInfo()['mode'] == MODES.index(mode)
    return dict(rows=tr.hits(), counters=tr.counters())


@pytest.mark.parametrize('case', cc.CASES[1:], ids=cc.IDS[1:])
def test_against_what_already_exists(native_lib, oracle, case):
  """a lens under a point source, written as a conicoid and as what the engine has had: K = 0 against the oracle on
  Common(sphere, slab), K = -1 against the oracle on the paraboloid of focal length R / 2, K = -0.5 and +1 against the
  device on Common(ellipsoid, slab).  Same tags and counters, points within 1e-9 mm, powers within 1e-12; the
  reference's own rows keep clear of the rim by 1e-6 mm"""
  from freecad.optics_design_workbench_amd.freecad_elements import point_source
  from freecad.optics_design_workbench_amd.scene import bake
  K, H = case
  R, n = cc.R0, 4100
  base = (1.0, -0.5, 30.0)
  slab = lambda d: make.makeBox(d, 'Slab', 100, 100, H, base=(base[0] - 50, base[1] - 50, base[2]))
  if K == 0.0:
    other = lambda d: make.makeCommon(d, [make.makeSphere(d, 'S', R, base=(base[0], base[1], base[2] + R)), slab(d)])
  elif K == -1.0:
    other = lambda d: make.makeParaboloid(d, 'P', R / 2, H, base=base)
  else:
    rz, rxy = R / (1.0 + K), R / np.sqrt(1.0 + K)
    other = lambda d: make.makeCommon(d, [make.makeEllipsoid(d, 'E', rz, rxy, rxy, base=(base[0], base[1], base[2] + rz)), slab(d)])

  def project(solid):
    doc, src = cc.document([('Lens', lambda d: [solid(d)], dict(RefractiveIndex=1.5, RecordHits=True, AbsorptionLength='40.0')),
                            ('Absorber', lambda d: [make.makeBox(d, 'A', 100, 100, 1, base=(-50, -50, 60))], {})],
                           source=dict(PowerDensity='exp(-theta^2/0.05)'))
    return bake.bakeScene(doc, src), point_source.bakeSource(doc, src), bake.bakeLimits(doc, src)
  mine, theirs = project(lambda d: cc.conicoid(d, 'C', R, K, H, base=base)), project(other)
  assert list(mine[0].prim_type) == [8, 0]
  if K in (0.0, -1.0):
    ref = oracle.trace(theirs[0], theirs[1], theirs[2], 0, n, SEED, hit_capacity=4 * n, nthreads=0)
    want, want_counters = ref['hits'], ref['counters']
  else:
    ref = _source_launch(theirs, 'off', n, 4 * n)
    want, want_counters = ref['rows'], ref['counters']
  # the reference's rows on the lens: none within 1e-6 mm of the rim circle
  local = want['point'] - np.array(base)
  on_lens = local[:, 2] < H + 1.0
  assert on_lens.sum() > n and cc.rim_distance(local[on_lens], R, K, H).min() > cc.RIM_TOL
  got = [_source_launch(mine, mode, n, 4 * n) for mode in MODES]
  _same_rows(got[0], got[1])
  rows = got[0]['rows']
  assert got[0]['counters'] == want_counters and len(want) > 2 * n
  assert np.array_equal(rows['tag'], want['tag'])
  figures = (np.abs(rows['point'] - want['point']).max(), np.abs(rows['direction'] - want['direction']).max(),
             np.abs(rows['power'] - want['power']).max())
  print('points %.3e mm, directions %.3e, powers %.3e' % figures)
  assert figures[0] < cc.TOL and figures[1] < cc.TOL and figures[2] < cc.POWER_TOL
  assert len(np.unique(rows['power'])) > n // 2                     # (the absorbing glass moves the power)


# ---- 6 ---------------------------------------------------------------------------------------------------------------
def test_segment_rows_take_the_tree(native_lib, scene1):
  """record_segments: the binary-tree kernel.  The hit rows are those of the launch without segments"""
  sc, lim, o, d, want = scene1
  plain = _launch(sc, lim, o, d)
  seg = _launch(sc, lim, o, d, segments=True)
  for col in ('tag', 'point', 'direction', 'power'):
    assert np.array_equal(plain['rows'][col], seg['rows'][col]), col
  # one segment up to every recorded point and one beyond the last
  assert len(seg['segments']) == len(plain['rows']) + len(o)
  _held(cc.per_ray(seg['rows'], o, d), want)


def test_facets_beside_a_conicoid_take_the_binary_tree(native_lib, scene1):
  """a tessellated ball in the scene: the mesh kernel's eight-wide tree does not know the kind, the binary tree does"""
  from freecad.optics_design_workbench_amd import _native
  _, lim, o, d, want = scene1
  ball = np.array([40.0, 300.0, -200.0])
  assert cc.point_line_distance(ball, o, o + d).min() > 10.0                      # (no line of the scene meets the ball)
  K, H = cc.CASES[0]
  sc, _ = cc.vacuum(lambda doc: [cc.conicoid(doc, 'C', cc.R0, K, H, **cc.PLACEMENTS[1]),
                                 make.makeTessellated(doc, make.makeSphere(doc, 'S', 5.0, base=tuple(ball)), 16)])
  assert _native.build_check(sc, lim)['structure'] == 'bvh' and (np.asarray(sc.prim_type) == 5).sum() > 100
  o2, d2 = np.vstack([o, ball + [0.7, 0.4, -50.0]]), np.vstack([d, [0.0, 0.0, 1.0]])
  got = cc.per_ray(_launch(sc, lim, o2, d2)['rows'], o2, d2)
  _held(got[:-1], want)
  assert len(got[-1]) == 2 and np.abs(np.linalg.norm(got[-1] - ball, axis=1) - 5.0).max() < 0.2   # (through the facets)


def test_power_weighted_detector_map(native_lib, scene1):
  """setDetector(det, power=True): count plane and power plane are numpy's binning of the launch's own rows"""
  sc, lim, o, d, want = scene1
  det = dict(group=-1, origin=(3.0, -7.0, 11.0), ex=(1.0, 0.0, 0.0), ey=(0.0, 0.0, 1.0), x_lo=-12.0, x_hi=12.0, y_lo=-10.0,
             y_hi=10.0, nx=20, ny=36)
  for mode in MODES:
    out = _launch(sc, lim, o, d, mode, det=det, power=True)
    counts, power, outside = power_scene.planes(out['rows'], det)
    assert counts.sum() > 20 and outside > 0 and out['counters']['hist_overflow'] == outside
    assert np.array_equal(out['hist'], counts) and np.array_equal(out['power'], power)
  _held(cc.per_ray(out['rows'], o, d), want)


@pytest.mark.parametrize('swept', ['K', 'R'])
def test_batch_of_three(native_lib, swept):
  """setSceneBatch of three conic constants (of three vertex radii): one launch of the compiled kernel's batch variant
  equals three single launches, bit for bit -- of the compiled kernel, and so of the generic ones.  Without a compiled
  kernel such a batch is refused: the generic flat kernel, which traces batches, leaves the kind out"""
  from freecad.optics_design_workbench_amd import _native
  from freecad.optics_design_workbench_amd.freecad_elements import point_source
  from freecad.optics_design_workbench_amd.scene import bake
  from freecad.optics_design_workbench_amd.simulation.tracer import Tracer
  doc, src = cc.document([('Lens', lambda d: [cc.conicoid(d, 'Solid', 12.0, -1.5, 6.0, base=(0.5, 0.0, 25.0))], dict(RefractiveIndex=1.5)),
                          ('Absorber', lambda d: [make.makeBox(d, 'A', 100, 100, 1, base=(-50, -50, 60))], {})],
                         source=dict(PowerDensity='exp(-theta^2/0.05)'))
  prs = []
  values = (-2.25, -1.5, 0.4) if swept == 'K' else (11.0, 12.0, 13.7)
  for v in values:
    if swept == 'K':
      doc.Solid.ConicConstant = v
    else:
      doc.Solid.VertexRadius = v
    prs.append((bake.bakeScene(doc, src), point_source.bakeSource(doc, src), bake.bakeLimits(doc, src)))
  assert [float(p[0].prim_params[0][1 if swept == 'K' else 0]) for p in prs] == list(values)
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


# ---- 7 ---------------------------------------------------------------------------------------------------------------
def test_conic_lens_collimates_a_point_source(native_lib):
  """make.makeConicLens (plano-hyperbolic, K = -n^2) in a lens group, a point source at the focus on the curved side
  emitting a cone, Tracer.trace() (rays generated on the device, the kernel compiled against the source): at an
  absorber behind the flat face every recorded direction is +z within 1e-12 in its transverse components"""
  from freecad.optics_design_workbench_amd.freecad_elements import point_source
  from freecad.optics_design_workbench_amd.scene import bake
  n_glass, f, n = cc.LENS['n'], cc.LENS['f'], 4100
  doc, src = cc.document(
      [('Lens', lambda d: [make.makeConicLens(d, 'L', f * (n_glass - 1.0), -n_glass**2, float('inf'), 0.0, 6.0, 30.0)], dict(RefractiveIndex=n_glass)),
       ('Absorber', lambda d: [make.makeBox(d, 'A', 100, 100, 1, base=(-50, -50, 40))], {})],
      source=dict(PowerDensity='1', ThetaDomain='0, 0.3', placement=Placement(base=(0.0, 0.0, -f))))
  pr = (bake.bakeScene(doc, src), point_source.bakeSource(doc, src), bake.bakeLimits(doc, src))
  assert sorted(pr[0].prim_type) == [0, 2, 8]
  got = [_source_launch(pr, mode, n, 2 * n) for mode in MODES]
  _same_rows(got[0], got[1])
  rows = got[0]['rows']
  assert len(rows) == n and got[0]['counters']['traced_rays'] == n
  worst = np.abs(rows['direction'][:, :2]).max()
  print(f'transverse direction components at the absorber {worst:.3e}')
  assert worst < 1e-12 and np.all(rows['direction'][:, 2] > 0)
  # the cone filled its part of the aperture: the collimated beam is a little wider than f tan(0.3) (the rays meet the
  # surface behind the vertex plane) and narrower than the lens
  assert f * np.tan(0.3) < np.hypot(rows['point'][:, 0], rows['point'][:, 1]).max() < 15.0
