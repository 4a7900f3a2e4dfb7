"""The even asphere (primitive kind 9) on the device, held to numbers worked out in numpy (tests/asphere_cases.py; the
CPU oracle does not know the kind): crossings of the general prescription against bracketing + bisection and of the
closed-form members against their closed forms and against kinds 6 and 8 on the device, the four crossings of a
hill-and-moat profile, trimming both ways, a parabolic mirror and Snell's law on the analytic normal, every route
(binary tree, beside facets, the grid's item branch), batches, and a singlet of make.makeAsphericLens under a point
source.  Every recorded point within 1e-9 mm, powers within 1e-12, counts exact; the generic and the compiled launch of
a scene agree row for row, bit for bit; every face-0 row satisfies |z - sag(rho)| <= 1e-9 in the local frame."""
import numpy as np
import pytest

import asphere_cases as ac
from freecad.optics_design_workbench_amd.freecad_elements import make
from freecad.optics_design_workbench_amd.scene.placement import Placement

pytestmark = pytest.mark.gpu

SEED = 0x0D15EA5E
MODES = ['off', 'structure']


def _launch(sc, lim, o, d, mode='off', segments=False):
  """explicit rays through a tracer of its own -> dict(rows, counters, info, [segments])"""
  from freecad.optics_design_workbench_amd.simulation.tracer import Tracer
  with Tracer(0) as tr:
    tr.compileScene(mode)
    tr.setScene(sc)
    tr.setLimits(lim)
    tr.setDetector(None)
    tr.reserveHits(len(o) * (lim.max_intersections + 1))
    if segments:
      tr.reserveSegments(len(o) * (lim.max_intersections + 1))
    tr.reset()
    tr.traceRays(o, d, record_segments=segments, histogram=False)
    tr.sync()
    out = dict(rows=tr.hits(), counters=tr.counters(), info=tr.compiledInfo())
    assert out['counters']['hits_dropped'] == 0
    if segments:
      out['segments'] = tr.segments()
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
  """every line (the reference excludes none): the expected number of points, each within TOL"""
  assert excluded is None or excluded.sum() == 0, np.nonzero(excluded)[0]
  worst = 0.0
  for k, (g, w) in enumerate(zip(got, want)):
    assert len(g) == len(w), (k, g, w)
    if len(w):
      worst = max(worst, float(np.abs(g - w).max()))
  print(f'worst deviation {worst:.3e} mm over {len(want)} lines')
  assert worst < ac.TOL


def _by_ray(rows):
  ray = (rows['tag'] & np.uint64(0xFFFFFFFFFFFF)).astype(np.int64)
  order = np.argsort(ray, kind='stable')
  return ray[order], rows[order]


def _on_surface(points, spec, pl=None):
  """the rows that lie on face 0 (clear of wall and cap) satisfy the surface's equation -> the largest residual"""
  x = np.asarray(points, float)
  if pl:
    inv = Placement(**pl).inverse().m
    x = x @ inv[:3, :3].T + inv[:3, 3]
  rho = np.hypot(x[:, 0], x[:, 1])
  face0 = (rho < spec['rim'] - 1e-3) & (x[:, 2] < spec['H'] - 1e-3)
  assert face0.sum() > 0
  worst = float(ac.residual(x[face0], spec).max())
  print(f'{face0.sum()} face-0 rows, residual |z - sag| at most {worst:.3e} mm')
  assert worst <= ac.TOL
  return worst


# ---- 1 ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lines1():
  """the general prescription's lines and what they record, worked out once (own frame)"""
  return ac.crossing_lines()


@pytest.fixture(scope='module')
def scene1(lines1):
  pl = ac.PLACEMENTS[1]
  O, D, want, excluded = lines1
  sc, lim = ac.vacuum(lambda d: [ac.asphere(d, 'A', ac.GENERAL, **pl)])
  return sc, lim, ac.to_world(pl, points=O), ac.to_world(pl, dirs=D), [ac.to_world(pl, points=w) for w in want]


@pytest.mark.parametrize('pl', ac.PLACEMENTS, ids=['at-origin', 'moved'])
def test_crossings_general_prescription(native_lib, lines1, pl):
  """c = 1/20, K = -0.8, a2 = 1e-5, a3 = -2e-8, a4 = 3e-11, rim 10, H 6: lines along and parallel to the axis, through
  the vertex, chords, through wall and cap, from inside, through the rim circle -+ 1e-6, a line that clears the surface
  by 1e-9 mm (nothing) beside one 1e-6 mm inside (its chord)"""
  O, D, want, excluded = lines1
  sc, lim = ac.vacuum(lambda d: [ac.asphere(d, 'A', ac.GENERAL, **pl)])
  o, d = ac.to_world(pl, points=O), ac.to_world(pl, dirs=D)
  rows = _both(sc, lim, o, d)
  got = ac.per_ray(rows, o, d)
  print([len(g) for g in got])
  _held(got, [ac.to_world(pl, points=w) for w in want], excluded)
  assert len(rows) == sum(len(w) for w in want)
  _on_surface(rows['point'], ac.GENERAL, pl)


@pytest.mark.parametrize('name', sorted(ac.MEMBERS))
def test_closed_form_members(native_lib, name):
  """c = 0 with a_1 alone, K = -1 with a_1 = a - c / 2 (conic and polynomial part sum to the paraboloid a rho^2), all
  coefficients zero with K = 0 (a sphere): crossings by the quadratic"""
  spec, o, d, want = ac.member_lines(name)
  sc, lim = ac.vacuum(lambda doc: [ac.asphere(doc, 'A', spec)])
  rows = _both(sc, lim, o, d)
  assert sum(len(w) for w in want) > 30
  _held(ac.per_ray(rows, o, d), want)


def _face0_rows(rows, o, d, rim, H):
  """per ray, the recorded points clear of wall and cap"""
  out = []
  for g in ac.per_ray(rows, o, d):
    keep = (np.hypot(g[:, 0], g[:, 1]) < rim - 1e-3) & (g[:, 2] < H - 1e-3)
    out.append(g[keep])
  return out


@pytest.mark.parametrize('K', ac.CONIC_KS)
def test_conic_members_against_the_conicoid(native_lib, K):
  """all coefficients zero: the conicoid's surface.  Rays that meet face 0 record the same points (1e-9 mm) as kind 8
  of the same vertex radius and conic constant on the device, and both lie on the closed-form crossings"""
  R, rim, H = ac.CONIC_R, ac.CONIC_RIM, ac.CONIC_H
  spec = dict(c=1.0 / R, K=K, coefs=(), rim=rim, H=H)
  o, d = ac.bundle(200, 0.4 * rim, 50.0, seed=61, tilt=0.05)
  o, d = np.vstack([o, o * [1, 1, -1]]), np.vstack([d, d * [1, 1, -1]])                  # from above and from below
  sa, lim = ac.vacuum(lambda doc: [ac.asphere(doc, 'A', spec)])
  sk, _ = ac.vacuum(lambda doc: [make.makeConicoid(doc, 'C', R, K, 8.0)])
  mine = _face0_rows(_both(sa, lim, o, d), o, d, rim, H)
  theirs = _face0_rows(_launch(sk, lim, o, d, 'structure')['rows'], o, d, rim, H)
  worst, n = 0.0, 0
  for k in range(len(o)):
    ts = [t for t in ac.conic_roots(o[k], d[k], R, K) if t > 0]
    x = np.array([o[k] + t * d[k] for t in ts]).reshape(-1, 3)
    x = x[(np.hypot(x[:, 0], x[:, 1]) < rim - 1e-3) & (x[:, 2] < H - 1e-3)]
    assert len(mine[k]) == len(theirs[k]) == len(x), k
    if len(x):
      worst = max(worst, np.abs(mine[k] - x).max(), np.abs(mine[k] - theirs[k]).max())
      n += len(x)
  print(f'K = {K}: {n} face-0 crossings, worst deviation {worst:.3e} mm')
  assert n >= len(o) and worst < ac.TOL


def test_paraboloid_member_against_kind_6(native_lib):
  """c = 0 with a_1 alone against the paraboloid of focal length 1 / (4 a_1) on the device"""
  spec = ac.MEMBERS['a1-alone']
  f = 1.0 / (4.0 * ac.PARABOLA_A)
  o, d = ac.bundle(300, 0.4 * spec['rim'], -50.0, seed=62, tilt=0.05)
  d = d * [1, 1, -1]
  sa, lim = ac.vacuum(lambda doc: [ac.asphere(doc, 'A', spec)])
  sp, _ = ac.vacuum(lambda doc: [make.makeParaboloid(doc, 'P', f, 8.0)])
  mine = _face0_rows(_both(sa, lim, o, d), o, d, spec['rim'], spec['H'])
  theirs = _face0_rows(_launch(sp, lim, o, d, 'structure')['rows'], o, d, spec['rim'], spec['H'])
  assert all(len(a) == len(b) == 1 for a, b in zip(mine, theirs))
  worst = max(np.abs(a - b).max() for a, b in zip(mine, theirs))
  print(f'worst deviation from kind 6: {worst:.3e} mm')
  assert worst < ac.TOL


# ---- 2 ---------------------------------------------------------------------------------------------------------------
def test_four_crossings(native_lib):
  """hill and moat (c = 0, a1 < 0 < a2), a level line through the axis between the moat's floor and the vertex:
  untrimmed, four surface rows at the closed-form abscissae; in a Common with a box over the far half, the third and the
  fourth only -- the smallest case in which 'the first two roots' would be wrong"""
  x4 = ac.moat_abscissae()
  assert len(x4) == 4 and np.all(np.diff(x4) > 1.0) and abs(x4[3]) < ac.MOAT['rim'] - 1.0
  o, d = np.array([[-100.0, 0.0, ac.MOAT_Z]]), np.array([[1.0, 0.0, 0.0]])
  want = np.array([[x, 0.0, ac.MOAT_Z] for x in x4])
  for trimmed, expect in ((False, want), (True, want[2:])):
    sc, lim = ac.moat_scene(trimmed)
    rows = _both(sc, lim, o, d)
    _held(ac.per_ray(rows, o, d), [expect])
    assert ac.residual(rows['point'], ac.MOAT).max() <= ac.TOL


# ---- 3 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ac.TRIMS)
def test_trimming_both_ways(native_lib, case):
  """Cut(block, asphere): the 'outside the asphere' literal through prim_sdist, the flipped faces of the cavity;
  Common(asphere, box): the other direction"""
  o, d = ac.trim_lines(case)
  sc, lim = ac.trim_scene(case)
  want, excluded = ac.trim_expected(case, o, d)
  rows = _both(sc, lim, o, d)
  worst = np.abs(ac.trim_distance(case, rows['point'])).max()
  print(f'recorded points off the boundary of the result by {worst:.3e} mm at most')
  assert worst < 2 * ac.TOL
  assert sum(len(w) for w in want) > 100
  _held(ac.per_ray(rows, o, d), want, excluded)


# ---- 4 ---------------------------------------------------------------------------------------------------------------
def test_parabolic_mirror(native_lib):
  """a_1 alone, the dish of Cut(block, asphere): an axis-parallel bundle from above reflects through (0, 0, 1 / (4 a_1)).
  An absorber catches the reflected rays: the segment from the mirror to it is the reflected ray"""
  o, d = ac.bundle(1500, 9.0, 50.0, seed=71)
  body = lambda doc: [make.makeCut(doc, ac.centred_box(doc, 'B', *ac.MIRROR_BLOCK), ac.asphere(doc, 'A', ac.MIRROR))]
  slab = lambda doc: [make.makeBox(doc, 'S', 400, 400, 1, base=(-200, -200, 80.0))]
  sc, lim = ac.baked([('Mirror', body, dict(RecordHits=True)), ('Absorber', slab, {})])
  rows = _both(sc, lim, o, d)
  n = len(o)
  assert len(rows) == 2 * n
  ray, rows = _by_ray(rows)
  assert np.array_equal(ray, np.repeat(np.arange(n), 2))
  h0, h1 = rows['point'][0::2], rows['point'][1::2]
  figures = (ac.residual(h0, ac.MIRROR).max(), np.abs(h0[:, :2] - o[:, :2]).max(), ac.point_line_distance(ac.FOCUS, h0, h1).max(),
             np.abs(rows['power'] - 1.0).max())
  print('mirror points off the surface %.3e mm, off their lines %.3e mm, past the focus %.3e mm, powers %.3e' % figures)
  assert max(figures[:3]) < ac.TOL and figures[3] < ac.POWER_TOL
  assert np.abs(h1[:, 2] - 80.0).max() < ac.TOL


def test_refraction_follows_the_analytic_normal(native_lib):
  """a lens group around the general prescription, a slanted bundle from below: the direction of the row after each
  face-0 hit is Snell's law, in numpy, on the analytic normal at the recorded point (1e-12)"""
  o, d = ac.bundle(1500, 4.0, -40.0, seed=72, tilt=0.08)
  d = d * [1, 1, -1]                                                       # upwards
  sc, lim = ac.baked([('Lens', lambda doc: [ac.asphere(doc, 'A', ac.GENERAL)], dict(RefractiveIndex=ac.LENS_N, RecordHits=True)),
                      ('Absorber', lambda doc: [make.makeBox(doc, 'S', 400, 400, 1, base=(-200, -200, 60.0))], {})])
  rows = _both(sc, lim, o, d)
  n = len(o)
  ray, rows = _by_ray(rows)
  assert len(rows) == 3 * n and np.array_equal(ray, np.repeat(np.arange(n), 3))
  first, second = rows[0::3], rows[1::3]
  assert ac.residual(first['point'], ac.GENERAL).max() <= ac.TOL
  assert np.abs(first['direction'] - d).max() < 1e-15
  want = ac.snell(d, ac.normal(first['point'], ac.GENERAL), 1.0 / ac.LENS_N)
  worst = np.abs(second['direction'] - want).max()
  print(f'refracted directions off Snell\'s law on the analytic normal by {worst:.3e}')
  assert worst < 1e-12
  assert np.abs(rows['power'] - 1.0).max() < ac.POWER_TOL


# ---- 5 ---------------------------------------------------------------------------------------------------------------
def test_segment_rows_take_the_tree(native_lib, scene1):
  """record_segments: the binary-tree kernel.  The hit rows are those of the flat (compiled) launch within TOL"""
  sc, lim, o, d, want = scene1
  flat = _launch(sc, lim, o, d, 'structure')
  seg = _launch(sc, lim, o, d, segments=True)
  assert np.array_equal(flat['rows']['tag'], seg['rows']['tag'])
  assert np.abs(flat['rows']['point'] - seg['rows']['point']).max() < ac.TOL
  assert len(seg['segments']) == len(flat['rows']) + len(o)
  _held(ac.per_ray(seg['rows'], o, d), want)


def test_facets_beside_an_asphere_take_the_binary_tree(native_lib, scene1):
  from freecad.optics_design_workbench_amd import _native
  _, lim, o, d, want = scene1
  ball = np.array([40.0, 300.0, -200.0])
  assert ac.point_line_distance(ball, o, o + d).min() > 10.0                      # (no line of the scene meets the ball)
  sc, _ = ac.vacuum(lambda doc: [ac.asphere(doc, 'A', ac.GENERAL, **ac.PLACEMENTS[1]),
                                 make.makeTessellated(doc, make.makeSphere(doc, 'S', 5.0, base=tuple(ball)), 16)])
  assert _native.build_check(sc, lim)['structure'] == 'bvh' and (np.asarray(sc.prim_type) == 5).sum() > 100
  o2, d2 = np.vstack([o, ball + [0.7, 0.4, -50.0]]), np.vstack([d, [0.0, 0.0, 1.0]])
  got = ac.per_ray(_launch(sc, lim, o2, d2)['rows'], o2, d2)
  _held(got[:-1], want)
  assert len(got[-1]) == 2 and np.abs(np.linalg.norm(got[-1] - ball, axis=1) - 5.0).max() < 0.2


def test_seventy_primitives_take_the_grid(native_lib):
  """35 aspheres among 35 spheres: the grid kernel's item branch.  Expected per line: the pieces of every asphere (the
  bisection source, in the asphere's frame) and the chords of every sphere"""
  from freecad.optics_design_workbench_amd import _native
  sc, lim = ac.lattice_scene()
  assert sc.n_prims == 70 and _native.build_check(sc, lim)['structure'] == 'grid'
  o, d = ac.lattice_lines()
  want, excluded = [], np.zeros(len(o), bool)
  for k in range(len(o)):
    ts = []
    for c in ac.LATTICE:
      if ac.point_line_distance(c + [0, 0, 3.0], o[k:k + 1], o[k:k + 1] + d[k:k + 1])[0] < 12.0:
        pcs, bad = ac.pieces(o[k] - c, d[k], ac.GENERAL)
        excluded[k] |= bad
        ts += [t for p in pcs for t in p]
      w = o[k] - (c + [0, 0, 14.0])
      b, cc_ = w @ d[k], w @ w - 16.0
      if b * b - cc_ > 0:
        sq = np.sqrt(b * b - cc_)
        excluded[k] |= 2 * sq < ac.APART
        ts += [-b - sq, -b + sq]
    want.append((o[k] + np.sort(ts)[:, None] * d[k]).reshape(-1, 3))
  assert sum(len(w) for w in want) > 100
  rows = _launch(sc, lim, o, d)['rows']
  _held(ac.per_ray(rows, o, d), want, excluded)


# ---- 6 ---------------------------------------------------------------------------------------------------------------
def _source_launch(pr, mode, n, cap, det=None, power=False):
  from freecad.optics_design_workbench_amd.simulation.tracer import Tracer
  with Tracer(0) as tr:
    tr.compileScene(mode)
    tr.setScene(pr[0])
    tr.setSource(pr[1])
    tr.setLimits(pr[2])
    tr.setDetector(det, power=power) if det is not None else tr.setDetector(None)
    tr.reserveHits(cap)
    tr.reset()
    tr.trace(0, n, SEED, histogram=det is not None)
    tr.sync()
    assert tr.compiledInfo()['mode'] == MODES.index(mode)
    out = dict(rows=tr.hits(), counters=tr.counters())
    if det is not None:
      out['hist'] = tr.histogram()
      out['power'] = tr.powerHistogramRaw() if power else None
    return out


def test_batch_of_three(native_lib):
  """three scenes that differ in K and a_2 only, in one launch of the compiled kernel's batch variant: identical, bit
  for bit, to three single launches, with one compilation; the generic batch is refused"""
  from freecad.optics_design_workbench_amd import _native
  from freecad.optics_design_workbench_amd.freecad_elements import point_source
  from freecad.optics_design_workbench_amd.scene import bake
  from freecad.optics_design_workbench_amd.simulation.tracer import Tracer
  spec = dict(ac.GENERAL)
  doc, src = ac.document([('Lens', lambda d: [ac.asphere(d, 'Solid', spec, base=(0.5, 0.0, 25.0))], dict(RefractiveIndex=1.5)),
                          ('Absorber', lambda d: [make.makeBox(d, 'A', 100, 100, 1, base=(-50, -50, 60))], {})],
                         source=dict(PowerDensity='exp(-theta^2/0.05)'))
  prs = []
  for K, a2 in ((-0.8, 1e-5), (-1.3, 2e-5), (0.2, -1e-5)):
    doc.Solid.ConicConstant = K
    doc.Solid.Coefficients = [0.0, a2, -2e-8, 3e-11]
    prs.append((bake.bakeScene(doc, src), point_source.bakeSource(doc, src), bake.bakeLimits(doc, src)))
  assert [float(p[0].prim_params[0][1]) for p in prs] == [-0.8, -1.3, 0.2] and [float(p[0].prim_coef[0][1]) for p in prs] == [1e-5, 2e-5, -1e-5]
  n, cap = 4100, 4100 + 1024
  singles = {}
  for mode in MODES:
    with Tracer(0) as tr:
      tr.compileScene(mode)
      singles[mode] = []
      caches = []
      for sc, bs, lim in prs:
        tr.setScene(sc)
        tr.setSource(bs)
        tr.setLimits(lim)
        tr.setDetector(None)
        tr.reserveHits(cap)
        tr.reset()
        tr.trace(0, n, SEED, histogram=False)
        tr.sync()
        info = tr.compiledInfo()
        assert info['mode'] == MODES.index(mode)
        caches.append(info['cache'])
        singles[mode].append(tr.hits())
      tr.setLimits(prs[0][2])
      tr.setSource(prs[0][1])
      if mode == 'off':
        with pytest.raises(_native.NativeError, match='unsupported'):
          tr.setSceneBatch([p[0] for p in prs])
        continue
      assert caches[1] >= 1 and caches[2] >= 1, caches                   # (the image carries K and the coefficients: one compilation)
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
def test_aspheric_lens_under_a_point_source(native_lib):
  """a singlet of make.makeAsphericLens under a point source, 1e5 rays, a detector with a power map: histogram and
  power plane equal between the two modes, rows equal bit for bit, every lens-surface row on its surface"""
  from freecad.optics_design_workbench_amd import scenes
  from freecad.optics_design_workbench_amd.freecad_elements import point_source
  from freecad.optics_design_workbench_amd.scene import bake
  front = dict(vertexRadius=20.0, conicConstant=-0.8, coefficients=(0.0, 1e-5, -2e-8, 3e-11))
  back = dict(curvature=-1.0 / 35.0, conicConstant=0.3, coefficients=(0.0, -4e-6))
  t, dia, z0 = 5.0, 18.0, 30.0
  doc, src = ac.document(
      [('Lens', lambda d: [make.makeAsphericLens(d, 'L', front=front, back=back, thickness=t, diameter=dia, base=(0.0, 0.0, z0))],
        dict(RefractiveIndex=1.5, RecordHits=True)),
       ('Absorber', lambda d: [make.makeBox(d, 'A', 100, 100, 1, base=(-50, -50, 70))], {})],
      source=dict(PowerDensity='exp(-theta^2/0.02)'))
  pr = (bake.bakeScene(doc, src), point_source.bakeSource(doc, src), bake.bakeLimits(doc, src))
  assert sorted(pr[0].prim_type) == [0, 9, 9]
  det = scenes.planeDetector(pr[0], pr[0].group_names[1], nx=32, ny=32, toward=np.zeros(3))
  n = 100000
  got = [_source_launch(pr, mode, n, 3 * n + 4096, det=det, power=True) for mode in MODES]
  _same_rows(got[0], got[1])
  assert np.array_equal(got[0]['hist'], got[1]['hist']) and np.array_equal(got[0]['power'], got[1]['power'])
  assert got[0]['counters']['hits_dropped'] == 0 and got[0]['hist'].sum() > n // 2
  x = got[0]['rows']['point'] - [0.0, 0.0, z0]
  rho = np.hypot(x[:, 0], x[:, 1])
  lens = (x[:, 2] < t + 3.0) & (rho < dia / 2 - 1e-3)
  fs = dict(c=1.0 / 20.0, K=-0.8, coefs=front['coefficients'])
  bs = dict(c=back['curvature'], K=0.3, coefs=back['coefficients'])
  res = np.minimum(ac.residual(x[lens], fs), np.abs(x[lens][:, 2] - t - ac.sag_u(rho[lens]**2, bs['c'], bs['K'], bs['coefs'])))
  print(f'{lens.sum()} rows on the lens surfaces, off them by {res.max():.3e} mm at most')
  assert lens.sum() > n and res.max() <= ac.TOL
