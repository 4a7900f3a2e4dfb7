"""Part::Torus, Part::Cone, Part::Cylinder and the paraboloid on the device, held to the exact line crossings of
tests/revolution_cases.py (long double; tests/test_revolution_cases.py holds that reference to mpmath and the CPU oracle
to the reference) and to the oracle, through every route: the generic flat kernel, the kernel compiled against the scene,
the binary tree (segment rows) and the grid kernel.

Per set and route: rows per ray, entering bits and the counters a Vacuum group implies equal to the reference's on every
line that is not excluded; points of slope >= 1e-3 within 1e-9 mm; on grazing crossings (distance from the reference
point) x slope within ten times the oracle's worst on the same set, measured in the same test; tags and counters equal
to the oracle's.  Compiled rows equal generic rows and the hit rows of a segment launch equal the plain launch's, bit for
bit.  Every test prints what it measured."""
import numpy as np
import pytest

import revolution_cases as rc

pytestmark = pytest.mark.gpu

COLS = ('tag', 'point', 'direction', 'power')


def _tracer(mode):
  from freecad.optics_design_workbench_amd.simulation.tracer import Tracer
  tr = Tracer(0)
  tr.compileScene(mode)
  return tr


def _run(tr, sc, lim, o, d, segments=False, rows_per_ray=8):
  tr.setScene(sc)
  tr.setLimits(lim)
  tr.setDetector(None)
  tr.reserveHits(len(o) * rows_per_ray)
  if segments:
    tr.reserveSegments(len(o) * rows_per_ray)
  tr.reset()
  tr.traceRays(o, d, record_segments=segments, histogram=False)
  tr.sync()
  out = dict(rows=tr.hits(), counters=tr.counters(), info=tr.compiledInfo())
  assert out['counters']['hits_dropped'] == 0
  return out


def _same(a, b, label, wrong):
  """bit for bit (the counter of nearest-hit queries aside where one launch records segments)"""
  ca, cb = ({k: v for k, v in x['counters'].items() if k != 'segments'} for x in (a, b))
  if ca != cb or len(a['rows']) != len(b['rows']):
    wrong.append(f'{label}: counters {ca} against {cb}')
    return False
  for col in COLS:
    if not np.array_equal(a['rows'][col], b['rows'][col]):
      diff = np.abs(a['rows']['point'] - b['rows']['point']).max() if col == 'point' else None
      wrong.append(f'{label}: column {col} differs (points by {diff})')
      return False
  return True


def _against_oracle(dev, ref, want, label, wrong):
  """tags of the lines that are not excluded and, where none is, the counters; the distance between the two is printed"""
  n = len(want.points)
  keep = lambda rows: rows[~want.excluded[(rows['tag'] & rc.RAY).astype(np.int64)]]
  a, b = keep(dev['rows']), keep(ref['hits'])
  if not np.array_equal(a['tag'], b['tag']):
    wrong.append(f'{label}: tags differ from the oracle\'s ({len(a)} rows against {len(b)})')
    return
  if not want.excluded.any() and dev['counters'] != ref['counters']:
    wrong.append(f'{label}: counters {dev["counters"]} against the oracle\'s {ref["counters"]}')
  print(f'{label}: device against the oracle {float(np.abs(a["point"] - b["point"]).max()) if len(a) else 0.0:.3e} mm over {len(a)} rows')


def _routes(oracle, trs, sc, lim, o, d, want, label, cap, wrong, rows_per_ray=8, edge_of=None):
  """one set through the generic launch, the compiled one and the segment launch of the tracers trs = (off, structure)"""
  ref = oracle.trace_rays(sc, lim, o, d, nthreads=0)
  _, oracle_product = rc.held(ref['hits'], ref['counters'], want, f'oracle, {label}', cap=cap, soft=wrong)
  off = _run(trs[0], sc, lim, o, d, rows_per_ray=rows_per_ray)
  spec = _run(trs[1], sc, lim, o, d, rows_per_ray=rows_per_ray)
  seg = _run(trs[0], sc, lim, o, d, segments=True, rows_per_ray=rows_per_ray)
  assert off['info']['mode'] == 0 and spec['info']['mode'] == 1, (off['info'], spec['info'])
  assert len(trs[0].segments()) == len(seg['rows']) + len(o)            # (one segment up to every row, one beyond the last)
  launches = [('generic', off)]
  # route against route: where a pair is not equal bit for bit, each is held to the reference on its own
  if not _same(off, spec, f'{label}: compiled against generic', wrong):
    launches.append(('compiled', spec))
  if not _same(off, seg, f'{label}: segment launch against plain', wrong):
    launches.append(('tree', seg))
  for route, out in launches:
    rc.held(out['rows'], out['counters'], want, f'{route}, {label}', grazing_bound=10.0 * oracle_product, cap=cap, soft=wrong)
    _against_oracle(out, ref, want, f'{route}, {label}', wrong)
    if edge_of is not None and len(out['rows']):
      far = rc.cylinder_boundary_distance(edge_of(out['rows']['point']), *rc.SOLIDS['cylinder'].par).max()
      per = np.bincount((out['rows']['tag'] & rc.RAY).astype(np.int64), minlength=len(o))
      print(f'{route}, {label}: recorded points up to {far:.3e} mm from the surface, at most {per.max()} rows per line')
      if far > 2.0 * rc.DIST_TOL or per.max() > 2:
        wrong.append(f'{route}, {label}: a point {far:.3e} mm from the surface, {per.max()} rows on a line')
  return off


def _structure(sc, lim):
  from freecad.optics_design_workbench_amd import _native
  return _native.build_check(sc, lim)['structure']


@pytest.mark.parametrize('placement', ['origin', 'moved'])
@pytest.mark.parametrize('name', list(rc.SOLIDS))
def test_solid_alone(native_lib, oracle, name, placement):
  """every set of the solid through the generic flat kernel (a paraboloid: the grid kernel, the flat generic kernel does
  not know it), the compiled kernel and the tree; launches of 1, 63, 64 and 65 lines give the first rows of the full one.
  On `margin-edge` (lines into a cylinder's cap within 3e-6 mm of the rim, across the margin of the side's skip: all of
  them in the excluded class) every recorded point lies within 2e-6 mm of the surface, two rows per line at most"""
  s = rc.SOLIDS[name]
  sc0, lim0 = rc.scene(name, placement)
  assert _structure(sc0, lim0) == ('grid' if s.kind == 'paraboloid' else 'flat')
  wrong = []
  P = rc.ec.Placement(**rc.PLACEMENTS[placement]) if rc.PLACEMENTS[placement] else None
  back = (lambda x: np.array([P.inverse() * p for p in x])) if P else (lambda x: x)
  trs = (_tracer('off'), _tracer('structure'))
  try:
    for label in rc.line_sets(name):
      o, d, limit, want = rc.world(name, label, placement)
      sc, lim = rc.scene(name, placement, limit)
      full = _routes(oracle, trs, sc, lim, o, d, want, f'{name} {placement} {label}', rc.cap_of(label), wrong,
                     edge_of=back if label in rc.EDGE_SETS else None)
      if label == 'random':
        ray = (full['rows']['tag'] & rc.RAY).astype(np.int64)
        for tr in trs:
          for n in (1, 63, 64, 65):
            part = _run(tr, sc, lim, o[:n], d[:n])
            for col in COLS:
              assert np.array_equal(part['rows'][col], full['rows'][col][ray < n]), (name, n, col)
  finally:
    for tr in trs:
      tr.close()
  assert not wrong, wrong


@pytest.mark.parametrize('name', list(rc.SOLIDS))
def test_solid_far_away(native_lib, oracle, name):
  """the random set with the solid at (3000, -7000, 11000) mm, rotated: the reference in the unmoved frame, mapped"""
  o, d, limit, want = rc.world(name, 'random', 'far')
  sc, lim = rc.scene(name, 'far', limit)
  wrong = []
  trs = (_tracer('off'), _tracer('structure'))
  try:
    _routes(oracle, trs, sc, lim, o, d, want, f'{name} far random', 0.01, wrong)
  finally:
    for tr in trs:
      tr.close()
  assert not wrong, wrong


@pytest.mark.parametrize('paraboloid, grid', [(True, False), (False, False), (False, True)], ids=['with-paraboloid', 'without', 'without-grid'])
def test_gallery(native_lib, oracle, monkeypatch, paraboloid, grid):
  """all solids side by side, with the paraboloid (the generic launch takes the grid kernel) and without (ten primitives:
  the generic flat kernel, whose instantiation without the paraboloid has the cylinder's skip; under ODW_BVH_THRESHOLD = 4
  the grid kernel): random lines over the gallery and every solid's constructed sets where it stands"""
  if grid:
    monkeypatch.setenv('ODW_BVH_THRESHOLD', '4')          # (read when the context is created, and by build_check)
  (sc, lim), names = rc.gallery(paraboloid)
  assert _structure(sc, lim) == ('grid' if paraboloid or grid else 'flat')
  wrong = []
  trs = (_tracer('off'), _tracer('structure'))
  try:
    for label, (o, d, limit) in rc.gallery_sets(paraboloid).items():
      want = rc.gallery_expected(label, paraboloid)
      _routes(oracle, trs, sc, lim, o, d, want, f'gallery {label}', 0.01, wrong, rows_per_ray=24)
  finally:
    for tr in trs:
      tr.close()
  assert not wrong, wrong


def test_spindle_torus_is_its_outer_sheet(native_lib):
  """Part::Torus (10, 12) passes the bake; the march of the distance function sees the boundary of the revolved disc,
  the outer sheet: a line in the equatorial plane through the centre crosses at x = -+ 22, the axis at z = -+ sqrt(44).
  (The oracle's quartic records the inner sheet as well and nothing on the axis: DESIGN.md section 3)"""
  sc, lim = rc.ec.vacuum(lambda d: [rc.make.makeTorus(d, 'T', 10.0, 12.0)])
  o, d = np.array([[-40.0, 0.0, 0.0], [0.0, 0.0, -40.0]]), np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
  want = [np.array([[-22.0, 0, 0], [22.0, 0, 0]]), np.array([[0, 0, -np.sqrt(44.0)], [0, 0, np.sqrt(44.0)]])]
  for mode in ('off', 'structure'):
    tr = _tracer(mode)
    try:
      got = rc.per_ray(_run(tr, sc, lim, o, d)['rows'], 2)
    finally:
      tr.close()
    print(mode, [g[0].tolist() for g in got])
    for (p, ent), w in zip(got, want):
      assert len(p) == 2 and np.abs(p - w).max() < rc.TOL, (mode, p, w)
    assert got[0][1].tolist() == [True, False]          # (on the axis the tube's normal has no direction: the bits there mean nothing)
