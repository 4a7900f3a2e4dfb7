"""The binary-tree kernel (odw_trace_kernel<true, ...>: nearest<BVH = true> of csrc/odw_kernels.hip) against closed forms
and the CPU oracle (-m gpu), on the cases of tests/grid_cases.py and tests/tree_cases.py (tests/test_tree_cases.py holds
the new ones without a GPU; tests/test_native_bvh_cover.py holds the tables the walk is handed).

Every launch here can only take the tree, which is asserted before it is made: odw_build_check reports nodes, and the
launch records segments or carries a wavelength per ray -- choose_kernel (csrc/odw_capi.hip) sends such launches to the
tree whatever else was built.  Each launch is a context of its own, explicit rays, no detector.

Hit rows are held to the closed form and to the oracle (points within ec.TOL = 1e-9 mm, tags and counters equal), segment
rows to the chain origin -> crossings -> closing segment and to oracle.trace_segments, and the hit rows of a segment
launch to those of the same scene's plain launch (the grid kernel, or the tree again where the scene has no grid).

One exception, by the reference's own arithmetic: on tree_cases.far_back_set the oracle's points are 2.5e-9 / 7.2e-9 mm
off the closed form (see there); the device is held to the closed form within ec.TOL, to the oracle in tags and counters."""
import numpy as np
import pytest

import ellipsoid_cases as ec
import grid_cases as gc
import tree_cases as tc
from grid_cases import held

pytestmark = pytest.mark.gpu

RAY = np.uint64(0xFFFFFFFFFFFF)
COLS = ('tag', 'point', 'direction', 'power')
SEG_COLS = ('tag', 'p1', 'p2', 'power')


def _launch(sc, lim, o, d, segments=True, wavelengths=None, hit_capacity=None, seg_capacity=None, tree=True, structure=None):
  """explicit rays through a tracer of its own -> dict(rows, counters, [segments, segment_count]).  tree: asserted before
  anything is launched -- the scene has tree nodes and the launch records segments or carries wavelengths; structure:
  what odw_build_check has to say of the scene"""
  from freecad.optics_design_workbench_amd import _native
  from freecad.optics_design_workbench_amd.simulation.tracer import Tracer
  info = _native.build_check(sc, lim)
  if structure is not None:
    assert info['structure'] == structure, info
  if tree:
    assert info['nodes'] > 0, info
    assert segments or wavelengths is not None or info['structure'] == 'bvh', info
  rows_per_ray = lim.max_intersections + 1
  with Tracer(0) as tr:
    tr.compileScene('off')
    tr.setScene(sc)
    tr.setLimits(lim)
    tr.setDetector(None)
    tr.reserveHits(hit_capacity if hit_capacity is not None else len(o) * rows_per_ray)
    if segments:
      tr.reserveSegments(seg_capacity if seg_capacity is not None else len(o) * rows_per_ray)
    tr.reset()
    tr.traceRays(o, d, record_segments=segments, wavelengths=wavelengths, histogram=False)
    tr.sync()
    out = dict(rows=tr.hits(), counters=tr.counters())
    if segments:
      out['segments'], out['segment_count'] = tr.segments(), tr.segmentCount()
  return out


def _vacuum_rows(rows, o, d):
  """vacuum bends nothing and takes nothing: every row with the direction its ray started with, unit powers"""
  if not len(rows):
    return
  ray = (rows['tag'] & RAY).astype(np.int64)
  unit = d / np.linalg.norm(d, axis=1)[:, None]
  assert np.abs(rows['direction'] - unit[ray]).max() < 1e-15
  first = np.r_[0, np.nonzero(np.diff(ray))[0] + 1]
  start = first[np.searchsorted(first, np.arange(len(rows)), side='right') - 1]
  assert np.array_equal(rows['direction'], rows['direction'][start])
  assert np.array_equal(rows['power'], np.ones(len(rows)))


def _tree_against_both(oracle, c, o, d, label, expected=gc.expected_for, plain='grid', oracle_points=True):
  """a segment launch (the tree) of the vacuum case c: hit rows against the closed form, the oracle and the plain launch,
  segment rows against the chain and oracle.trace_segments -> the launch"""
  want, excluded = expected(c, o, d)
  limit = float(c.lim.max_ray_length)
  seg = _launch(c.sc, c.lim, o, d)
  rows, cnt = seg['rows'], seg['counters']
  assert cnt['hits_dropped'] == 0 and cnt['traced_rays'] == len(o) and seg['segment_count'] == (len(seg['segments']), 0)
  worst, crossings = held(rows, o, d, want, excluded, f'tree, {label}')
  _vacuum_rows(rows, o, d)
  ref_segs = None
  if c.oracle_knows:
    ref = oracle.trace_rays(c.sc, c.lim, o, d, nthreads=0)
    assert {k: v for k, v in cnt.items() if k != 'segments'} == {k: v for k, v in ref['counters'].items() if k != 'segments'}, (label, cnt, ref['counters'])
    assert np.array_equal(rows['tag'], ref['hits']['tag']), label
    # (points: every row; on the far random sets the rows of the rays tree_cases.ill_conditioned keeps -- the oracle is
    #  the one that cannot hold the others)
    kept = ~excluded[(rows['tag'] & RAY).astype(np.int64)] if expected is tc.far_expected else np.ones(len(rows), bool)
    dev = float(np.abs(rows['point'] - ref['hits']['point'])[kept].max()) if kept.any() else 0.0
    print(f'{label}: tree against the oracle {dev:.3e} mm over {int(kept.sum())} of {len(rows)} rows')
    assert dev < ec.TOL or not oracle_points, label
    got = oracle.trace_segments(c.sc, c.lim, origins=o, dirs=d)
    ref_segs = got['segments']
    assert cnt['segments'] == got['counters']['segments'] == len(seg['segments'])
  else:
    # (the oracle has no ellipsoid: the closed form alone, and the counters it implies)
    assert excluded.sum() == 0
    assert cnt['recorded_hits'] == len(rows) == crossings and cnt['escaped'] == len(o) and cnt['capped'] == cnt['died'] == 0
    assert len(seg['segments']) == crossings + len(o)
  tc.held_segments(seg['segments'], ref_segs, o, d, want, excluded, f'tree, {label}, segments', limit=limit, ref_points=oracle_points,
                   ref_kept_only=expected is tc.far_expected)
  # the same scene's plain launch
  flat = _launch(c.sc, c.lim, o, d, segments=False, tree=False, structure=plain)
  assert np.array_equal(rows['tag'], flat['rows']['tag']), label
  assert {k: v for k, v in cnt.items() if k != 'segments'} == {k: v for k, v in flat['counters'].items() if k != 'segments'}, label
  dev = float(np.abs(rows['point'] - flat['rows']['point']).max()) if len(rows) else 0.0
  print(f'{label}: tree against the plain launch ({plain}) {dev:.3e} mm')
  assert dev < ec.TOL, label
  return seg


# ---- closed forms on the tree ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['lattice', 'mixed'])
def test_aimed_rays(native_lib, oracle, name):
  c = gc.case(name)
  for label, (o, d) in gc.aimed_sets(name).items():
    seg = _tree_against_both(oracle, c, o, d, f'{name} {label}')
    if label.startswith('axis') and name == 'lattice':
      got = ec.per_ray(seg['rows'], o, d)
      assert all(len(got[k]) == 0 for k in np.nonzero(gc.AXIS_GRAZING)[0])           # 2 + 1e-9 beside a row: nothing
    if label == 'length-limit':
      beyond = gc.length_limit()[2]
      ray = (seg['rows']['tag'] & RAY).astype(np.int64)
      assert not beyond[ray].any() and set(ray) == set(np.nonzero(~beyond)[0]) and seg['counters']['escaped'] == len(o)


@pytest.mark.parametrize('name', ['cloud', 'staggered', 'seventy'])
def test_random_lines(native_lib, oracle, name):
  c = gc.case(name)
  _tree_against_both(oracle, c, *gc.random_set(name), f'{name} random lines')


def test_in_plane_inside_and_overlap_starts(native_lib, oracle):
  c = gc.case('staggered')
  _tree_against_both(oracle, c, *gc.in_plane(c.solids), 'staggered in-plane')
  c = gc.case('cloud')
  _tree_against_both(oracle, c, *gc.inside_starts(), 'cloud inside starts')
  _tree_against_both(oracle, c, *gc.overlap_starts(), 'cloud overlap starts')


# ---- far placement and tiny components: the float32 culling -----------------------------------------------------------------------
@pytest.mark.parametrize('name', ['lattice', 'mixed'])
def test_far_placement(native_lib, oracle, name):
  c = tc.far_case(name)
  for label, (o, d) in tc.far_sets(name).items():
    _tree_against_both(oracle, c, o, d, f'far {name} {label}', expected=tc.far_expected if label == 'random' else gc.expected_for)
  back = tc.far_case(name, tc.FAR_LIMIT)
  _tree_against_both(oracle, back, *tc.far_back_set(name), f'far {name} random+1000', expected=tc.far_expected, oracle_points=False)


def test_tiny_components(native_lib, oracle):
  c = tc.far_case('lattice')
  for label, (o, d) in tc.tiny_sets().items():
    seg = _tree_against_both(oracle, c, o, d, label)
    assert len(seg['rows']) == 104 and len(seg['segments']) == 104 + 12


# ---- facets in the binary tree -------------------------------------------------------------------------------------------------------
def test_facets(native_lib, oracle, monkeypatch):
  c = tc.facet_case()
  sets = tc.facet_sets()
  mesh = {label: _launch(c.sc, c.lim, o, d, segments=False, tree=False, structure='wide-bvh') for label, (o, d) in sets.items()}
  monkeypatch.setenv('ODW_MESH_KERNEL', '0')
  for label, (o, d) in sets.items():
    seg = _tree_against_both(oracle, c, o, d, f'facets {label}', plain='bvh')
    # the plain launch under ODW_MESH_KERNEL=0 is the binary tree too: the rows of the segment launch, and those of the
    # mesh kernel (the variable unset), bit for bit
    plain = _launch(c.sc, c.lim, o, d, segments=False, structure='bvh')
    for col in COLS:
      assert np.array_equal(plain['rows'][col], seg['rows'][col]), (label, col)
      assert np.array_equal(plain['rows'][col], mesh[label]['rows'][col]), (label, col)
    assert plain['counters'] == mesh[label]['counters']
    if label == 'face diagonals':
      p = tc.face_diagonals()[2]
      got = ec.per_ray(seg['rows'], o, d)
      assert all((np.abs(g - p[k]).max(1) < ec.TOL).sum() == 1 for k, g in enumerate(got))      # one crossing on the shared edge


# ---- the CHROMA instantiation ---------------------------------------------------------------------------------------------------------
def test_chroma_instantiation(native_lib):
  """a wavelength per ray, no compiled kernel: odw_trace_chroma_kernel walks the tree.  The scenes have no dispersion: the rows
  of the segment launch as bytes, and the closed form"""
  sets = [(gc.case('lattice'), f'lattice {label}', o, d, gc.expected_for) for label, (o, d) in gc.aimed_sets('lattice').items()]
  sets.append((tc.far_case('lattice'), 'far lattice random', *tc.far_sets('lattice')['random'], tc.far_expected))
  for c, label, o, d, expected in sets:
    wl = 400.0 + 300.0 * ((np.arange(len(o)) * 37) % 101) / 101.0
    seg = _launch(c.sc, c.lim, o, d)
    chroma = _launch(c.sc, c.lim, o, d, segments=False, wavelengths=wl)
    for col in COLS:
      assert chroma['rows'][col].tobytes() == seg['rows'][col].tobytes(), (label, col)
    assert {k: v for k, v in chroma['counters'].items() if k != 'segments'} == {k: v for k, v in seg['counters'].items() if k != 'segments'}
    held(chroma['rows'], o, d, *expected(c, o, d), f'chroma, {label}')


# ---- launch sizes ------------------------------------------------------------------------------------------------------------------------
def test_launch_sizes(native_lib):
  c = gc.case('lattice')
  o, d = ec.random_lines(1025, seed=13, span=25.0)
  o = o + np.array([20.0, 15.0, 15.0])
  full = _launch(c.sc, c.lim, o, d)
  assert len(full['rows']) > 500 and full['counters']['traced_rays'] == 1025
  ray = (full['rows']['tag'] & RAY).astype(np.int64)
  seg_ray = tc.seg_fields(full['segments'])[0]
  assert len(full['segments']) == len(full['rows']) + 1025
  for n in (1, 63, 64, 65):
    part = _launch(c.sc, c.lim, o[:n], d[:n])
    cnt = part['counters']
    assert cnt['traced_rays'] == n and cnt['recorded_hits'] == len(part['rows']) == (ray < n).sum()
    for col in COLS:
      assert np.array_equal(part['rows'][col], full['rows'][col][ray < n]), (n, col)
    assert part['segment_count'] == ((seg_ray < n).sum(), 0)
    for col in SEG_COLS:
      assert np.array_equal(part['segments'][col], full['segments'][col][seg_ray < n]), (n, col)


# ---- the tree's own interaction code ---------------------------------------------------------------------------------------------------
def _same(a, b, label):
  (ra, ca), (rb, cb) = a, b
  ca, cb = ({k: v for k, v in c.items() if k != 'segments'} for c in (ca, cb))
  assert ca == cb, (label, ca, cb)
  assert np.array_equal(ra['tag'], rb['tag']), label
  figures = (float(np.abs(ra['point'] - rb['point']).max()), float(np.abs(ra['power'] - rb['power']).max()))
  print(f'{label}: points %.3e mm, powers %.3e over {len(ra)} rows' % figures)
  assert figures[0] < ec.TOL and figures[1] < ec.POWER_TOL


@pytest.mark.parametrize('variant', ['capped', 'power-limit', 'sequential'])
def test_interactions(native_lib, oracle, monkeypatch, variant):
  """the bench of grid_cases through the tree (ODW_BVH_THRESHOLD=4 when the context is made, segment rows) against the oracle
  and against the flat kernel of a context made without it; the variants of test_gpu_grid.py::test_interactions.
  sequential: the per-lane `mask` test of the leaf loop"""
  sc, lim = gc.bench_variant(*gc.bench(), variant)
  o, d, station = gc.bench_rays()
  flat = _launch(sc, lim, o, d, segments=False, tree=False, structure='flat')
  monkeypatch.setenv('ODW_BVH_THRESHOLD', '4')
  tree = _launch(sc, lim, o, d, structure='grid')
  ref = oracle.trace_rays(sc, lim, o, d, nthreads=0)
  _same((tree['rows'], tree['counters']), (ref['hits'], ref['counters']), f'{variant}: tree against the oracle')
  _same((tree['rows'], tree['counters']), (flat['rows'], flat['counters']), f'{variant}: tree against the flat kernel')
  want = oracle.trace_segments(sc, lim, origins=o, dirs=d)
  got = tree['segments']
  assert tree['segment_count'] == (len(want['segments']), 0) and tree['counters']['segments'] == want['counters']['segments']
  assert np.array_equal(got['tag'], want['segments']['tag'])
  figures = (float(np.abs(got['p1'] - want['segments']['p1']).max()), float(np.abs(got['p2'] - want['segments']['p2']).max()),
             float(np.abs(got['power'] - want['segments']['power']).max()))
  print(f'{variant}: segments against the oracle: p1 %.3e mm, p2 %.3e mm, powers %.3e over {len(got)} rows' % figures)
  assert figures[0] < ec.TOL and figures[1] < ec.TOL and figures[2] < ec.POWER_TOL
  gc.bench_figures(tree['rows'], tree['counters'], station, variant)


# ---- lists that are too small: the designed overflow --------------------------------------------------------------------------------
def test_lists_too_small(native_lib):
  c = gc.case('lattice')
  o, d = gc.random_set('lattice')
  want, excluded = gc.expected_for(c, o, d)
  total = sum(len(w) for w in want)
  full = _launch(c.sc, c.lim, o, d)
  assert excluded.sum() == 0 and len(full['rows']) == total and len(full['segments']) == total + len(o)
  # a hit list a third of what the launch records
  small = _launch(c.sc, c.lim, o, d, hit_capacity=total // 3)
  rows, cnt = small['rows'], small['counters']
  assert cnt['recorded_hits'] == total and cnt['hits_dropped'] > 0
  assert 0 < len(rows) <= total // 3 and len(rows) + cnt['hits_dropped'] == cnt['recorded_hits']
  assert small['segment_count'] == (total + len(o), 0)
  ray = (rows['tag'] & RAY).astype(np.int64)
  worst = 0.0
  for k in np.unique(ray):
    p = rows['point'][ray == k]
    assert len(p) <= len(want[k])
    worst = max(worst, float(np.abs(p[:, None, :] - want[k][None, :, :]).max(-1).min(-1).max()))
  print(f'hit list of {total // 3} for {total} rows: {len(rows)} stored, worst {worst:.3e} mm')
  assert worst < ec.TOL
  # a segment list a third of the segments
  n_seg = total + len(o)
  capacity = n_seg // 3
  small = _launch(c.sc, c.lim, o, d, seg_capacity=capacity)
  assert small['segment_count'] == (capacity, n_seg - capacity) and len(small['segments']) == capacity
  assert small['counters']['hits_dropped'] == 0 and len(small['rows']) == total
  keys = {(int(t), *map(float, a), *map(float, b)) for t, a, b in zip(full['segments']['tag'], full['segments']['p1'], full['segments']['p2'])}
  stored = small['segments']
  assert all((int(t), *map(float, a), *map(float, b)) in keys for t, a, b in zip(stored['tag'], stored['p1'], stored['p2']))
