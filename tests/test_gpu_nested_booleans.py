"""Nested booleans on the device (-m gpu): every kernel on the native clause lists (cond_inside bit 1) against the
oracle on the per-clause expansion (tests/nested_booleans.py) -- identical counters, identical tags (ray | group |
isEntering: no primitive index), coordinates within 1e-9 mm -- on the generic flat kernel and the scene-compiled one,
the grid kernel, the mesh kernel and a seeded fuzz of random nested trees; a batch launch over the bore radius of a
bored, fused mount against single launches; a surface source on a nested solid; the new validation of the cond
words.  (The closed forms of tests/test_nested_booleans.py run here too, through its `backend` fixture.)"""
import copy

import numpy as np
import pytest

from csg_reference import groupSolids
from nested_booleans import expand, mount, n_clauses, nested_scene
from random_scenes import rays
from test_bake_independent import sdist
from test_nested_booleans import _mount_scene
from test_surface_source import _source

from freecad.optics_design_workbench_amd import _native, scenes
from freecad.optics_design_workbench_amd.freecad_elements import make, surface_source
from freecad.optics_design_workbench_amd.scene import Document

pytestmark = pytest.mark.gpu


def _device(tr, sc, lim, o, d):
  tr.setScene(sc); tr.setLimits(lim); tr.setDetector(None)
  tr.reserveHits(len(o) * (lim.max_intersections + 1))
  tr.reset()
  tr.traceRays(o, d)
  tr.sync()
  return tr.hits(), tr.counters()


def _compare(g, gc, r, n, exact=True):
  """-> number of rays whose hit sequences differ (exact: none may, and the counters agree); coordinates: first hits
  within 1e-9 mm, the whole rows as well where the rays go straight on (exact), else within the first four hits
  1e-7 (rounding amplified by every bounce off a curved surface, as in tests/test_gpu_fuzz.py)"""
  rr, cc = r['hits'], r['counters']
  gr = (g['tag'] & np.uint64(0xFFFFFFFFFFFF)).astype(np.int64)
  if len(g) != len(rr) or not np.array_equal(g['tag'], rr['tag']):
    assert not exact, (len(g), len(rr))
    rk = (rr['tag'] & np.uint64(0xFFFFFFFFFFFF)).astype(np.int64)
    return int((np.bincount(gr, minlength=n) != np.bincount(rk, minlength=n)).sum())
  if exact:
    assert {k: gc[k] for k in cc} == dict(cc), (gc, cc)
  if not len(g):
    return 0
  dev = np.abs(g['point'] - rr['point']).max(axis=1)
  first = np.r_[True, gr[1:] != gr[:-1]]
  assert dev[first].max() < 1e-9, float(dev[first].max())
  if exact:
    assert dev.max() < 1e-9, float(dev.max())
  else:
    start = np.maximum.accumulate(np.where(first, np.arange(len(gr)), 0))
    assert dev[np.arange(len(gr)) - start < 4].max() < 1e-7
  return 0


def _mount_rays(rs, n, z0=0.0):
  """rays from below the mounts, spread over them"""
  o = np.column_stack([rs.uniform(-16, 16, n), rs.uniform(-6, 24, n), np.full(n, z0)])
  t = np.column_stack([rs.uniform(-16, 16, n), rs.uniform(-6, 24, n), np.full(n, 60.0)])
  d = t - o
  return o, d / np.linalg.norm(d, axis=1)[:, None]


@pytest.mark.parametrize('compile', ['off', 'structure'])
def test_flat_kernels(native_lib, oracle, compile):
  """one mount (bored tube + flange) and a detector, and random nested trees in Vacuum groups: straight lines, every
  row within 1e-9 mm"""
  from freecad.optics_design_workbench_amd.simulation.tracer import Tracer
  rs = np.random.RandomState(5)
  cases = [_mount_scene(2.5, kind='Vacuum')[1:] + (None,)]
  for s in range(3):
    sc, lim, targets, _ = nested_scene(np.random.RandomState(7300 + s), optical=False, dist_tol='1e-6')
    cases.append((sc, lim, targets))
  with Tracer(0) as tr:
    tr.compileScene(compile)
    for sc, lim, targets in cases:
      assert max(n_clauses(sc)) > 1
      assert _native.build_check(sc, lim)['structure'] == 'flat'
      o, d = _mount_rays(rs, 20000) if targets is None else rays(rs, targets, 20000)
      g, gc = _device(tr, sc, lim, o, d)
      assert tr.compiledInfo()['mode'] == (1 if compile == 'structure' else 0)
      r = oracle.trace_rays(expand(sc), lim, o, d, nthreads=0)
      assert len(r['hits']) > 2000
      _compare(g, gc, r, len(o))


@pytest.mark.parametrize('how', ['many-primitives', 'threshold'])
def test_grid_kernel(native_lib, oracle, monkeypatch, how):
  """22 placed mounts (67 primitives: the grid kernel), and six (19) with the grid kernel forced from 16 primitives
  on (ODW_BVH_THRESHOLD, read when the context is created)"""
  from freecad.optics_design_workbench_amd.simulation.tracer import Tracer
  if how == 'threshold':
    monkeypatch.setenv('ODW_BVH_THRESHOLD', '16')
  doc, sc, lim = _mount_scene(2.5, copies=22 if how == 'many-primitives' else 6, kind='Vacuum')
  assert sc.n_prims > 16 and _native.build_check(sc, lim)['structure'] == 'grid'
  o, d = _mount_rays(np.random.RandomState(11), 20000)
  with Tracer(0) as tr:
    g, gc = _device(tr, sc, lim, o, d)
  r = oracle.trace_rays(expand(sc), lim, o, d, nthreads=0)
  assert len(r['hits']) > 2000
  _compare(g, gc, r, len(o))


def test_mesh_kernel(native_lib, oracle):
  """a mount behind a tessellated ball lens (the mesh kernel: facets and analytic primitives in one tree)"""
  from freecad.optics_design_workbench_amd.simulation.tracer import Tracer
  doc, sc, lim = _mount_scene(2.5, lens=True, kind='Vacuum')
  assert _native.build_check(sc, lim)['structure'] == 'wide-bvh'
  o, d = _mount_rays(np.random.RandomState(12), 20000)
  with Tracer(0) as tr:
    g, gc = _device(tr, sc, lim, o, d)
  r = oracle.trace_rays(expand(sc), lim, o, d, nthreads=0)
  assert len(r['hits']) > 2000
  assert _compare(g, gc, r, len(o), exact=False) <= 2


def test_random_nested_scenes(native_lib, oracle):
  """20 random nested scenes (the four patterns, depth 2 - 3, off-axis placements, random optical types) x 2e4 rays,
  the first four with the scene-compiled kernel"""
  from freecad.optics_design_workbench_amd.simulation.tracer import Tracer
  n = 20000
  scenes_done = differing = 0
  with Tracer(0) as tr:
    for s in range(20):
      rs = np.random.RandomState(8800 + s)
      sc, lim, targets, _ = nested_scene(rs)
      tr.compileScene('structure' if s < 4 else 'off')
      o, d = rays(rs, targets, n)
      g, gc = _device(tr, sc, lim, o, d)
      r = oracle.trace_rays(expand(sc), lim, o, d, nthreads=0)
      differing += _compare(g, gc, r, n, exact=False)
      scenes_done += max(n_clauses(sc)) > 1
  assert scenes_done >= 16 and differing <= 2, (scenes_done, differing)


def test_batch_over_the_bore_radius(native_lib):
  """a sweep of the bore radius is one structure (same trimming lists, clause marks included): one batch launch,
  every scene's rows bit for bit those of its own launch"""
  from freecad.optics_design_workbench_amd.simulation.tracer import Tracer
  projects = []
  for bore in (1.8, 2.5, 3.3):
    doc, sc, lim = _mount_scene(bore)
    projects.append(scenes.bakeProject(doc))
  assert max(n_clauses(projects[0].scene)) > 1
  m, seed = 20000, 77
  with Tracer(0) as tr:
    tr.compileScene('structure')
    tr.setLimits(projects[0].limits)
    tr.setSource(projects[0].source)
    tr.setSceneBatch([p.scene for p in projects])
    tr.reset()
    tr.traceBatch(0, m, seed, 2 * m)
    tr.sync()
    assert tr.counters()['traced_rays'] == 3 * m
    got = []
    for k in range(len(projects)):
      tr.batchSelect(k)
      got.append(tr.hits())
    tr.batchSelect(None)
  with Tracer(0) as tr:
    tr.compileScene('structure')
    for p, g in zip(projects, got):
      tr.setScene(p.scene); tr.setSource(p.source); tr.setLimits(p.limits); tr.setDetector(None)
      tr.reserveHits(2 * m)
      tr.reset()
      tr.trace(0, m, seed)
      tr.sync()
      one = tr.hits()
      assert len(one) > 1000
      for col in ('point', 'direction', 'power', 'tag'):
        assert np.array_equal(one[col], g[col]), col
  # (the bore changes the rows: three different scenes)
  assert len(got[0]) != len(got[2]) or not np.array_equal(got[0]['point'], got[2]['point'])


def test_surface_source_on_a_nested_solid(native_lib):
  """every emitted origin is on the true boundary (membership flips within +-1e-5 mm along the ray): none on the parts
  of the tube's and flange's faces that the fuse and the bore trim away"""
  from freecad.optics_design_workbench_amd.simulation.tracer import Tracer
  doc = Document()
  part = mount(doc, 2.5, base=(1.0, -2.0, 3.0))
  make.makeOpticalGroup(doc, 'Absorber', [part], name='G')
  solid, = groupSolids(doc)['G']
  s = surface_source.bakeSurfaceSource(doc, _source(doc, [(part, [])], ThetaDomain='0, 0.2'))
  assert (np.asarray(s.cond_inside) & 2).any()
  n = 40000
  with Tracer(0) as tr:
    tr.setSource(s)
    o, d = tr.generateRays(0, n, 1234)
  # (judged away from edges: MARGIN back along the ray every primitive's surface is at least MARGIN / 2 away)
  margin = 1e-3
  near = np.zeros(n, dtype=bool)
  for p in range(len(s.prim_type)):
    m = np.linalg.inv(s.prim_to_world[p].m)
    x = o - margin * d
    near |= np.abs(sdist(int(s.prim_type[p]), s.prim_params[p], x @ m[:3, :3].T + m[:3, 3])) < margin / 2
  judge = ~near
  assert judge.sum() > 0.8 * n
  inner, outer = solid.inside(o - 1e-5 * d), solid.inside(o + 1e-5 * d)
  bad = judge & ~(inner & ~outer)
  assert not bad.any(), (int(bad.sum()), o[bad][:3].tolist())
  # the bore's wall emits (kept inside the tube OR the flange)
  rho = np.hypot(o[:, 0] - 1.4, o[:, 1] + 2.3)
  assert (np.abs(rho - 2.5) < 1e-9).sum() > 0.02 * n


def test_cond_words_are_validated(native_lib):
  from freecad.optics_design_workbench_amd.simulation.tracer import Tracer
  doc, sc, lim = _mount_scene(2.5)
  with Tracer(0) as tr:
    tr.setScene(sc)                                     # (0 .. 3: accepted)
    bad = copy.copy(sc)
    bad.cond_inside = np.asarray(sc.cond_inside).copy()
    bad.cond_inside[0] = 4
    with pytest.raises(_native.NativeError, match='invalid'):
      tr.setScene(bad)
    # a list of several clauses whose first condition does not open one
    p = next(p for p, k in enumerate(n_clauses(sc)) if k > 1)
    bad.cond_inside = np.asarray(sc.cond_inside).copy()
    bad.cond_inside[int(sc.prim_cond_off[p])] &= 1
    with pytest.raises(_native.NativeError, match='invalid'):
      tr.setScene(bad)
