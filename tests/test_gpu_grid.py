"""The grid kernel (csrc/odw_grid.hip) against closed forms and the CPU oracle (-m gpu), on the cases of tests/grid_cases.py
(tests/test_grid_cases.py holds the cases themselves without a GPU): sphere clouds with several records per cell and spheres
listed in several cells, cell and item tables in global memory, rays with zero direction components, in the planes of
the grid, along the lines and through the points where planes meet, rays that start outside, on the boundary, inside solids
and beyond the length limit, partly filled rings, generated rays, the kernel's own interaction code, a hit list that is
too small.

Which instantiation a test launches follows from odw_build_check (`spheres`: every primitive an untrimmed sphere; the
tables' place: grid_cases.tables_in_lds) and is asserted where the test counts on it:
  SPHERES, LDS       lattice, cloud, staggered            SPHERES, global    big (13^3)
  items, LDS         mixed, the bench                     items, global      seventy"""
import copy
import dataclasses

import numpy as np
import pytest

import ellipsoid_cases as ec
import grid_cases as gc
from grid_cases import held

pytestmark = pytest.mark.gpu

RAY = np.uint64(0xFFFFFFFFFFFF)
COLS = ('tag', 'point', 'direction', 'power')


def _launch(sc, lim, o, d, capacity=None, expect=None):
  """explicit rays through a tracer of its own -> (rows, counters); expect: ('grid', spheres, in LDS) of odw_build_check,
  asserted before anything is launched"""
  from freecad.optics_design_workbench_amd import _native
  from freecad.optics_design_workbench_amd.simulation.tracer import Tracer
  if expect is not None:
    info = _native.build_check(sc, lim)
    assert info['structure'] == expect[0], info
    if expect[0] == 'grid':
      assert gc.tables_in_lds(info) == expect[2], info
  with Tracer(0) as tr:
    tr.setScene(sc)
    tr.setLimits(lim)
    tr.setDetector(None)
    tr.reserveHits(capacity if capacity is not None else len(o) * (lim.max_intersections + 1))
    tr.reset()
    tr.traceRays(o, d)
    tr.sync()
    return tr.hits(), tr.counters()


def _case_launch(c, o, d):
  from freecad.optics_design_workbench_amd import _native
  if c.in_lds:
    assert gc.sphere_records(_native.build_check(c.sc, c.lim)) == c.spheres
  return _launch(c.sc, c.lim, o, d, expect=('grid', c.spheres, c.in_lds))


def _against_both(oracle, c, o, d, label, by_name=()):
  """device rows against the closed form and against the oracle's rows: counters and tags equal, points within 1e-9 mm of
  both, every row of a ray with the direction it started with, bit for bit"""
  want, excluded = gc.expected_for(c, o, d)
  rows, cnt = _case_launch(c, o, d)
  assert cnt['hits_dropped'] == 0 and cnt['traced_rays'] == len(o)
  worst, crossings = held(rows, o, d, want, excluded, f'device, {label}', by_name)
  ray = (rows['tag'] & RAY).astype(np.int64)
  if len(rows):
    first = np.r_[0, np.nonzero(np.diff(ray))[0] + 1]
    start = first[np.searchsorted(first, np.arange(len(rows)), side='right') - 1]
    assert np.array_equal(rows['direction'], rows['direction'][start])                  # vacuum bends nothing
    unit = d / np.linalg.norm(d, axis=1)[:, None]
    assert np.abs(rows['direction'] - unit[ray]).max() < 1e-15
    assert np.array_equal(rows['power'], np.ones(len(rows)))
  if c.oracle_knows:
    ref = oracle.trace_rays(c.sc, c.lim, o, d, nthreads=0)
    assert cnt == ref['counters'], (label, cnt, ref['counters'])
    assert np.array_equal(rows['tag'], ref['hits']['tag']), label
    dev = float(np.abs(rows['point'] - ref['hits']['point']).max()) if len(rows) else 0.0
    print(f'{label}: device against the oracle {dev:.3e} mm over {len(rows)} rows')
    assert dev < ec.TOL
  else:
    # (the oracle has no ellipsoid: the closed form alone, and the counters it implies)
    assert excluded.sum() == 0
    assert cnt['recorded_hits'] == len(rows) == crossings and cnt['escaped'] == len(o) and cnt['capped'] == cnt['died'] == 0
  return rows, cnt


# ---- aimed rays on the two lattices (SPHERES / items, tables in LDS) -------------------------------------------------------
@pytest.mark.parametrize('name', ['lattice', 'mixed'])
def test_aimed_rays(native_lib, oracle, name):
  c = gc.case(name)
  for label, (o, d) in gc.aimed_sets(name).items():
    rows, cnt = _against_both(oracle, c, o, d, f'{name} {label}')
    if label.startswith('axis') and name == 'lattice':
      got = ec.per_ray(rows, o, d)
      assert all(len(got[k]) == 0 for k in np.nonzero(gc.AXIS_GRAZING)[0])           # 2 + 1e-9 beside a row: nothing
    if label == 'length-limit':
      beyond = gc.length_limit()[2]
      ray = (rows['tag'] & RAY).astype(np.int64)
      assert not beyond[ray].any() and set(ray) == set(np.nonzero(~beyond)[0]) and cnt['escaped'] == len(o)


def test_rays_in_the_planes_of_the_staggered_scene(native_lib, oracle):
  c = gc.case('staggered')
  o, d = gc.in_plane(c.solids)
  _against_both(oracle, c, o, d, 'staggered in-plane')


# ---- random lines: several records per cell, spheres listed in several cells, tables in global memory ---------------------
@pytest.mark.parametrize('name', ['cloud', 'staggered', 'big', 'seventy'])
def test_random_lines(native_lib, oracle, name):
  from freecad.optics_design_workbench_amd import _native
  c = gc.case(name)
  if name in ('big', 'seventy'):
    info = _native.build_check(c.sc, c.lim)
    assert info['structure'] == 'grid' and not gc.tables_in_lds(info), info       # otherwise this tests nothing new
    assert c.spheres == (name == 'big')
  o, d = gc.random_set(name)
  _against_both(oracle, c, o, d, f'{name} random lines')


def test_rays_started_inside_the_cloud(native_lib, oracle):
  c = gc.case('cloud')
  _against_both(oracle, c, *gc.inside_starts(), 'cloud inside starts')
  _against_both(oracle, c, *gc.overlap_starts(), 'cloud overlap starts')


# ---- launch sizes: a ring filled partly, exactly, across chunks ---------------------------------------------------------------
def test_launch_sizes(native_lib):
  c = gc.case('lattice')
  o, d = ec.random_lines(1025, seed=13, span=25.0)
  o = o + np.array([20.0, 15.0, 15.0])
  full, cnt = _case_launch(c, o, d)
  assert len(full) > 500 and cnt['traced_rays'] == 1025
  ray = (full['tag'] & RAY).astype(np.int64)
  for n in (1, 63, 64, 65):
    rows, cnt = _case_launch(c, o[:n], d[:n])
    assert cnt['traced_rays'] == n and cnt['recorded_hits'] == len(rows) == (ray < n).sum()
    for col in COLS:
      assert np.array_equal(rows[col], full[col][ray < n]), (n, col)


# ---- generated rays --------------------------------------------------------------------------------------------------------
def test_generated_rays(native_lib, oracle):
  from freecad.optics_design_workbench_amd import _native
  from freecad.optics_design_workbench_amd.simulation.tracer import Tracer
  sc, src, lim = gc.cloud_project()
  info = _native.build_check(sc, lim)
  assert info['structure'] == 'grid' and info['grid_items'] == 390 and gc.tables_in_lds(info)
  n, seed = 5000, 0x0D15EA5E
  ref = oracle.trace(sc, src, lim, 0, n, seed, hit_capacity=40 * n, nthreads=0)
  with Tracer(0) as tr:
    tr.setScene(sc)
    tr.setSource(src)
    tr.setLimits(lim)
    tr.setDetector(None)
    tr.reserveHits(40 * n)
    tr.reset()
    tr.trace(0, n, seed, histogram=False)
    tr.sync()
    rows, cnt = tr.hits(), tr.counters()
  assert cnt == ref['counters'] and len(rows) > 2 * n
  want = ref['hits']
  assert np.array_equal(rows['tag'], want['tag'])
  figures = (np.abs(rows['point'] - want['point']).max(), np.abs(rows['direction'] - want['direction']).max(),
             np.abs(rows['power'] - want['power']).max())
  print('generated rays: points %.3e mm, directions %.3e, powers %.3e' % figures)
  # (the two samplers draw the same angles; sine and cosine of the device's and of the host's library may differ in the
  #  last place, and a component is a product of two of them: 4 ulp of 1.  The source's power is copied)
  assert figures[0] < ec.TOL and figures[1] <= 4 * 2.0**-52 and figures[2] == 0.0
  ray = (rows['tag'] & RAY).astype(np.int64)
  first = np.r_[0, np.nonzero(np.diff(ray))[0] + 1]
  start = first[np.searchsorted(first, np.arange(len(rows)), side='right') - 1]
  assert np.array_equal(rows['direction'], rows['direction'][start])                    # vacuum bends nothing


# ---- the grid kernel's own interaction code ------------------------------------------------------------------------------------
def _same(a, b, label):
  (ra, ca), (rb, cb) = a, b
  assert ca == cb, (label, ca, cb)
  assert np.array_equal(ra['tag'], rb['tag']), label
  figures = (float(np.abs(ra['point'] - rb['point']).max()), float(np.abs(ra['power'] - rb['power']).max()))
  print(f'{label}: points %.3e mm, powers %.3e over {len(ra)} rows' % figures)
  assert figures[0] < ec.TOL and figures[1] < ec.POWER_TOL


@pytest.mark.parametrize('variant', ['capped', 'power-limit', 'sequential'])
def test_interactions(native_lib, oracle, monkeypatch, variant):
  """the bench of grid_cases on the grid (ODW_BVH_THRESHOLD=4 when the context is made) against the oracle and against the
  flat kernel of a context made without it.  capped: MaxIntersections = 6 stops the rays between the perfect mirrors;
  power-limit: 0.8^3 < 0.6 ends the rays between the lossy ones at their third reflection; sequential: four steps, the
  third without the lossy mirrors, then nothing"""
  sc, lim = gc.bench()
  o, d, station = gc.bench_rays()
  if variant == 'power-limit':
    lim = dataclasses.replace(lim, power_tol=0.6)
  if variant == 'sequential':
    sc = copy.copy(sc)
    every = (1 << len(sc.group_type)) - 1
    sc.seq_enabled, sc.seq_mask = 1, np.array([every, every, every & ~1, every], np.uint64)
  flat = _launch(sc, lim, o, d, expect=('flat',))
  monkeypatch.setenv('ODW_BVH_THRESHOLD', '4')
  grid = _launch(sc, lim, o, d, expect=('grid', False, True))
  ref = oracle.trace_rays(sc, lim, o, d, nthreads=0)
  _same(grid, (ref['hits'], ref['counters']), f'{variant}: grid against the oracle')
  _same(grid, flat, f'{variant}: grid against the flat kernel')
  rows, cnt = grid
  per_ray = np.bincount((rows['tag'] & RAY).astype(np.int64), minlength=len(o))
  assert cnt['grating_in_medium'] == (station == 'in-medium').sum() == 100
  assert (per_ray[station == 'inside-ball'] == 1).all()
  if variant != 'sequential':
    assert (per_ray[station == 'tir'] == 4).all()                  # in, the side face (reflected totally), out, the floor
    assert (per_ray[station == 'perfect'] == 6).all() and cnt['capped'] == (200 if variant == 'capped' else 100)
    assert (per_ray[station == 'lossy'] == (6 if variant == 'capped' else 3)).all()
    assert len(np.unique(rows['power'])) > 300                        # (the absorbing glass moves the power)
  else:
    assert cnt['capped'] == 0 and per_ray.max() <= 4


# ---- a hit list that is too small: the designed overflow ------------------------------------------------------------------------
def test_hit_list_too_small(native_lib):
  c = gc.case('lattice')
  o, d = gc.random_set('lattice')
  want, excluded = gc.expected_for(c, o, d)
  total = sum(len(w) for w in want)
  rows, cnt = _launch(c.sc, c.lim, o, d, capacity=total // 3, expect=('grid', True, True))
  assert excluded.sum() == 0 and cnt['recorded_hits'] == total and cnt['hits_dropped'] > 0
  assert 0 < len(rows) <= total // 3 and len(rows) + cnt['hits_dropped'] == cnt['recorded_hits']
  ray = (rows['tag'] & RAY).astype(np.int64)
  worst = 0.0
  for k in np.unique(ray):
    p = rows['point'][ray == k]
    assert len(p) <= len(want[k])
    worst = max(worst, float(np.abs(p[:, None, :] - want[k][None, :, :]).max(-1).min(-1).max()))
  print(f'hit list of {total // 3} for {total} rows: {len(rows)} stored, worst {worst:.3e} mm')
  assert worst < ec.TOL
