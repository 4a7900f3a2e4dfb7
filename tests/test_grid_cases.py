"""The cases of tests/grid_cases.py hold without a GPU: every scene takes the grid with the sizes and the table placement
its test counts on (odw_build_check), and on every ray set the CPU oracle records exactly the crossings of the closed
form, within 1e-9 mm.  tests/test_gpu_grid.py then holds the grid kernel to both."""
import numpy as np
import pytest

import ellipsoid_cases as ec
import grid_cases as gc
from grid_cases import held

# rays decided by rounding in the oracle itself, by (scene, set, index): none was found
BY_NAME = {}


def _oracle_rows(oracle, c, o, d):
  out = oracle.trace_rays(c.sc, c.lim, o, d, nthreads=0)
  return out['hits'], out['counters']


@pytest.mark.parametrize('name', gc.SCENES)
def test_scenes_take_the_grid_with_their_tables_where_the_tests_count_on_them(native_lib, name):
  from freecad.optics_design_workbench_amd import _native
  c = gc.case(name)
  info = _native.build_check(c.sc, c.lim)
  print(name, info)
  assert info['structure'] == 'grid' and info['primitives'] == len(c.solids) and info['dead_primitives'] == 0
  assert (info['grid_cells'], info['grid_items']) == (c.cells, c.items), info
  assert gc.tables_in_lds(info) == c.in_lds, info
  if c.in_lds:
    assert gc.sphere_records(info) == c.spheres, info
  # the planes as this file restates them give the same number of cells
  assert np.prod([len(p) - 1 for p in gc.planes(c.solids)]) == c.cells
  if name in ('lattice', 'mixed'):
    assert name != 'lattice' or info['grid_lds_bytes'] == 63696
    px, py, pz = gc.planes(c.solids)
    assert np.abs(px[1:-1] - [5, 15, 25, 35]).max() < 1e-12 and np.abs(py[1:-1] - [5, 15, 25]).max() < 1e-12
  if name == 'big':
    assert info['grid_lds_bytes'] == 59744


@pytest.mark.parametrize('name', ['cloud', 'staggered', 'big', 'seventy'])
def test_random_lines(oracle, name):
  c = gc.case(name)
  o, d = gc.random_set(name)
  want, excluded = gc.expected_for(c, o, d)
  assert excluded.sum() == 0                                     # a condition of the sets, not a measurement
  assert sum(len(w) for w in want) > 500
  if name == 'cloud':
    assert sum(len(w) for w in want) == 7028 and max(len(w) for w in want) == 16
  if not c.oracle_knows:
    return
  rows, cnt = _oracle_rows(oracle, c, o, d)
  held(rows, o, d, want, excluded, f'{name} random lines')
  assert cnt['recorded_hits'] == sum(len(w) for w in want) and cnt['traced_rays'] == cnt['escaped'] == len(o)


def test_rays_started_inside_the_cloud(oracle):
  c = gc.case('cloud')
  o, d = gc.inside_starts()
  want, excluded = gc.expected_for(c, o, d)
  assert excluded.sum() == 0
  inside = sum(np.linalg.norm(o - s[1], axis=1) < s[2] for s in c.solids)
  assert (inside == 1).sum() > 50 and (inside >= 2).sum() > 10
  rows, cnt = _oracle_rows(oracle, c, o, d)
  held(rows, o, d, want, excluded, 'cloud inside starts')
  o, d = gc.overlap_starts()
  inside = sum(np.linalg.norm(o - s[1], axis=1) < s[2] for s in c.solids)
  assert len(o) == 60 and (inside >= 2).all()
  want, excluded = gc.expected_for(c, o, d)
  assert excluded.mean() <= 0.05
  held(_oracle_rows(oracle, c, o, d)[0], o, d, want, excluded, 'cloud overlap starts')


@pytest.mark.parametrize('name', ['lattice', 'mixed'])
def test_aimed_sets(oracle, name):
  c = gc.case(name)
  rays = kept = 0
  for label, (o, d) in gc.aimed_sets(name).items():
    want, excluded = gc.expected_for(c, o, d)
    if label.startswith('axis'):
      # the rays 2 + 1e-9 beside a row graze: nothing recorded (a cube in the row is met within its tolerance: its own
      # matter); the rays 1.999 beside it record the full chord of every sphere of the row.  Nothing else is excluded
      assert np.array_equal(excluded, gc.AXIS_GRAZING)
      rows, _ = _oracle_rows(oracle, c, o, d)
      got = ec.per_ray(rows, o, d)
      chord = 2 * np.sqrt(gc.RADIUS**2 - 1.999**2)
      for k in np.nonzero(gc.AXIS_GRAZING)[0]:
        spheres_only = all(np.linalg.norm(g - s[1]) > 4.0 for g in got[k] for s in c.solids if s[0] == 'sphere')
        assert (len(got[k]) == 0) if name == 'lattice' else spheres_only, (label, k, got[k])
      for k in np.nonzero(gc.AXIS_CHORD)[0]:
        assert len(want[k]) == 2 * gc.SHAPE[k // 8]
        steps = np.linalg.norm(np.diff(want[k], axis=0), axis=1)[::2]
        if name == 'lattice':
          assert np.abs(steps - chord).max() < 1e-9
    elif label == 'length-limit':
      beyond = gc.length_limit()[2]
      assert excluded.sum() == 0 and all(len(w) == 0 for w, b in zip(want, beyond) if b) and all(len(w) >= 2 for w, b in zip(want, beyond) if not b)
    elif label == 'in-plane':
      assert excluded.sum() == 0 and all(len(w) == 0 for w in want)
    else:
      assert excluded.sum() == 0, (label, np.nonzero(excluded)[0])
    rows, cnt = _oracle_rows(oracle, c, o, d)
    held(rows, o, d, want, excluded, f'{name} {label}', BY_NAME.get((name, label), ()))
    assert cnt['traced_rays'] == cnt['escaped'] == len(o)
    rays += len(o)
    # (the grazing rays of the axis sets are held to an expectation of their own above: they stay)
    kept += len(o) - (0 if label.startswith('axis') else int(excluded.sum())) - len(BY_NAME.get((name, label), ()))
  assert kept >= 0.95 * rays, (kept, rays)


def test_rays_in_the_planes_of_the_staggered_scene(oracle):
  """the even cuts of the staggered scene pass through spheres: a ray in such a plane crosses solids listed on both sides"""
  c = gc.case('staggered')
  o, d = gc.in_plane(c.solids)
  want, excluded = gc.expected_for(c, o, d)
  assert len(o) == 45 and excluded.mean() <= 0.05 and sum(len(w) for w in want) > 60
  held(_oracle_rows(oracle, c, o, d)[0], o, d, want, excluded, 'staggered in-plane')
