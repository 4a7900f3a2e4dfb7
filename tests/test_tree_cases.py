"""The cases of tests/tree_cases.py hold without a GPU: on every new set the CPU oracle records exactly the crossings of the
closed form, within 1e-9 mm, its segment rows are the chain through them, and the conditions of the sets hold as
conditions: nothing excluded on the aimed, tiny-component, face-centre and face-diagonal sets (but the grazing rays
grid_cases.AXIS_GRAZING names), at most 5 % on the far random sets, at least 60 crossings per set (the far aimed sets: per
family -- the in-plane rays of a lattice cross nothing by design).  tests/test_gpu_tree.py then holds the binary-tree
kernel to both.

Facet diagonals: the oracle records exactly one row where a ray meets the edge two triangles of a face share (the shared
edge is not widened), so no ray had to be named."""
import numpy as np
import pytest

import ellipsoid_cases as ec
import grid_cases as gc
import tree_cases as tc
from grid_cases import held

# rays decided by the reference's tolerance rule in the oracle itself, by (case, set): none was found
BY_NAME = {}


def _oracle(oracle, c, o, d, label, want, excluded, by_name=()):
  """oracle rows against the closed form, oracle segments against the chain -> crossings"""
  out = oracle.trace_rays(c.sc, c.lim, o, d, nthreads=0)
  _, crossings = held(out['hits'], o, d, want, excluded, label, by_name)
  assert out['counters']['traced_rays'] == out['counters']['escaped'] == len(o)
  segs = oracle.trace_segments(c.sc, c.lim, origins=o, dirs=d)['segments']
  tc.held_segments(segs, segs, o, d, want, excluded, f'{label}, segments', by_name, float(c.lim.max_ray_length))
  return crossings


@pytest.mark.parametrize('name', ['lattice', 'mixed'])
def test_far_placement(oracle, native_lib, name):
  from freecad.optics_design_workbench_amd import _native
  c = tc.far_case(name)
  info = _native.build_check(c.sc, c.lim)
  print(name, info)
  assert info['nodes'] > 0 and info['primitives'] == 80 and info['dead_primitives'] == 0
  assert float(c.lim.max_ray_length) == 1000.0
  # neither a box edge nor an origin of the random set is a float32 number
  edges = np.array([np.r_[s[1] - 2.0 - 2e-6, s[1] + 2.0 + 2e-6] if s[0] == 'sphere' else np.r_[s[1] - 2e-6, s[2] + 2e-6] for s in c.solids])
  assert (edges.astype(np.float32).astype(float) != edges).all()
  aimed = 0
  for label, (o, d) in tc.far_sets(name).items():
    want, excluded = gc.expected_for(c, o, d)
    if label == 'random':
      assert (o.astype(np.float32).astype(float) != o).any(1).all()
      want, excluded = tc.far_expected(c, o, d)
      print(f'far {name} random: {int(excluded.sum())} of {len(o)} rays excluded')
      assert excluded.mean() <= 0.05, (label, excluded.sum())
      assert _oracle(oracle, c, o, d, f'far {name} {label}', want, excluded) >= 60
      continue
    if label.startswith('axis'):
      assert np.array_equal(excluded, gc.AXIS_GRAZING), label
      # (what a grazing ray records is the oracle's own matter -- test_grid_cases holds it on the unmoved scene)
      by_name = tuple(np.nonzero(gc.AXIS_GRAZING)[0])
    else:
      assert excluded.sum() == 0, (label, np.nonzero(excluded)[0])
      by_name = ()
    if label == 'length-limit':
      beyond = gc.length_limit()[2]
      assert all(len(w) == 0 for w, b in zip(want, beyond) if b) and all(len(w) >= 2 for w, b in zip(want, beyond) if not b)
    aimed += _oracle(oracle, c, o, d, f'far {name} {label}', want, excluded, by_name)
  assert aimed >= 60
  # the second random set: from 1000 mm further away, under the longer limit
  back = tc.far_case(name, tc.FAR_LIMIT)
  assert float(back.lim.max_ray_length) == tc.FAR_LIMIT
  o, d = tc.far_back_set(name)
  want, excluded = tc.far_expected(back, o, d)
  print(f'far {name} random+1000: {int(excluded.sum())} of {len(o)} rays excluded')
  assert excluded.mean() <= 0.05, excluded.sum()
  # (it meets what the first meets and whatever lies behind the first's origins)
  first = gc.expected_for(c, *tc.far_sets(name)['random'])[0]
  assert sum(len(w) for w in want) >= sum(len(w) for w in first)
  assert sum(len(w) for w, skip in zip(want, excluded) if not skip) >= 60
  # the oracle on it: the rows of the closed form, ray by ray -- but NOT within ec.TOL (see tree_cases.far_back_set: the
  # reference's local direction costs t * a few ulp of 11000 mm, measured here as 2.5e-9 mm on the lattice and 7.2e-9 mm
  # on the mixed lattice at t = 1050 mm).  The figure is printed, the device is held to the closed form in test_gpu_tree
  rows = oracle.trace_rays(back.sc, back.lim, o, d, nthreads=0)
  worst = tc.same_crossings(rows['hits'], o, d, want, excluded, f'far {name} random+1000 (oracle)')
  assert rows['counters']['traced_rays'] == rows['counters']['escaped'] == len(o)
  assert worst < 4.0 * (tc.BACK + 100.0) * float(np.spacing(np.abs(o).max()))           # (t times 4 ulp: what that costs at most)


def test_tiny_components(oracle):
  c = tc.far_case('lattice')
  # 1 / 1e-40 overflows float32 and not float64; 1 / 1e-30 stays finite in float32 (3.4e38 is the largest), as do its
  # products with the 60 mm the slabs lie away; 1e-200 is a zero in float32 and 1 / 1e-200 infinite there
  with np.errstate(over='ignore'):
    for z in (1e-40, -1e-40, 1e-30, -1e-30):
      assert z in tc.TINY and np.isfinite(1.0 / z) and np.isinf(np.float32(1.0 / z)) == (abs(z) == 1e-40)
  for label, (o, d) in tc.tiny_sets().items():
    want, excluded = gc.expected_for(c, o, d)
    assert excluded.sum() == 0 and len(o) == 12, label
    for k, w in enumerate(want):
      assert len(w) == 2 * gc.SHAPE[k // 4], (label, k)                   # the whole row, centre line and chord
    assert _oracle(oracle, c, o, d, label, want, excluded) >= 60


def test_facets_in_the_binary_tree(oracle, native_lib, monkeypatch):
  from freecad.optics_design_workbench_amd import _native
  c = tc.facet_case()
  assert (np.asarray(c.sc.prim_type) == 5).sum() == 12 * 27 and len(c.sc.prim_type) == 12 * 27 + 53
  assert _native.build_check(c.sc, c.lim)['structure'] == 'wide-bvh'               # (the mesh kernel, the variable unset)
  monkeypatch.setenv('ODW_MESH_KERNEL', '0')
  info = _native.build_check(c.sc, c.lim)
  print(info)
  assert info['structure'] == 'bvh' and info['nodes'] > 0, info
  for label, (o, d) in tc.facet_sets().items():
    want, excluded = gc.expected_for(c, o, d)
    if label == 'random':
      assert excluded.mean() <= 0.05
    else:
      assert excluded.sum() == 0, (label, np.nonzero(excluded)[0])
    if label == 'face diagonals':
      # the closed form says one crossing at the point on the shared edge
      p = tc.face_diagonals()[2]
      assert len(o) == 2 * 6 * 27
      for k, w in enumerate(want):
        assert (np.abs(w - p[k]).max(1) < 1e-9).sum() == 1, (k, w, p[k])
    assert _oracle(oracle, c, o, d, f'facets {label}', want, excluded, BY_NAME.get(('facets', label), ())) >= 60


@pytest.mark.parametrize('name', ['lattice', 'cloud'])
def test_segment_chains_of_the_grid_cases(oracle, name):
  """the chain on scenes test_grid_cases already holds: the aimed sets of the lattice, the random lines of the cloud"""
  c = gc.case(name)
  sets = gc.aimed_sets(name) if name == 'lattice' else {'random': gc.random_set(name), 'inside': gc.inside_starts()}
  for label, (o, d) in sets.items():
    want, excluded = gc.expected_for(c, o, d)
    _oracle(oracle, c, o, d, f'{name} {label}', want, excluded, tuple(np.nonzero(excluded)[0]))
