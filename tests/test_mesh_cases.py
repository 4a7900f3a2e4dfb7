"""The cases of tests/mesh_cases.py hold without a GPU: the gallery is the scene it claims to be (4204 facets, 3180 of them
flagged strictly convex, the eight-wide tree), and on every ray set, on the gallery and on the gallery moved by
tree_cases.T, the CPU oracle records per ray exactly the crossings of the brute-force reference, within 1e-9 mm.  No ray
of any set is excluded.  tests/test_gpu_mesh.py then holds the mesh kernel to both.

One exception, as in tests/test_tree_cases.py: on the set that starts 1000 mm further back the oracle is held in rows per
ray only (tree_cases.far_back_set: 1050 mm down a ray its local direction costs a few 1e-9 mm); its distance is printed.

Worst distance of the oracle from the reference, gallery / far gallery (mm): random 1.0e-11 / 3.8e-10, aimed 5.1e-12 /
1.1e-10, back 2.0e-10 / 2.0e-9, tiny components 2.8e-14 / 0, starts 1.5e-13 / 3.1e-11, length limit 1.0e-12 / 1.8e-12."""
import numpy as np
import pytest

import ellipsoid_cases as ec
import grid_cases as gc
import mesh_cases as mc
import tree_cases as tc
from grid_cases import held

PLACEMENTS = [pytest.param(False, id='gallery'), pytest.param(True, id='far')]


def _oracle(oracle, name, far):
  """the oracle's rows of a set against the reference -> (rows, origins, directions, expected points)"""
  g, o, d, want = mc.placed(name, far)
  out = oracle.trace_rays(g.sc, g.lim, o, d, nthreads=0)
  cnt = out['counters']
  assert cnt['traced_rays'] == cnt['escaped'] == len(o) and cnt['recorded_hits'] == len(out['hits']) == sum(len(w) for w in want)
  label = f'{"far " if far else ""}gallery, {name} (oracle)'
  if name == 'back':
    worst = tc.same_crossings(out['hits'], o, d, want, mc.nothing_excluded(o), label)
    assert worst < 4.0 * (tc.BACK + 300.0) * float(np.spacing(np.abs(o).max()))          # (t times 4 ulp: what that costs at most)
  else:
    held(out['hits'], o, d, want, mc.nothing_excluded(o), label)
  return out['hits'], o, d, want


def test_gallery_is_the_scene_it_claims(native_lib):
  from freecad.optics_design_workbench_amd import _native
  from freecad.optics_design_workbench_amd.scene import geometry
  assert [len(mc.facets_of(s)) for s in mc.SOLIDS] == [2208, 1024, 960, 12]
  for g in (mc.gallery(), mc.far_gallery(), mc.far_gallery(tc.FAR_LIMIT)):
    tri = np.asarray(g.sc.prim_type) == geometry.TRIANGLE
    assert tri.sum() == 4204 and len(g.sc.prim_type) == 4205
    flags = np.asarray(g.sc.prim_flags)[tri]
    both = 0x2 | 0x8                                                     # ODW_FLAG_CONVEX | ODW_FLAG_STRICTLY_CONVEX
    assert ((flags & both) == both).sum() == 3180 and ((flags & both) == 0).sum() == 1024
    info = _native.build_check(g.sc, g.lim)
    print(info)
    assert info['structure'] == 'wide-bvh' and info['primitives'] == 4205 and info['dead_primitives'] == 0, info
  assert float(mc.far_gallery(tc.FAR_LIMIT).lim.max_ray_length) == tc.FAR_LIMIT and float(mc.gallery().lim.max_ray_length) == 1000.0
  # far away nine vertices in ten (the cube's and a few on the axes are whole numbers) and every origin of the random set
  # are no float32 numbers
  v = np.concatenate([mc.meshes()[s][0] for s in mc.SOLIDS]) + mc.T
  assert (v.astype(np.float32).astype(float) != v).any(1).mean() > 0.9
  o = mc.random_set()[0] + mc.T
  assert (o.astype(np.float32).astype(float) != o).any(1).all()


def test_reference_on_lines_worked_out_by_hand():
  """the brute-force reference itself: a line through the cube, the sphere and the ball along an axis, a line through a
  vertex of the cube (one crossing there, not six), the length limit"""
  lo, hi = mc.CUBE_C - mc.CUBE_HALF, mc.CUBE_C + mc.CUBE_HALF
  o = np.array([[mc.CUBE_C[0] - 50.0, mc.CUBE_C[1] + 1.0, mc.CUBE_C[2] + 0.5], [0.0, 0.0, -20.0], lo - 30.0, [0.0, 0.0, -1000.0 + 28.0]])
  d = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [1.0, 1.0, 1.0], [0.0, 0.0, 1.0]])
  want = mc.facet_crossings(o, d, 1000.0)
  assert np.abs(want[0] - [[lo[0], o[0, 1], o[0, 2]], [hi[0], o[0, 1], o[0, 2]]]).max() < 1e-12
  assert np.abs(want[1] - [[0.0, 0.0, 29.0], [0.0, 0.0, 41.0]]).max() < 1e-12
  assert len(want[2]) == 2 and np.abs(want[2] - [lo, hi]).max() < 1e-12
  assert len(want[3]) == 0 and len(mc.facet_crossings(o[3:], d[3:], 1002.0)[0]) == 2


@pytest.mark.parametrize('far', PLACEMENTS)
def test_random_lines(oracle, far):
  _, o, d, want = _oracle(oracle, 'random', far)
  assert sum(len(w) for w in want) == 1608
  octants = {tuple(s) for s in (d > 0)}
  assert len(octants) == 8
  # every solid is met, the torus four times by some ray
  assert max(len(w) for w in want) >= 4


@pytest.mark.parametrize('far', PLACEMENTS)
def test_edges_and_vertices(oracle, far):
  rows, o, d, want = _oracle(oracle, 'aimed', far)
  _, _, points, on_edge = mc.aimed_set()
  assert len(o) == 2160 and on_edge.sum() == 1620
  mc.aimed_once(rows, o, d, points + (mc.T if far else 0.0), 'aimed (oracle)')
  # (the reference says the same)
  for k, w in enumerate(want):
    assert (np.abs(w - (points[k] + (mc.T if far else 0.0))).max(1) < ec.TOL).sum() == 1, k


@pytest.mark.parametrize('far', PLACEMENTS)
def test_from_far_back(oracle, far):
  _, o, d, want = _oracle(oracle, 'back', far)
  assert sum(len(w) for w in want) == 1608                              # what the first random set meets


@pytest.mark.parametrize('far', PLACEMENTS)
def test_tiny_components(oracle, far):
  with np.errstate(over='ignore'):
    for z in (1e-40, -1e-40, 1e-30, -1e-30):
      assert z in tc.TINY and np.isfinite(1.0 / z) and np.isinf(np.float32(1.0 / z)) == (abs(z) == 1e-40)
  for name in mc.tiny_sets():
    _, o, d, want = _oracle(oracle, name, far)
    assert len(o) == 36
    # the cube twice, the ball twice; the line through the ball along x also crosses the torus: its tube twice (four
    # crossings) coming from -x, the far side of the tube (two) from +x, where the ray starts in the torus' hole
    assert [len(w) for w in want] == [2, 2, 2, 2, 2, 6, 2, 2, 2, 2, 2, 4] + [2] * 24, name


@pytest.mark.parametrize('far', PLACEMENTS)
def test_starts_and_length_limit(oracle, far):
  rows, o, d, want = _oracle(oracle, 'starts', far)
  _, _, centroid, recorded = mc.starts_set()
  shift = mc.T if far else 0.0
  assert recorded.sum() == 200 and np.isfinite(centroid[:, 0]).sum() == 400
  got = ec.per_ray(rows, o, d)
  for k in np.nonzero(np.isfinite(centroid[:, 0]))[0]:
    for points in (want[k], got[k]):
      assert (np.abs(points - (centroid[k] + shift)).max(1) < ec.TOL).sum() == int(recorded[k]), (k, points)
  inside = np.nonzero(~np.isfinite(centroid[:, 0]))[0]
  assert len(inside) == 400 and all(len(want[k]) >= 1 for k in inside)     # (they start inside a solid: at least the way out)
  rows, o, d, want = _oracle(oracle, 'length-limit', far)
  _, _, points, beyond = mc.length_limit_set()
  assert beyond.sum() == 30 and all(len(want[k]) == 0 for k in np.nonzero(beyond)[0])
  for k in np.nonzero(~beyond)[0]:
    assert len(want[k]) >= 2 and np.abs(want[k][0] - (points[k] + shift)).max() < ec.TOL


@pytest.mark.parametrize('variant', ['capped', 'power-limit', 'sequential'])
def test_faceted_bench(oracle, native_lib, variant):
  """grid_cases.bench(faceted=True) is a scene of the mesh kernel, and the oracle gives the station figures that do not
  depend on the tessellation"""
  from freecad.optics_design_workbench_amd import _native
  sc, lim = mc.faceted_bench(variant)
  assert _native.build_check(sc, lim)['structure'] == 'wide-bvh'
  o, d, station = gc.bench_rays()
  ref = oracle.trace_rays(sc, lim, o, d, nthreads=0)
  gc.bench_figures(ref['hits'], ref['counters'], station, variant)


# ---- ties between facets: the rule of nearest_skipping (and of intersect_tri, which test_gpu_mesh.py holds to it) ----------------
@pytest.mark.parametrize('swapped', [False, True])
def test_facets_that_tie_go_by_their_number(oracle, swapped):
  """a ray through the edge that a facet facing it shares with one facing away meets both within rounding of each other:
  one row, at the aimed point, with the entering bit of the facet listed first -- whichever t came out a bit smaller"""
  sc, lim, o, d, points = mc.wedges(swapped=swapped)
  rows = oracle.trace_rays(sc, lim, o, d, nthreads=0)['hits']
  assert np.array_equal((rows['tag'] & np.uint64(0xFFFFFFFFFFFF)).astype(np.int64), np.arange(len(o)))     # one row per ray
  assert np.abs(rows['point'] - points).max() < ec.TOL
  assert np.array_equal(rows['tag'] >> np.uint64(63), np.full(len(o), 0 if swapped else 1, np.uint64))


@pytest.mark.parametrize('offset, group', [(5e-10, 1), (-5e-10, 0)])
def test_a_facet_and_an_analytic_face_compare_exactly(oracle, offset, group):
  """a patch of facets 5e-10 mm above (below) the top of a box, inside the window of the facet rule: the nearer of the
  two is met, as between analytic faces -- the window is for facets among themselves"""
  sc, lim, o, d = mc.facet_on_a_box(offset)
  rows = oracle.trace_rays(sc, lim, o, d, nthreads=0)['hits']
  first = mc.first_rows(rows, o)
  assert (first >= 0).all()
  assert np.array_equal((rows['tag'][first] >> np.uint64(48)) & np.uint64(0x7FFF), np.full(len(o), group, np.uint64))
  assert np.abs(rows['point'][first][:, 2] - max(offset, 0.0)).max() < ec.TOL
