"""Exact CSG for nested booleans: trimming conditions in disjunctive normal form (scene/geometry.py flatten ->
cond_inside bit 1 opens a clause -> the kernels keep a candidate if any clause holds).

CPU: the four disjunctive patterns and a three-level tree bake; their faces against `csg_reference` (membership
straight from the features) and, on the per-clause expansion the oracle can trace (tests/nested_booleans.py), chords
and closed-form crossings; scenes without nested booleans keep plain conjunctions; the scene-compiled kernel of a
nested structure compiles for gfx950 and is shared by a sweep; fan grids on trimmed faces.  The closed forms run on
the device too (`backend` fixture, -m gpu): the device on the clause lists, the oracle on the expansion."""
import glob
import os

import numpy as np
import pytest

from conftest import SCENES
from csg_reference import groupSolids
from nested_booleans import assert_conjunctive, expand, mount, n_clauses, nested_scene
from test_bake_independent import check_chords, sample_face, sdist, solid_table

from freecad.optics_design_workbench_amd.freecad_elements import make
from freecad.optics_design_workbench_amd.scene import Document, Placement, bake, geometry

TOL = 1e-9
EPS = 1e-5          # probe distance along the normal
MARGIN = 1e-3       # samples this close to a trimming surface are not judged


def _q(axis, deg):
  a = np.asarray(axis, float) / np.linalg.norm(axis)
  return tuple(np.r_[a * np.sin(np.radians(deg) / 2), np.cos(np.radians(deg) / 2)])


def _pl(base, axis=(1, 2, 3), deg=0.0):
  return dict(placement=Placement(base=base, quat=_q(axis, deg)))


def _parts(d):
  A = lambda: make.makeBox(d, 'A', 10, 10, 10, **_pl((0.3, -0.2, 0.1), (1, 2, 3), 17))
  B = lambda: make.makeBox(d, 'B', 8, 9, 7, **_pl((5, 3, 2), (2, -1, 1), 29))
  C = lambda: make.makeCylinder(d, 'C', 3, 30, **_pl((7, 5, -8), (1, 1, 0), 11))
  D = lambda: make.makeSphere(d, 'D', 6.5, **_pl((8, 6, 6)))
  return A, B, C, D


SHAPES = {
    'cut-of-fuse': lambda d, A, B, C, D: make.makeCut(d, make.makeFuse(d, [A(), B()], 'F'), C(), 'X'),
    'common-of-fuse': lambda d, A, B, C, D: make.makeCommon(d, [make.makeFuse(d, [A(), B()], 'F'), C()], 'X'),
    'cut-by-common': lambda d, A, B, C, D: make.makeCut(d, C(), make.makeCommon(d, [A(), B()], 'M'), 'X'),
    'fuse-of-cut': lambda d, A, B, C, D: make.makeFuse(d, [make.makeCut(d, A(), B(), 'K'), D()], 'X'),
    'three-levels': lambda d, A, B, C, D: make.makeCommon(
        d, [make.makeCut(d, make.makeFuse(d, [A(), B()], 'F'), C(), 'K'), D()], 'X'),
}


def _doc(shape, kind='Lens'):
  doc = Document()
  make.makeOpticalGroup(doc, kind, [SHAPES[shape](doc, *_parts(doc))])
  make.makeSimulationSettings(doc)
  src = make.makePointSource(doc)
  return doc, bake.bakeScene(doc, src), bake.bakeLimits(doc, src)


def _verdict(scene, p, wp):
  """the baked trimming condition of primitive p at world points wp: any clause whose literals all hold, and
  whether every literal's surface is clear of the point by MARGIN"""
  lo, hi = int(scene.prim_cond_off[p]), int(scene.prim_cond_off[p + 1])
  ok = np.zeros(len(wp), dtype=bool) if hi > lo else np.ones(len(wp), dtype=bool)
  clear = np.ones(len(wp), dtype=bool)
  held = None
  for c in range(lo, hi):
    if held is not None and int(scene.cond_inside[c]) & 2:
      ok |= held
      held = None
    if held is None:
      held = np.ones(len(wp), dtype=bool)
    o, want_inside = int(scene.cond_prim[c]), bool(int(scene.cond_inside[c]) & 1)
    m = np.linalg.inv(scene.prim_to_world[o].m)
    sd = sdist(int(scene.prim_type[o]), scene.prim_params[o], wp @ m[:3, :3].T + m[:3, 3])
    held &= (sd <= 0) if want_inside else (sd >= 0)
    clear &= np.abs(sd) > MARGIN
  if held is not None:
    ok |= held
  return ok, clear


def check_faces(doc, scene, n_per_face, seed=1):
  """check A of test_bake_independent for lists of clauses: points of a face that the clauses keep lie on the
  solid's boundary with the baked outward normal, points they reject do not"""
  rs = np.random.RandomState(seed)
  solids = solid_table(doc, scene)
  judged = kept = 0
  for p in range(scene.n_prims):
    kind, par = int(scene.prim_type[p]), scene.prim_params[p]
    R, t = scene.prim_to_world[p].m[:3, :3], scene.prim_to_world[p].m[:3, 3]
    flags = int(scene.prim_flags[p])
    flip = -1.0 if flags & 1 else 1.0
    solid = solids[int(scene.prim_solid[p])]
    for f in range(geometry.N_FACES[kind]):
      lp, ln = sample_face(kind, par, f, n_per_face, rs)
      wp, wn = lp @ R.T + t, (ln @ R.T) * flip
      ok, clear = _verdict(scene, p, wp)
      ok &= bool((flags >> (8 + f)) & 1)
      inner, outer = solid.inside(wp - EPS * wn), solid.inside(wp + EPS * wn)
      assert not np.any(clear & ok & ~inner & outer), (solid.name, p, f, 'outward normal points into the solid')
      bad = clear & (ok != (inner & ~outer))
      assert not bad.any(), (solid.name, p, f, int(bad.sum()), wp[bad][:3].tolist(), ok[bad][:3].tolist())
      judged += int(clear.sum())
      kept += int((clear & ok).sum())
  return judged, kept


# ---------------------------------------------------------------------------
# 1. the bake
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('shape', list(SHAPES))
def test_nested_booleans_bake(shape):
  """each of these was refused as "a disjunction; nested this way it needs FreeCAD" before"""
  doc, sc, lim = _doc(shape)
  assert set(np.unique(sc.cond_inside).tolist()) <= {0, 1, 2, 3}
  assert max(n_clauses(sc)) > 1                         # some face is kept by one of several clauses
  for p, k in enumerate(n_clauses(sc)):                 # a list of several clauses marks every clause's first literal
    lo, hi = int(sc.prim_cond_off[p]), int(sc.prim_cond_off[p + 1])
    assert k == 1 or (k > 1 and int(sc.cond_inside[lo]) & 2) or hi == lo
    assert not any(int(sc.cond_inside[c]) & 2 for c in range(lo, hi)) or k > 1
  assert not any(int(f) & 2 for f in sc.prim_flags)     # (ODW_FLAG_CONVEX: none of these is convex)


def test_simplification_and_caps():
  """duplicate literals, p AND NOT p, subsumed clauses go in lists of several clauses; above MAX_CLAUSES the tree is
  refused (and left to the stored shape)"""
  doc = Document()
  A, B, C, D = _parts(doc)
  a = A()
  # Cut(Fuse(A, B), A): the faces of B are kept outside A; A's own faces nowhere (outside A AND inside A)
  cut = make.makeCut(doc, make.makeFuse(doc, [a, B()], 'F'), a, 'X')
  tree, = geometry.solids_of(cut)
  flat = geometry.flatten(tree)
  for fp in flat:
    for cl in fp.clauses:
      keys = [(id(o), i) for o, i in cl]
      assert len(keys) == len(set(keys))
      if len(fp.clauses) > 1:
        assert not any((k, not i) in keys for k, i in keys)
  # sixteen spheres fused, the whole cut out of a box: the box's faces are kept outside every sphere (one clause),
  # the spheres' faces inside the box AND outside the others (one clause each) -- wide, not disjunctive
  d2 = Document()
  spheres = [make.makeSphere(d2, f'S{i}', 1.0, base=(3.0 * i, 0.0, 0.0)) for i in range(16)]
  tool = make.makeFuse(d2, spheres, 'F')
  t2, = geometry.solids_of(make.makeCut(d2, make.makeBox(d2, 'B', 60, 2, 2, base=(-2, -1, -1)), tool, 'X'))
  assert all(len(fp.clauses) == 1 for fp in geometry.flatten(t2))
  # a box cut by the Common of 17 spheres with one box each: outside a Common = 17 clauses
  d3 = Document()
  parts = [make.makeSphere(d3, f'S{i}', 5.0, base=(0.1 * i, 0.0, 0.0)) for i in range(17)]
  t3, = geometry.solids_of(make.makeCut(d3, make.makeBox(d3, 'B', 4, 4, 4), make.makeCommon(d3, parts, 'M'), 'X'))
  with pytest.raises(geometry.UnsupportedGeometry, match='clauses'):
    geometry.flatten(t3)


# ---------------------------------------------------------------------------
# 2. the bake against csg_reference
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('shape', list(SHAPES))
def test_faces_and_chords_against_csg_reference(oracle, shape):
  doc, sc, lim = _doc(shape, 'Vacuum')
  judged, kept = check_faces(doc, sc, 8000)
  assert kept > 0.05 * judged > 0
  ex = expand(sc)
  assert ex.n_prims > sc.n_prims
  assert check_chords(doc, ex, lim, oracle, 300) > 100


def test_random_nested_trees_against_csg_reference(oracle):
  done = 0
  for s in range(12):
    rs = np.random.RandomState(9100 + s)
    sc, lim, targets, doc = nested_scene(rs, optical=False)
    judged, kept = check_faces(doc, sc, 1500, seed=s)
    assert judged > 0
    check_chords(doc, expand(sc), lim, oracle, 60, seed=s)
    done += max(n_clauses(sc)) > 1
  assert done >= 8


# ---------------------------------------------------------------------------
# 3. closed forms (oracle on the expansion; the device on the clause lists)
# ---------------------------------------------------------------------------
def _vacuum(elems):
  doc = Document()
  make.makeOpticalGroup(doc, 'Vacuum', elems(doc))
  make.makeSimulationSettings(doc, DistanceTolerance='1e-6')
  src = make.makePointSource(doc)
  return bake.bakeScene(doc, src), bake.bakeLimits(doc, src)


def _crossings(backend, sc, lim, origins, dirs):
  origins, dirs = np.asarray(origins, float), np.asarray(dirs, float)
  rows = backend.traceRays(expand(sc) if backend.name == 'oracle' else sc, lim, origins, dirs)
  ray = (rows['tag'] & np.uint64(0xFFFFFFFFFFFF)).astype(np.int64)
  out = []
  for k in range(len(origins)):
    p = rows['point'][ray == k]
    out.append(np.sort((p - origins[k]) @ dirs[k]))
  return out


# (the same solids moved and turned: the crossings are the same distances along the moved rays)
MOVES = [Placement(), Placement(base=(3.0, -7.0, 11.0), quat=_q((1, 2, -1), 37.0))]


def _moved(P, o, d):
  return [P * np.asarray(x, float) for x in o], [P.m[:3, :3] @ np.asarray(x, float) for x in d]


@pytest.mark.parametrize('move', [0, 1], ids=['at-origin', 'moved'])
def test_bored_fused_blocks_crossings(backend, move):
  """Cut(Fuse(box [0,10]^3, box [8,18]x[2,8]x[2,8]), cylinder r 1.5 about x = 12, y = 5): the inner faces of the
  fused blocks are gone, the bore's wall is kept inside either block"""
  P = MOVES[move]

  def elems(d):
    a = make.makeBox(d, 'A', 10, 10, 10)
    b = make.makeBox(d, 'B', 10, 6, 6, base=(8, 2, 2))
    c = make.makeCylinder(d, 'C', 1.5, 30, base=(12, 5, -10))
    return [make.makeCut(d, make.makeFuse(d, [a, b], 'F'), c, 'X', placement=P)]
  sc, lim = _vacuum(elems)
  o = [(-10, 5, 5), (9, 5, -10), (15, -10, 5), (12, -10, 5), (12, 5, -15), (9.0, 1.0, -10)]
  d = [(1, 0, 0), (0, 0, 1), (0, 1, 0), (0, 1, 0), (0, 0, 1), (0, 0, 1)]
  want = [[10, 20.5, 23.5, 28], [10, 20], [12, 18], [12, 13.5, 16.5, 18], [], [10, 20]]
  got = _crossings(backend, sc, lim, *_moved(P, o, d))
  for g, w in zip(got, want):
    assert len(g) == len(w) and np.abs(g - w).max(initial=0) < TOL, (g, w)


@pytest.mark.parametrize('move', [0, 1], ids=['at-origin', 'moved'])
def test_slab_of_fused_spheres_crossings(backend, move):
  """Common(Fuse(sphere r 5 at 0, sphere r 5 at x = 6), slab |z| <= 2): the spheres' inner caps are gone, the slab's
  faces are kept inside either sphere"""
  P = MOVES[move]

  def elems(d):
    s1 = make.makeSphere(d, 'S1', 5)
    s2 = make.makeSphere(d, 'S2', 5, base=(6, 0, 0))
    slab = make.makeBox(d, 'Sl', 30, 20, 4, base=(-10, -10, -2))
    return [make.makeCommon(d, [make.makeFuse(d, [s1, s2], 'F'), slab], 'X', placement=P)]
  sc, lim = _vacuum(elems)
  r20 = np.sqrt(20.0)
  o = [(-20, 0, 0), (0, 0, -20), (3, 0, -20), (0, -20, 0), (2, -20, 1), (8, -20, 1.5)]
  d = [(1, 0, 0), (0, 0, 1), (0, 0, 1), (0, 1, 0), (0, 1, 0), (0, 1, 0)]
  w8 = np.sqrt(25 - 4 - 2.25)
  want = [[15, 31], [18, 22], [18, 22], [15, 25], [20 - r20, 20 + r20], [20 - w8, 20 + w8]]
  got = _crossings(backend, sc, lim, *_moved(P, o, d))
  for g, w in zip(got, want):
    assert len(g) == len(w) and np.abs(g - np.asarray(w)).max(initial=0) < TOL, (g, w)


# ---------------------------------------------------------------------------
# 4. scenes without nested booleans: plain conjunctions
# ---------------------------------------------------------------------------
def test_scenes_without_nested_booleans_keep_plain_conjunctions():
  from freecad.optics_design_workbench_amd import scenes
  from random_scenes import scene
  baked = 0
  for path in sorted(glob.glob(os.path.join(SCENES, '*.FCStd'))):
    try:
      pr = scenes.bakeProject(path)
    except Exception:                                   # (scenes that need files outside the fixture set)
      continue
    assert_conjunctive(pr.scene)
    baked += 1
  assert baked >= 10
  for s in range(20):
    sc, lim, targets = scene(np.random.RandomState(4200 + s), rich=(s % 3 == 2), crowded=(s % 5 == 4))
    assert_conjunctive(sc)
    assert expand(sc).n_prims == sc.n_prims


# ---------------------------------------------------------------------------
# 5. the scene-compiled kernel of a nested structure
# ---------------------------------------------------------------------------
def _mount_scene(bore=2.5, copies=1, lens=False, kind='Absorber'):
  """`copies` mounts (Vacuum: recording where rays enter and leave them), optionally behind a tessellated ball lens,
  and a detector plate"""
  doc = Document()
  parts = [mount(doc, bore, base=(9.0 * (k % 3) - 9.0, 9.0 * (k // 3), 40.0), name=f'M{k}') for k in range(copies)]
  make.makeOpticalGroup(doc, kind, parts, name='OpticalMountGroup', RecordHits=True)
  if lens:
    ball = make.makeSphere(doc, 'Ball', 8.0, base=(0.2, -0.1, 22.0))
    make.makeOpticalGroup(doc, 'Lens', [make.makeTessellated(doc, ball, 24)], name='OpticalLensGroup', RefractiveIndex=1.5)
  make.makeOpticalGroup(doc, 'Absorber', [make.makeBox(doc, 'Det', 60, 60, 1, base=(-30, -30, 80))], name='Detector',
                        RecordHits=True)
  make.makeSimulationSettings(doc, DistanceTolerance='1e-6')
  src = make.makePointSource(doc)
  return doc, bake.bakeScene(doc, src), bake.bakeLimits(doc, src)


def test_nested_structure_compiles_and_is_shared_by_a_sweep(native_lib):
  from freecad.optics_design_workbench_amd import _native
  headers = []
  for bore in (2.0, 2.5, 3.1):
    doc, sc, lim = _mount_scene(bore)
    header, code_bytes = _native.compile_check(sc, lim, 'structure')
    assert code_bytes > 10000
    headers.append(header)
  assert headers[0] == headers[1] == headers[2]
  # the cond table carries the clause marks (bit 30 of a cond word): the bore's wall is kept inside the tube OR the
  # flange
  table = header.split(' cond(int i) { constexpr int T[] = {')[1].split('}')[0]
  words = [int(w) for w in table.split(',')]
  assert words == [int(q) | (int(i) & 2) << 29 | (-(1 << 31) if int(i) & 1 else 0) for q, i in zip(sc.cond_prim, sc.cond_inside)]
  assert sum(1 for w in words if w & (1 << 30)) >= 2


# ---------------------------------------------------------------------------
# 6. fan grids on the faces of a nested solid
# ---------------------------------------------------------------------------
def test_fan_grid_on_the_faces_of_a_nested_solid():
  """every grid point that valid() keeps lies on the solid's boundary (csg_reference)"""
  from freecad.optics_design_workbench_amd.freecad_elements import surface_fans
  doc = Document()
  part = mount(doc, 2.5, base=(1.0, -2.0, 3.0))
  make.makeOpticalGroup(doc, 'Absorber', [part], name='G')
  solid, = groupSolids(doc)['G']
  tree, = geometry.solids_of(part)
  flat = geometry.flatten(tree)
  assert max(len(fp.clauses) for fp in flat) > 1
  views = surface_fans._boolean_faces(tree, Placement(), 1e-6)
  assert len(views) >= 5
  judged = 0
  for v in views:
    for (u, w), x, _ in surface_fans.makeSurfaceGrid(v, 400, 1e-6):
      n = np.asarray(v.normal(u, w), float)
      n /= np.linalg.norm(n)
      # (judged where the point keeps clear of every edge and every other surface: MARGIN below the face, every
      #  primitive's surface is at least MARGIN / 2 away -- its own is MARGIN away unless an edge of it is near)
      if min(abs(_sd(fp, x - MARGIN * n)) for fp in flat) < MARGIN / 2:
        continue
      assert solid.inside(x - EPS * n)[0] and not solid.inside(x + EPS * n)[0], (x.tolist(), n.tolist())
      judged += 1
  assert judged > 300


def _sd(fp, x):
  q = (np.asarray(x, float) - fp.to_world.m[:3, 3]) @ fp.to_world.m[:3, :3]
  return float(sdist(fp.kind, fp.params, q[None])[0])


def test_cond_words_are_validated_on_the_host(native_lib):
  """cond_inside outside 0..3, and clause marks in a list whose first condition has none, are refused
  (odw_build_check runs the validation of odw_upload_scene without a device)"""
  from freecad.optics_design_workbench_amd import _native
  import copy
  doc, sc, lim = _mount_scene(2.5)
  assert _native.build_check(sc, lim)['structure'] == 'flat'
  bad = copy.copy(sc)
  bad.cond_inside = np.asarray(sc.cond_inside).copy()
  bad.cond_inside[0] = 4
  with pytest.raises(_native.NativeError, match='invalid'):
    _native.build_check(bad, lim)
  p = next(p for p, k in enumerate(n_clauses(sc)) if k > 1)
  bad.cond_inside = np.asarray(sc.cond_inside).copy()
  bad.cond_inside[int(sc.prim_cond_off[p])] &= 1
  with pytest.raises(_native.NativeError, match='invalid'):
    _native.build_check(bad, lim)
