"""The conicoid (primitive kind 8: x^2 + y^2 + (1 + K) z^2 <= 2 R z, 0 <= z <= H) without a GPU: the bake and the flat
tables against membership read straight from the features, the host builders and the compiler of scene kernels
(`odw_build_check`, `odw_compile_check`: no device needed), the tessellation, make.makeConicLens against its defining
inequality, what stays refused by name, and the numpy references of the device tests against themselves."""
import copy

import numpy as np
import pytest

import conicoid_cases as cc
from conftest import project
from freecad.optics_design_workbench_amd.freecad_elements import make
from freecad.optics_design_workbench_amd.scene import Document, bake, geometry
from freecad.optics_design_workbench_amd.scene.geometry import UnsupportedGeometry
from freecad.optics_design_workbench_amd.scene.placement import Placement


def _local(sc, p, x):
  m = np.asarray(sc.prim_xform[p], float).reshape(3, 4)          # global -> local
  return x @ m[:, :3].T + m[:, 3]


def _sdist(sc, p, x):
  """distance of the points x from primitive p of the flat tables"""
  q, par = _local(sc, p, x), np.asarray(sc.prim_params[p], float)
  if sc.prim_type[p] == geometry.BOX:
    return cc.box_distance(q, np.zeros(3), par[:3])
  if sc.prim_type[p] == geometry.CYLINDER:
    return np.maximum(np.hypot(q[:, 0], q[:, 1]) - par[0], np.maximum(-q[:, 2], q[:, 2] - par[1]))
  assert sc.prim_type[p] == geometry.CONICOID
  return cc.distance(q, par[0], par[1], par[2])


def _member(sc, x):
  """membership from the flat tables of ONE solid: a conjunction (inside every primitive, outside the flipped ones:
  Common, Cut; every literal of every trimming list asks for that side of its operand), or a union (Fuse: no flips,
  every literal asks for the outside of its operand).  -> (inside, distance from the nearest surface)"""
  flip = (np.asarray(sc.prim_flags) & 1).astype(bool)
  conds = [(p, int(sc.cond_prim[c]), bool(sc.cond_inside[c] & 1)) for p in range(sc.n_prims) for c in range(sc.prim_cond_off[p], sc.prim_cond_off[p + 1])]
  assert all(o != p for p, o, _ in conds)
  sd = np.array([_sdist(sc, p, x) for p in range(sc.n_prims)])
  if conds and not flip.any() and not any(inside for _, _, inside in conds):
    return np.any(sd < 0, axis=0), np.abs(sd).min(axis=0)
  assert all(inside == (not flip[o]) for _, o, inside in conds)
  return np.all(np.where(flip[:, None], sd > 0, sd < 0), axis=0), np.abs(sd).min(axis=0)


def test_bake_and_build(native_lib):
  from freecad.optics_design_workbench_amd import _native
  pl = cc.PLACEMENTS[1]
  rng = np.random.default_rng(3)
  x = rng.uniform(-22, 22, (20000, 3))
  lim = bake.Limits(dist_tol=1e-6)
  # ---- alone: kind, parameters with the rim filled in, the two faces, the convex flag, the box
  for (K, H), name in zip(cc.CASES, cc.IDS):
    doc, src = cc.document([('Vacuum', lambda d: [cc.conicoid(d, 'C', cc.R0, K, H, **pl)], {})])
    sc = bake.bakeScene(doc, src)
    rim = np.sqrt(2 * cc.R0 * H - (1 + K) * H * H)
    assert list(sc.prim_type) == [geometry.CONICOID] == [8] == [_native.PRIM_CONICOID]
    assert np.array_equal(sc.prim_params[0][:3], [cc.R0, K, H]) and abs(sc.prim_params[0][3] - rim) < 1e-14
    assert ((int(sc.prim_flags[0]) >> 8) & 0xff) == 0b101 and int(sc.prim_flags[0]) & _native.FLAG_CONVEX
    got, near = _member(sc, x)
    direct = cc.feature_member(doc.C)(x)
    keep = near > 10 * cc.DIST_TOL
    assert keep.sum() > 19900 and np.array_equal(got[keep], direct[keep]) and 50 < direct.sum() < 10000, name
    info = _native.build_check(sc, lim)
    assert info['structure'] in ('grid', 'bvh') and info['primitives'] == 1 and info['dead_primitives'] == 0
    # points of the surface and of the cap lie in the box; the cap's own box is the disc's
    P = Placement(**pl)
    rho, phi = rim * np.sqrt(rng.uniform(0, 1, 2000)), rng.uniform(0, 2 * np.pi, 2000)
    s = np.stack([rho * np.cos(phi), rho * np.sin(phi), cc.sag(rho, cc.R0, K)], axis=1)
    w = np.array([P * p for p in np.vstack([s, s * [1, 1, 0] + [0, 0, H]])])
    lo, hi = geometry.world_aabb(sc.prim_to_world[0], *geometry.local_bounds(geometry.CONICOID, sc.prim_params[0]))
    assert np.all(w >= lo - 1e-12) and np.all(w <= hi + 1e-12)
    flo, fhi = geometry.face_local_bounds(geometry.CONICOID, sc.prim_params[0], 2)
    assert np.allclose(flo, [-rim, -rim, H], atol=1e-14) and np.allclose(fhi, [rim, rim, H], atol=1e-14)
    flo, fhi = geometry.face_local_bounds(geometry.CONICOID, sc.prim_params[0], 0)
    assert np.allclose(flo, [-rim, -rim, 0], atol=1e-14) and np.allclose(fhi, [rim, rim, H], atol=1e-14)
  # ---- in a Cut (both ways), a Common and a Fuse with a box
  K, H = cc.CASES[0]
  builders = {
      'cut-block': lambda d: make.makeCut(d, cc.centred_box(d, 'B', *cc.BLOCK), cc.conicoid(d, 'C', cc.R0, K, H), name='S'),
      'cut-conicoid': lambda d: make.makeCut(d, cc.conicoid(d, 'C', cc.R0, K, H), cc.centred_box(d, 'B', *cc.DRILL), name='S'),
      'common': lambda d: make.makeCommon(d, [cc.conicoid(d, 'C', cc.R0, K, H), cc.centred_box(d, 'B', *cc.HALF)], name='S'),
      'fuse': lambda d: make.makeFuse(d, [cc.conicoid(d, 'C', cc.R0, K, H), cc.centred_box(d, 'B', *cc.DRILL)], name='S')}
  for case, build in builders.items():
    doc, src = cc.document([('Vacuum', lambda d: [build(d)], {})])
    sc = bake.bakeScene(doc, src)
    assert sorted(sc.prim_type) == [geometry.BOX, geometry.CONICOID]
    c = list(sc.prim_type).index(geometry.CONICOID)
    assert abs(sc.prim_params[c][3] - cc.rim_of(cc.R0, K, H)) < 1e-14 and ((int(sc.prim_flags[c]) >> 8) & 0xff) & ~0b101 == 0
    assert bool(int(sc.prim_flags[c]) & 1) == (case == 'cut-block')                    # (the tool of a Cut is flipped)
    got, near = _member(sc, x)
    direct = cc.feature_member(doc.S)(x)
    if case != 'fuse':
      assert np.array_equal(direct, cc.trim_member(case, x))
    keep = near > 10 * cc.DIST_TOL
    assert keep.sum() > 19900 and np.array_equal(got[keep], direct[keep]) and 200 < direct.sum() < 19000, case
    info = _native.build_check(sc, lim)
    assert info['structure'] in ('grid', 'bvh') and info['primitives'] == 2 and info['dead_primitives'] == 0
  # ---- facets beside a conicoid: the binary tree (the mesh kernel's eight-wide tree does not know the kind)
  def with_mesh(extra):
    return cc.vacuum(lambda d: [make.makeTessellated(d, make.makeSphere(d, 'S', 5.0, base=(100, 0, 0)), 16)] + extra(d))[0]
  assert _native.build_check(with_mesh(lambda d: []), lim)['structure'] == 'wide-bvh'
  assert _native.build_check(with_mesh(lambda d: [cc.conicoid(d, 'C', cc.R0, K, H)]), lim)['structure'] == 'bvh'
  # ---- bad parameters: by the bake (naming the object) and by the library
  for bad in ((0.0, -1.0, 5.0), (10.0, -1.0, 0.0), (10.0, 1.0, 5.1), (10.0, float('nan'), 5.0), (float('inf'), 0.0, 5.0)):
    with pytest.raises(UnsupportedGeometry, match='Bad.*conicoid'):
      cc.vacuum(lambda d: [cc.conicoid(d, 'Bad', *bad)])


def test_build_check_accepts_and_refuses(native_lib):
  from freecad.optics_design_workbench_amd import _native
  lim = bake.Limits(dist_tol=1e-6)
  alone, _ = cc.vacuum(lambda d: [cc.conicoid(d, 'C', cc.R0, 1.0, 5.0)])          # (up to the equator itself: accepted)
  assert _native.build_check(alone, lim)['primitives'] == 1
  # (the library fills the rim whatever the descriptor says)
  other = copy.copy(alone)
  other.prim_params = np.array([[cc.R0, 1.0, 5.0, 123.0]])
  assert _native.build_check(other, lim) == _native.build_check(alone, lim)
  assert _native.spec_image(other, lim)['image'].tobytes() == _native.spec_image(alone, lim)['image'].tobytes()
  for bad in ((0.0, -1.0, 5.0), (-3.0, -1.0, 5.0), (10.0, -1.0, 0.0), (10.0, -2.0, -1.0), (10.0, 1.0, 5.0 + 1e-9), (10.0, float('nan'), 5.0),
              (float('nan'), 0.0, 5.0), (10.0, 0.0, float('nan')), (10.0, float('inf'), 5.0)):
    sb = copy.copy(alone)
    sb.prim_params = np.array([list(bad) + [0.0]])
    with pytest.raises(_native.NativeError, match='invalid argument.*conicoid'):
      _native.build_check(sb, lim)
  capped = copy.copy(alone)
  capped.prim_flags = np.asarray(alone.prim_flags) | (0b010 << 8)                  # face 1: the vertex is a point
  with pytest.raises(_native.NativeError, match='unsupported.*conicoid'):
    _native.build_check(capped, lim)


def test_value_image_entries(native_lib):
  """the constants the conicoid's branch derives from parameters and tolerance, hoisted into the value image: H + tol,
  (rim + tol)^2 and 1 + K, each the very operations the generic kernels perform"""
  from freecad.optics_design_workbench_amd import _native
  tol = 1e-6
  for K, H in cc.CASES:
    sc, _ = cc.vacuum(lambda d: [cc.conicoid(d, 'C', 10.3, K, H, **cc.PLACEMENTS[1]), make.makeBox(d, 'B', 1, 2, 3, base=(50, 0, 0))])
    out = _native.spec_image(sc, bake.Limits(dist_tol=tol))
    img, par, der = out['image'], int(out['par'][0]), int(out['der'][0])
    rim = np.sqrt(2.0 * 10.3 * H - (1.0 + K) * H * H)
    assert np.array_equal(img[par:par + 4], [10.3, K, H, rim]) and der > par
    assert np.array_equal(img[der:der + 3], [H + tol, (rim + tol) * (rim + tol), 1.0 + K])
    assert int(out['der'][1]) == der + 3 or int(out['frame'][1]) == der + 3           # (three entries, no more)


def test_compile_check(native_lib):
  from freecad.optics_design_workbench_amd import _native
  lim = bake.Limits(dist_tol=1e-6)
  K, H = cc.CASES[0]
  three = cc.vacuum(lambda d: [cc.conicoid(d, 'C', cc.R0, K, H), make.makeParaboloid(d, 'P', 10.0, 5.0, base=(100, 0, 0)),
                               make.makeEllipsoid(d, 'E', 5.0, 3.0, 2.0, base=(0, 100, 0))])[0]
  for scn, rare in ((cc.vacuum(lambda d: [cc.conicoid(d, 'C', cc.R0, K, H, **cc.PLACEMENTS[1])])[0], 4), (cc.trim_scene('cut-block')[0], 4), (three, 7)):
    header, code_bytes = _native.compile_check(scn, lim, 'structure')              # (arch: gfx950)
    assert code_bytes > 10000 and f'static constexpr int rare() {{ return {rare}; }}' in header
  pr = project('lensesAndMirrors')
  header, _ = _native.compile_check(pr.scene, pr.limits, 'structure')
  assert 'static constexpr int rare() { return 0; }' in header


@pytest.mark.parametrize('case', cc.CASES, ids=cc.IDS)
def test_tessellation(case):
  K, H = case
  rim = cc.rim_of(cc.R0, K, H)
  v, tri, vn = geometry.tessellate(geometry.CONICOID, (cc.R0, K, H, rim), 48)
  on_cap = v[:, 2] == H
  rho = np.hypot(v[:, 0], v[:, 1])
  assert np.abs(v[~on_cap, 2] - cc.sag(rho[~on_cap], cc.R0, K)).max() < 1e-12 and np.abs(cc.q_of(v[~on_cap], cc.R0, K)).max() < 1e-11
  assert rho.max() <= rim + 1e-12 and on_cap.sum() > 48
  # vertex normals: the gradient's on the surface, +z on the cap (the rim row belongs to both faces: either)
  g = np.stack([v[:, 0], v[:, 1], (1.0 + K) * v[:, 2] - cc.R0], axis=1)
  g /= np.linalg.norm(g, axis=1)[:, None]
  d_surface, d_cap = np.abs(vn - g).max(axis=1), np.abs(vn - [0, 0, 1]).max(axis=1)
  assert d_surface[~on_cap].max() < 1e-12 and np.minimum(d_surface, d_cap).max() < 1e-12
  assert (d_surface < 1e-12).sum() > len(v) // 2 and (d_cap < 1e-12).sum() > 48
  assert geometry.mesh_convexity(v, tri) > 0
  doc = Document()
  mesh = make.makeTessellated(doc, cc.conicoid(doc, 'C', cc.R0, K, H, **cc.PLACEMENTS[1]), 24)
  assert len(mesh.Triangles) > 300


LENSES = {'biconvex': dict(radius1=30.0, conic1=-0.6, radius2=-45.0, conic2=-3.0, thickness=6.0, diameter=20.0),
          'plano-hyperbolic': dict(radius1=20.0, conic1=-2.25, radius2=float('inf'), conic2=0.0, thickness=6.0, diameter=30.0),
          'meniscus': dict(radius1=25.0, conic1=-1.0, radius2=40.0, conic2=0.5, thickness=4.0, diameter=24.0)}


@pytest.mark.parametrize('kind', list(LENSES))
def test_conic_lens(native_lib, kind):
  """the baked solid of make.makeConicLens against rho <= D / 2, sag1(rho) <= z <= t + sag2(rho)"""
  from freecad.optics_design_workbench_amd import _native
  spec = LENSES[kind]
  pl = cc.PLACEMENTS[1]
  doc, src = cc.document([('Lens', lambda d: [make.makeConicLens(d, 'L', **spec, **pl)], dict(RefractiveIndex=1.5))])
  sc = bake.bakeScene(doc, src)
  kinds = sorted(sc.prim_type)
  assert kinds == {'biconvex': [geometry.CYLINDER, 8, 8], 'plano-hyperbolic': [geometry.CYLINDER, 8], 'meniscus': [geometry.CYLINDER, 8, 8]}[kind]
  assert doc.L.TypeId == ('Part::Cut' if kind == 'meniscus' else 'Part::MultiCommon')
  assert _native.build_check(sc, bake.Limits(dist_tol=1e-6))['dead_primitives'] == 0
  rng = np.random.default_rng(4)
  xl = rng.uniform([-16, -16, -4], [16, 16, 12], (20000, 3))
  xw = np.array([Placement(**pl) * p for p in xl])
  direct = cc.conic_lens_member(xl, **spec)
  assert np.array_equal(cc.feature_member(doc.L)(xw), direct)
  got, near = _member(sc, xw)
  keep = (near > 10 * cc.DIST_TOL) & cc.conic_lens_margin(xl, **spec)
  assert keep.sum() > 19800 and np.array_equal(got[keep], direct[keep]) and 500 < direct.sum() < 8000
  # no two faces of the operands coincide: every plane of the blank lies clear of the conicoids' caps and vertices
  caps = []
  for p in range(sc.n_prims):
    m = np.linalg.inv(Placement(**pl).m) @ sc.prim_to_world[p].m                   # the operand's frame in the lens's
    z0, zdir, h = m[2, 3], m[2, 2], sc.prim_params[p][1 if sc.prim_type[p] == geometry.CYLINDER else 2]
    caps.append(sorted([z0, z0 + zdir * h]) if sc.prim_type[p] == geometry.CYLINDER else [z0 + zdir * h])
  planes = np.sort(np.concatenate(caps))
  assert np.diff(planes).min() > 1e-3, planes


def test_conic_lens_refusals():
  doc = Document()
  with pytest.raises(ValueError, match='does not reach the edge'):
    make.makeConicLens(doc, 'A', 10.0, 0.0, float('inf'), 0.0, 5.0, 20.5)
  with pytest.raises(ValueError, match='beyond its equator'):                       # a ball lens: more than a half
    make.makeConicLens(doc, 'B', 10.0, 0.0, -10.0, 0.0, 20.0, 19.0)
  with pytest.raises(ValueError, match='edge thickness'):
    make.makeConicLens(doc, 'C', 20.0, -2.25, float('inf'), 0.0, 3.0, 30.0)
  assert not doc.Objects                                                          # (nothing half built)


def test_refusals_by_name(native_lib):
  from freecad.optics_design_workbench_amd.freecad_elements import surface_fans, surface_source
  K, H = cc.CASES[0]
  par = (cc.R0, K, H, cc.rim_of(cc.R0, K, H))
  with pytest.raises(UnsupportedGeometry, match='conicoid'):
    surface_source.faceArea(geometry.CONICOID, par, 0)
  with pytest.raises(UnsupportedGeometry, match='conicoid'):
    surface_fans._primitive_faces(geometry.CONICOID, par, Placement(), ['Face1'], 1e-6)
  with pytest.raises(UnsupportedGeometry, match='conicoid'):
    surface_fans._primitive_face_table(geometry.CONICOID, par, Placement(), 1e-6)
  proxy = {'module': 'freecad.optics_design_workbench.freecad_elements.surface_source', 'class': 'SurfaceSourceProxy', 'state': {}}
  # a surface source on a conicoid, and on a box that a conicoid trims
  for elems, active in ((lambda d: [cc.conicoid(d, 'S', cc.R0, K, H)], 'Face1'),
                        (lambda d: [make.makeCut(d, cc.centred_box(d, 'B', *cc.BLOCK), cc.conicoid(d, 'C', cc.R0, K, H), name='S')], 'Face6')):
    doc, _ = cc.document([('Vacuum', elems, {})])
    src = doc.addObject('App::LinkGroupPython', 'Surf', Proxy=proxy, ActiveSurfaces=[(doc.S, [active])], PowerDensity='1', Wavelength=500.0,
                        ThetaDomain='0, pi/4')
    with pytest.raises(UnsupportedGeometry, match='conicoid'):
      surface_source.bakeSurfaceSource(doc, src)
  # ... while a box face that a conicoid trims does get its fan grid: the containment tests know the kind.  The
  # conicoid here is an operand without faces of its own (a tool that only trims, as the BRep reader makes them)
  lo, hi = cc.BLOCK
  tree = geometry.Node('cut', children=[
      geometry.Node('prim', placement=Placement(base=tuple(lo)), kind=geometry.BOX, params=tuple(hi - lo) + (0.0,), source='B'),
      geometry.Node('prim', kind=geometry.CONICOID, params=par, source='C', facemask=0)], source='S')
  views = surface_fans._boolean_faces(tree, Placement(), 1e-6)
  assert len(views) == 6
  top = [v for v in views if abs(v.value(*np.mean(np.reshape(v.range, (2, 2)), axis=1))[2] - hi[2]) < 1e-12]
  assert len(top) == 1
  # the top face z = 5 of the block without the disc the conicoid takes out of it
  r5 = cc.rim_of(cc.R0, K, hi[2])
  assert abs(top[0].area - (40.0 * 40.0 - np.pi * r5 * r5)) < 0.02 * 1600.0
  grid = surface_fans.makeSurfaceGrid(top[0], 400, 1e-6)
  pts = np.array([g[1] for g in grid], float).reshape(-1, 3)
  assert len(pts) > 100 and np.all(np.hypot(pts[:, 0], pts[:, 1]) >= r5 - 1e-6) and np.abs(pts[:, 2] - hi[2]).max() < 1e-12

  class FP:
    kind, params, to_world = geometry.CONICOID, par, Placement()
  for xq, inside, strictly in (([0, 0, 4.0], True, True), ([0, 0, -1e-7], True, False), ([0, 0, -1e-5], False, False), ([0, 0, 8.0 + 1e-7], True, False),
                               ([cc.rim_of(cc.R0, K, 4.0) + 1e-7, 0, 4.0], True, False), ([cc.rim_of(cc.R0, K, 4.0) - 1e-5, 0, 4.0], True, True),
                               ([0, 0, 2 * cc.R0 / (1 + K) - 1.0], False, False)):              # (inside the absent sheet)
    assert surface_fans._inside_primitive(FP, xq, 1e-6) == inside and surface_fans._strictly_inside_primitive(FP, xq, 1e-6) == strictly, xq


def test_sets_exclude_nothing_and_references_meet_their_foci():
  """the line sets of the device tests: the numpy reference leaves none out; its mirror and lens constructions meet
  their foci within 1e-12 mm"""
  for (K, H), name in zip(cc.CASES, cc.IDS):
    O, D, want, excluded, counts = cc.crossing_lines(K, H)
    hyper = K < -1
    assert excluded.sum() == 0 and counts['lines'] == (35 if hyper else 30) and counts['one'] == 6, name
    # nothing: the two lines outside the rim, the one that clears the surface; and through the absent sheet
    assert counts['none'] == (5 if hyper else 3)
    assert all(len(w) == 2 for w in want[:counts['first_inside']][:20]) and [len(w) for w in want[20:24]] == [0, 0, 0, 2]
    inside = want[counts['first_inside']:counts['first_inside'] + 6]
    assert all(len(w) == 1 for w in inside) and all(abs(w[0][2] - H) < 1e-14 for w in inside[:3]) and all(w[0][2] < H for w in inside[3:])
    if hyper:
      assert [len(w) for w in want[-5:]] == [2, 2, 2, 0, 0]
    pts = np.vstack([w for w in want if len(w)])
    assert np.abs(np.where(np.abs(pts[:, 2] - H) < 1e-14, 0.0, cc.q_of(pts, cc.R0, K))).max() < 1e-11
  for case in cc.TRIMS:
    o, d = cc.trim_lines(case)
    want, excluded = cc.trim_expected(case, o, d)
    assert excluded.sum() == 0 and sum(len(w) > 0 for w in want) > 700 and sum(len(w) == 4 for w in want) == {'cut-block': 49, 'cut-conicoid': 111, 'common': 0}[case]
    pts = np.vstack([w for w in want if len(w)])
    assert np.abs(cc.trim_distance(case, pts)).max() < 1e-12
  for concave in (False, True):
    o, d = cc.mirror_concave_rays() if concave else cc.mirror_convex_rays()
    x, r, miss = cc.mirror_reference(o, d, concave)
    assert len(o) == 4100 and np.isfinite(x).all() and miss.max() < 1e-12
    assert np.abs(cc.q_of(x, cc.MIRROR['R'], cc.MIRROR['K'])).max() < 1e-12 and cc.rim_distance(x, **cc.MIRROR).min() > 1.0
  o, d = cc.lens_rays()
  x, r, miss = cc.lens_reference(o, d)
  assert len(o) == 4100 and miss.max() < 1e-12 and r[:, 2].max() < -0.8
  assert abs(cc.E - np.sqrt(-cc.MIRROR['K'])) == 0 and cc.LENS['R'] == cc.LENS['f'] * (cc.LENS['n'] - 1) and cc.LENS['K'] == -cc.LENS['n']**2
