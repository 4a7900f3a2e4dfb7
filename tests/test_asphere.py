"""The even asphere (primitive kind 9: the slug rho <= rim, sag(rho) <= z <= H under a conic plus even polynomial sag)
without a GPU: the numpy references of the device tests against each other on the closed-form members, the bake of
make.makeAsphere and make.makeAsphericLens, membership against the definition of the solid, the tessellation, every
refusal through `odw_build_check` and through scene/geometry.py, what stays refused by name, scenes without aspheres
against their tables and header text, and the compiled header of an asphere scene built for gfx950."""
import numpy as np
import pytest

import asphere_cases as ac
from freecad.optics_design_workbench_amd.freecad_elements import make
from freecad.optics_design_workbench_amd.scene import Document, bake, geometry
from freecad.optics_design_workbench_amd.scene.geometry import UnsupportedGeometry
from freecad.optics_design_workbench_amd.scene.placement import Placement


def _local(sc, p, x):
  m = np.asarray(sc.prim_xform[p], float).reshape(3, 4)          # global -> local
  return x @ m[:, :3].T + m[:, 3]


def _spec_of(sc, p):
  par = np.asarray(sc.prim_params[p], float)
  return dict(c=par[0], K=par[1], H=par[2], rim=par[3], coefs=tuple(sc.prim_coef[p]))


# ---- the references against each other ------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(ac.MEMBERS))
def test_references_agree_on_closed_form_members(name):
  """bracketing + bisection against the quadratic, on the lines of the device test: same counts, points within 1e-12,
  and the bisection source excludes no line.  (A check of the references of tests/asphere_cases.py themselves: it runs
  no code of the feature)"""
  spec, o, d, want = ac.member_lines(name)
  got, excluded = ac.expected(o, d, spec)
  assert excluded.sum() == 0
  assert [len(g) for g in got] == [len(w) for w in want] and sum(len(w) for w in want) > 30
  worst = max(np.abs(g - w).max() for g, w in zip(got, want) if len(w))
  assert worst < 1e-12, worst


def test_sag_forms_agree():
  """the sag of geometry.py, of the cases module, and the closed forms of the members"""
  rho = np.linspace(0, 10, 501)
  for spec in list(ac.MEMBERS.values()) + [ac.GENERAL, ac.MOAT]:
    a = geometry.asphere_sag(rho, spec['c'], spec['K'], spec['coefs'])
    assert np.abs(a - ac.sag(rho, spec)).max() < 1e-15
    h = 1e-6
    num = (ac.sag_u(rho**2 + h, spec['c'], spec['K'], spec['coefs']) - ac.sag_u(rho**2 - h, spec['c'], spec['K'], spec['coefs'])) / (2 * h)
    assert np.abs(num[1:] - geometry.asphere_sag_du(rho, spec['c'], spec['K'], spec['coefs'])[1:]).max() < 1e-8
  for name in ('a1-alone', 'conic-plus-a1'):
    assert np.abs(ac.sag(rho, ac.MEMBERS[name]) - ac.PARABOLA_A * rho**2).max() < 1e-15
  assert np.abs(ac.sag(rho, ac.MEMBERS['sphere']) - (20.0 - np.sqrt(400.0 - rho**2))).max() < 1e-14
  for K in ac.CONIC_KS:                                      # the conicoid's surface: rho^2 = 2 R z - (1 + K) z^2
    z = geometry.asphere_sag(rho[:450], 1.0 / ac.CONIC_R, K, ())
    assert np.abs(rho[:450]**2 - (2.0 * ac.CONIC_R * z - (1.0 + K) * z * z)).max() < 1e-12
  x4 = ac.moat_abscissae()
  assert np.abs(ac.sag(np.abs(x4), ac.MOAT) - ac.MOAT_Z).max() < 1e-15


def test_general_lines_are_all_held():
  """the bisection source excludes none of the explicit lines; the written-down expectations lie on the solid's
  boundary.  (A check of the references themselves: it runs no code of the feature)"""
  O, D, want, excluded = ac.crossing_lines()
  assert excluded.sum() == 0 and len(O) == len(want) > 30
  assert sum(len(w) == 0 for w in want) >= 3 and sum(len(w) == 1 for w in want) >= 5
  pts = np.vstack([w for w in want if len(w)])
  assert np.abs(ac.distance(pts, ac.GENERAL)).max() < 2e-9


# ---- bake ------------------------------------------------------------------------------------------------------------
def test_bake_of_an_asphere(native_lib):
  from freecad.optics_design_workbench_amd import _native
  pl = ac.PLACEMENTS[1]
  sc, lim = ac.vacuum(lambda d: [ac.asphere(d, 'A', ac.GENERAL, **pl)])
  assert list(sc.prim_type) == [geometry.ASPHERE] == [9] == [_native.PRIM_ASPHERE] and geometry.KIND_NAMES[9] == 'asphere'
  assert np.array_equal(sc.prim_params[0], [0.05, -0.8, 6.0, 10.0])
  assert sc.prim_coef.shape == (1, 8) and np.array_equal(sc.prim_coef[0], [0.0, 1e-5, -2e-8, 3e-11, 0, 0, 0, 0])
  assert ((int(sc.prim_flags[0]) >> 8) & 0xff) == 0b111 and not int(sc.prim_flags[0]) & _native.FLAG_CONVEX
  info = _native.build_check(sc, lim)
  assert info['structure'] in ('grid', 'bvh') and info['primitives'] == 1 and info['dead_primitives'] == 0
  # membership of random points, from the flat tables, against the definition; the distance rule's sign
  rng = np.random.default_rng(5)
  x = rng.uniform(-12, 12, (20000, 3)) + [0, 0, 3.0]
  w = np.array([Placement(**pl) * p for p in x])
  q = _local(sc, 0, w)
  assert np.abs(q - x).max() < 1e-12
  sd = ac.distance(q, _spec_of(sc, 0))
  direct = ac.member(x, ac.GENERAL)
  keep = np.abs(sd) > 10 * ac.DIST_TOL
  assert keep.sum() > 19900 and np.array_equal(sd[keep] < 0, direct[keep]) and 500 < direct.sum() < 10000
  # the box: the disc from the conservative lowest sag to H, around surface, wall and cap
  lo, hi = geometry.local_bounds(geometry.ASPHERE, (0.05, -0.8, 6.0, 10.0) + tuple(sc.prim_coef[0]))
  assert np.array_equal(hi, [10.0, 10.0, 6.0]) and lo[0] == lo[1] == -10.0 and -0.01 < lo[2] <= 0.0
  flo, fhi = geometry.face_local_bounds(geometry.ASPHERE, (0.05, -0.8, 6.0, 10.0) + tuple(sc.prim_coef[0]), 2)
  assert flo[2] == fhi[2] == 6.0
  # vertexRadius instead of curvature: exactly one of the two
  d = Document()
  assert make.makeAsphere(d, 'B', vertexRadius=20.0, semiDiameter=5.0, height=2.0).Curvature == 0.05
  assert make.makeAsphere(d, 'C', vertexRadius=float('inf'), semiDiameter=5.0, height=2.0).Curvature == 0.0
  for kw in (dict(), dict(curvature=0.05, vertexRadius=20.0)):
    with pytest.raises(ValueError, match='one of the two'):
      make.makeAsphere(d, 'D', semiDiameter=5.0, height=2.0, **kw)
  with pytest.raises(ValueError, match='eight'):
    make.makeAsphere(d, 'E', curvature=0.0, coefficients=[0.0] * 9)
  # a scene without aspheres keeps the field NULL
  plain, _ = ac.vacuum(lambda doc: [make.makeSphere(doc, 'S', 5.0)])
  assert plain.prim_coef is None and not _native.scene_desc(plain)[0].prim_coef
  assert bool(_native.scene_desc(sc)[0].prim_coef)


def test_bake_of_booleans_and_the_lens(native_lib):
  """trimming lists of Cut and Common; the singlet is the Common of two slugs, one turned round, and its membership is
  the defining inequality of make.makeAsphericLens"""
  from freecad.optics_design_workbench_amd import _native
  sc, lim = ac.trim_scene('cut-block')
  assert list(sc.prim_type) == [0, 9] and int(sc.prim_flags[1]) & 1 and ((int(sc.prim_flags[1]) >> 8) & 0xff) == 0b011
  assert list(sc.cond_prim) == [1, 0] and list(sc.cond_inside) == [0, 1]
  sc, lim = ac.trim_scene('common')
  assert list(sc.prim_type) == [9, 0] and list(sc.cond_prim) == [1, 0] and list(sc.cond_inside) == [1, 1]
  assert ((int(sc.prim_flags[0]) >> 8) & 0xff) == 0b011                       # (the cap lies above the box)
  front = dict(vertexRadius=20.0, conicConstant=-0.8, coefficients=(0.0, 1e-5, -2e-8, 3e-11))
  back = dict(curvature=-1.0 / 35.0, conicConstant=0.3, coefficients=(0.0, -4e-6))
  t, dia = 5.0, 18.0
  sc, lim = ac.baked([('Lens', lambda d: [make.makeAsphericLens(d, 'L', front=front, back=back, thickness=t, diameter=dia)], {})])
  assert list(sc.prim_type) == [9, 9] and list(sc.cond_prim) == [1, 0] and list(sc.cond_inside) == [1, 1]
  assert not any(int(f) & _native.FLAG_CONVEX for f in sc.prim_flags) and not any(int(f) & 1 for f in sc.prim_flags)
  assert np.array_equal(sc.prim_params[0][[0, 1, 3]], [0.05, -0.8, 9.0]) and np.array_equal(sc.prim_coef[0][:4], front['coefficients'])
  # the back slug, turned round: the opposite sag, one per cent wider than the lens
  assert np.array_equal(sc.prim_params[1][[0, 1]], [1.0 / 35.0, 0.3]) and abs(sc.prim_params[1][3] - 9.09) < 1e-12
  assert np.array_equal(sc.prim_coef[1][:2], [0.0, 4e-6])
  assert all(((int(f) >> 8) & 4) == 0 for f in sc.prim_flags)                 # (neither cap is a face of the lens)
  assert _native.build_check(sc, lim)['dead_primitives'] == 0
  rng = np.random.default_rng(6)
  x = rng.uniform(-11, 11, (20000, 3)) + [0, 0, 2.5]
  rho = np.hypot(x[:, 0], x[:, 1])
  with np.errstate(invalid='ignore'):
    s1 = geometry.asphere_sag(np.minimum(rho, 9.0), 0.05, -0.8, front['coefficients'])
    s2 = geometry.asphere_sag(np.minimum(rho, 9.0), back['curvature'], 0.3, back['coefficients'])
  direct = (rho < 9.0) & (x[:, 2] > s1) & (x[:, 2] < t + s2)
  sd = np.maximum(ac.distance(_local(sc, 0, x), _spec_of(sc, 0)), ac.distance(_local(sc, 1, x), _spec_of(sc, 1)))
  keep = np.abs(sd) > 10 * ac.DIST_TOL
  assert keep.sum() > 19900 and np.array_equal(sd[keep] < 0, direct[keep]) and 300 < direct.sum() < 10000
  with pytest.raises(ValueError, match='meet inside'):
    make.makeAsphericLens(Document(), 'X', front=dict(vertexRadius=20.0), back=dict(vertexRadius=-20.0), thickness=1.0, diameter=18.0)


def test_link_scale_magnifies_the_prescription():
  """z = sag(rho) magnified by s: curvature / s, K, lengths s, a_i s^(1 - 2 i)"""
  node = geometry.Node('prim', kind=geometry.ASPHERE, params=(0.05, -0.8, 6.0, 10.0) + ac.coefs8(ac.GENERAL['coefs']))
  big = geometry._scaled([node], 2.0)[0]
  rho = np.linspace(0, 20, 101)
  s = geometry.asphere_sag(rho, big.params[0], big.params[1], big.params[4:])
  assert big.params[2:4] == (12.0, 20.0) and np.abs(s - 2.0 * ac.sag(rho / 2.0, ac.GENERAL)).max() < 1e-14


# ---- tessellation ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('spec', [ac.GENERAL, ac.MOAT], ids=['general', 'moat'])
def test_tessellation(spec):
  """rings on the surface (1e-12), wall, cap; a closed mesh with every facet wound outward"""
  params = (spec['c'], spec['K'], spec['H'], spec['rim']) + ac.coefs8(spec['coefs'])
  v, tri, vn = geometry.tessellate(geometry.ASPHERE, params, 96)
  rho = np.hypot(v[:, 0], v[:, 1])
  on_cap, on_wall = np.abs(v[:, 2] - spec['H']) < 1e-12, np.abs(rho - spec['rim']) < 1e-12
  on_surface = np.abs(v[:, 2] - ac.sag(np.minimum(rho, spec['rim']), spec)) < 1e-12
  assert np.all(on_cap | on_wall | on_surface) and on_surface.sum() > 500 and on_cap.sum() > 100
  assert np.abs(np.linalg.norm(vn, axis=1) - 1.0).max() < 1e-12
  # outward: a step along the facet's normal from its centroid leaves the solid, a step back enters it (the step is
  # longer than the rings' chords lie off the surface: rim^2 / 24^2 * curvature / 8 < 0.02 mm on both profiles)
  c = v[tri].mean(axis=1)
  n = np.cross(v[tri[:, 1]] - v[tri[:, 0]], v[tri[:, 2]] - v[tri[:, 0]])
  n /= np.linalg.norm(n, axis=1)[:, None]
  eps = 0.05
  assert not ac.member(c + eps * n, spec).any()
  assert ac.member(c - eps * n, spec).mean() > 0.97                         # (all but facets at the edges)
  assert (n * vn[tri].mean(axis=1)).sum(1).min() > 0.9
  # closed: every edge is shared by two facets (vertices welded by position)
  key = {tuple(np.round(p, 9)): i for i, p in enumerate(v)}
  ids = np.array([key[tuple(np.round(p, 9))] for p in v])[tri]
  edges = np.sort(np.concatenate([ids[:, [0, 1]], ids[:, [1, 2]], ids[:, [2, 0]]]), axis=1)
  edges = edges[edges[:, 0] != edges[:, 1]]
  _, cnt = np.unique(edges, axis=0, return_counts=True)
  assert np.all(cnt == 2)
  # make.makeTessellated takes the solid
  d = Document()
  mesh = make.makeTessellated(d, ac.asphere(d, 'A', spec), 24)
  assert mesh is not None


# ---- refusals ------------------------------------------------------------------------------------------------------------
BAD = [
    (dict(c=float('nan')), 'finite'),
    (dict(K=float('inf')), 'finite'),
    (dict(H=float('nan')), 'finite'),
    (dict(coefs=(0.0, float('nan'))), 'finite'),
    (dict(rim=0.0), 'semi-diameter'),
    (dict(rim=-2.0), 'semi-diameter'),
    (dict(c=0.1, K=0.0, rim=9.95, H=9.5), '0.98'),
    (dict(H=1.0), 'height'),
    (dict(H=float(ac.sag(10.0, ac.GENERAL))), 'height'),
]


@pytest.mark.parametrize('change, word', BAD, ids=[str(i) for i in range(len(BAD))])
def test_refusals(native_lib, change, word):
  """every refusal of the library through odw_build_check (return code and message), and geometry.py raising
  UnsupportedGeometry for the same input, in words"""
  from freecad.optics_design_workbench_amd import _native
  spec = dict(ac.GENERAL, **change)
  sc, lim = ac.vacuum(lambda d: [ac.asphere(d, 'A', ac.GENERAL)])
  sc.prim_params = np.array([[spec['c'], spec['K'], spec['H'], spec['rim']]])
  sc.prim_coef = np.array([ac.coefs8(spec['coefs'])])
  with pytest.raises(_native.NativeError, match=r'(?s)invalid.*asphere.*' + word):
    _native.build_check(sc, lim)
  with pytest.raises(UnsupportedGeometry, match=r'(?s)asphere.*' + word):
    ac.vacuum(lambda d: [ac.asphere(d, 'A', spec)])


def test_refusals_of_the_descriptor(native_lib):
  from freecad.optics_design_workbench_amd import _native
  sc, lim = ac.vacuum(lambda d: [ac.asphere(d, 'A', ac.GENERAL)])
  assert _native.build_check(sc, lim)['primitives'] == 1
  sc.prim_flags = np.array([0xf << 8], dtype=np.int32)
  with pytest.raises(_native.NativeError, match=r'(?s)unsupported.*asphere.*faces'):
    _native.build_check(sc, lim)
  sc.prim_flags = np.array([7 << 8], dtype=np.int32)
  sc.prim_coef = None
  with pytest.raises(_native.NativeError, match=r'(?s)unsupported.*asphere.*prim_coef'):
    _native.build_check(sc, lim)
  sc.prim_coef = np.zeros((2, 8))
  with pytest.raises(ValueError, match='prim_coef'):
    _native.scene_desc(sc)
  sc.prim_type = np.array([10], dtype=np.int32)
  sc.prim_coef = np.zeros((1, 8))
  with pytest.raises(_native.NativeError, match='unknown primitive type'):
    _native.build_check(sc, lim)


def test_refused_by_name_as_sources():
  from freecad.optics_design_workbench_amd.freecad_elements import surface_fans, surface_source
  params = (0.05, -0.8, 6.0, 10.0) + ac.coefs8(ac.GENERAL['coefs'])
  with pytest.raises(UnsupportedGeometry, match='asphere as a surface source'):
    surface_source.faceArea(geometry.ASPHERE, params, 0)
  with pytest.raises(UnsupportedGeometry, match='asphere as fan grids'):
    surface_fans._primitive_face_table(geometry.ASPHERE, params, Placement(), 1e-6)
  fp = geometry.FlatPrim(geometry.ASPHERE, params, Placement(), False, [[]], 7, 'A')
  for f in (surface_fans._inside_primitive, surface_fans._strictly_inside_primitive):
    with pytest.raises(UnsupportedGeometry, match='trimmed by an asphere'):
      f(fp, np.zeros(3), 1e-6)


# ---- scenes without aspheres; the compiled header ---------------------------------------------------------------------
def test_scenes_without_aspheres_are_what_they_were(native_lib):
  """the value image and the header text of scenes that hold no asphere do not depend on the new descriptor field: a
  descriptor with a prim_coef table (rows ignored) gives the same image, offsets and header as one without.  A proxy,
  inside this tree, for "the same as before": the comparison with the parent commit's own header text and code size is
  the record in profiles/asphere.md (lensesAndMirrors), and the existing image tests (tests/test_spec_image.py) hold
  the layout of such scenes to the operations written out"""
  import copy
  from freecad.optics_design_workbench_amd import _native
  from conicoid_cases import CASES, R0, conicoid
  sc, lim = ac.baked([('Lens', lambda d: [make.makeCommon(d, [make.makeSphere(d, 'S', 8.0, base=(0, 0, 3)), make.makeCylinder(d, 'C', 5.0, 9.0)]),
                                         conicoid(d, 'K', R0, *CASES[0], base=(30, 0, 0))], {})])
  assert sc.prim_coef is None
  a = _native.spec_image(sc, lim)
  head_a, bytes_a = _native.compile_check(sc, lim, 'structure')
  assert 'rare() { return 4; }' in head_a
  other = copy.copy(sc)
  other.prim_coef = np.full((sc.n_prims, 8), 0.37)
  b = _native.spec_image(other, lim)
  head_b, bytes_b = _native.compile_check(other, lim, 'structure')
  assert head_a == head_b and bytes_a == bytes_b
  assert np.array_equal(a['image'], b['image']) and all(np.array_equal(a[k], b[k]) for k in ('frame', 'par', 'box', 'der'))
  assert list(np.diff(a['par'])) == [int(a['par'][k + 1] - a['par'][k]) for k in range(sc.n_prims - 1)]
  assert _native.build_check(sc, lim) == _native.build_check(other, lim)


def test_compiled_header_of_an_asphere_scene(native_lib):
  """rare() carries bit 3, the parameter block is 4 + 12 words with the coefficients and bounds in it, three derived
  words built with the device's operations; the header compiles for gfx950"""
  from freecad.optics_design_workbench_amd import _native
  sc, lim = ac.baked([('Lens', lambda d: [ac.asphere(d, 'A', ac.GENERAL, base=(0, 0, 2.0)), make.makeSphere(d, 'S', 3.0, base=(30, 0, 0))], {})])
  head, code_bytes = _native.compile_check(sc, lim, 'structure')
  assert 'rare() { return 8; }' in head and code_bytes > 10000
  im = _native.spec_image(sc, lim)
  img, par, der = im['image'], int(im['par'][0]), int(im['der'][0])
  assert int(im['box'][0]) == par + 16
  assert np.array_equal(img[par:par + 4], [0.05, -0.8, 6.0, 10.0]) and np.array_equal(img[par + 4:par + 12], ac.coefs8(ac.GENERAL['coefs']))
  M, L, z_min, top = geometry.asphere_bounds(0.05, -0.8, 10.0, ac.GENERAL['coefs'])
  assert np.allclose(img[par + 12:par + 15], [M, L, z_min], rtol=1e-12, atol=1e-15) and img[par + 15] == 0.0
  tol = lim.dist_tol
  assert list(img[der:der + 3]) == [6.0 + tol, (10.0 + tol) * (10.0 + tol), 100.0]
  # the bounds bound: sampled |s_rr|, |s_r / r|, |s_r| over the disc
  rho = np.linspace(1e-6, 10.0 * 1.001, 4001)
  s1 = geometry.asphere_sag_du(rho, 0.05, -0.8, ac.GENERAL['coefs'])
  s_r = 2.0 * rho * s1
  s_rr = np.gradient(s_r, rho)
  assert L >= np.abs(s_r).max() and M >= np.abs(2.0 * s1).max() and M >= np.abs(s_rr[2:-2]).max() * (1 - 1e-6)
  assert 6.0 > top > float(ac.sag(10.0, ac.GENERAL)) and z_min <= 0.0
