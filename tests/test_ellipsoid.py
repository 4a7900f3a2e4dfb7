"""Part::Ellipsoid without a GPU: the bake (FreeCAD's own construction of the solid: radii, latitude segment, sweep),
the flat tables against the inequalities they stand for, the host builders and the compiler of scene kernels
(`odw_build_check`, `odw_compile_check`: no device needed), the tessellation, and what stays refused by name."""
import copy

import numpy as np
import pytest

import ellipsoid_cases as ec
from conftest import project
from freecad.optics_design_workbench_amd.freecad_elements import make
from freecad.optics_design_workbench_amd.scene import Document, bake, geometry
from freecad.optics_design_workbench_amd.scene.geometry import UnsupportedGeometry
from freecad.optics_design_workbench_amd.scene.placement import Placement


def _local(sc, p, x):
  m = np.asarray(sc.prim_xform[p], float).reshape(3, 4)          # global -> local
  return x @ m[:, :3].T + m[:, 3]


def _sdist(sc, p, x):
  """distance of the points x from primitive p of the flat tables: box exactly, ellipsoid to first order"""
  q, par = _local(sc, p, x), np.asarray(sc.prim_params[p], float)
  if sc.prim_type[p] == geometry.BOX:
    return ec.box_distance(q, np.zeros(3), par[:3])
  assert sc.prim_type[p] == geometry.ELLIPSOID
  return ec.first_order_distance(q, par[:3])


def _member(sc, x):
  """a conjunction of primitives, as these solids are: inside every primitive, outside the flipped ones (Cut tools);
  and every literal of every trimming list asks for that same side of its operand"""
  flip = (np.asarray(sc.prim_flags) & 1).astype(bool)
  for p in range(sc.n_prims):
    for c in range(sc.prim_cond_off[p], sc.prim_cond_off[p + 1]):
      assert sc.cond_prim[c] != p and bool(sc.cond_inside[c] & 1) == (not flip[sc.cond_prim[c]])
  sd = np.array([_sdist(sc, p, x) for p in range(sc.n_prims)])
  inside = np.all(np.where(flip[:, None], sd > 0, sd < 0), axis=0)
  return inside, np.abs(sd).min(axis=0)


def test_bake_and_build(native_lib):
  from freecad.optics_design_workbench_amd import _native
  # ---- radii by FreeCAD's construction: rx = Radius2, ry = Radius3 (0: Radius2), rz = Radius1
  sc, lim = ec.vacuum(lambda d: [make.makeEllipsoid(d, 'E', 50.0, 30.0, 20.0), make.makeEllipsoid(d, 'F', 50.0, 30.0, 0.0, base=(200, 0, 0)),
                                 make.makeEllipsoid(d, 'G', base=(0, 300, 0))])
  assert list(sc.prim_type) == [geometry.ELLIPSOID] * 3 == [7] * 3
  assert np.array_equal(sc.prim_params, [[30.0, 20.0, 50.0, 0.0], [30.0, 30.0, 50.0, 0.0], [4.0, 4.0, 2.0, 0.0]])
  assert all(((f >> 8) & 0xff) == 1 and f & _native.FLAG_CONVEX for f in sc.prim_flags)         # one face; convex
  # ---- latitude segment and sweep, before the scaling
  doc = Document()
  seg = geometry._primitive_of(make.makeEllipsoid(doc, 'S', 50.0, 30.0, 20.0, angle1=-30.0, angle2=60.0, angle3=120.0))
  assert seg.op == 'common' and [k.kind for k in seg.children] == [geometry.ELLIPSOID, geometry.BOX, geometry.BOX, geometry.BOX]
  slab = seg.children[1]
  assert abs(slab.placement.m[2, 3] - 50.0 * np.sin(np.radians(-30.0))) < 1e-12
  assert abs(slab.placement.m[2, 3] + slab.params[2] - 50.0 * np.sin(np.radians(60.0))) < 1e-12
  assert slab.params[0] >= 2 * 50.0 and -slab.placement.m[0, 3] >= 50.0
  azimuth = lambda n: np.degrees(np.arctan2(n.placement.m[1, 0], n.placement.m[0, 0]))
  assert abs(azimuth(seg.children[2])) < 1e-12
  # the plane at 120 degrees on the sphere of radius rx, scaled by ry / rx in y: through (rx cos, ry sin)
  want = np.degrees(np.arctan2(20.0 * np.sin(np.radians(120.0)), 30.0 * np.cos(np.radians(120.0))))
  assert abs(azimuth(seg.children[3]) - (want - 180.0)) < 1e-9 and abs(want - 120.0) > 5
  # ... and as a solid: membership of points against the construction itself (unit sphere, then the scaling)
  rng = np.random.default_rng(3)
  x = rng.uniform(-55, 55, (20000, 3))
  u = x / np.array([30.0, 20.0, 50.0])                             # back on the unit sphere
  az = np.degrees(np.arctan2(u[:, 1], u[:, 0])) % 360.0
  direct = ((u * u).sum(1) < 1) & (u[:, 2] > np.sin(np.radians(-30.0))) & (u[:, 2] < np.sin(np.radians(60.0))) & (az < 120.0)
  scs, _ = ec.vacuum(lambda d: [make.makeEllipsoid(d, 'S', 50.0, 30.0, 20.0, angle1=-30.0, angle2=60.0, angle3=120.0)])
  got, near = _member(scs, x)
  keep = near > 10 * ec.DIST_TOL
  assert keep.sum() > 19900 and np.array_equal(got[keep], direct[keep]) and 500 < direct.sum() < 5000
  with pytest.raises(UnsupportedGeometry):
    ec.vacuum(lambda d: [make.makeEllipsoid(d, 'S', angle3=270.0)])
  with pytest.raises(UnsupportedGeometry):
    ec.vacuum(lambda d: [make.makeEllipsoid(d, 'S', radius1=0.0)])
  # ---- membership from the flat tables against the inequalities: alone (moved), Common and Cut with a box
  pl = ec.PLACEMENTS[1]
  P = Placement(**pl)
  alone, _ = ec.vacuum(lambda d: [ec.ellipsoid(d, 'E', ec.RADII, **pl)])
  Pi = P.inverse()
  xl = np.array([Pi * p for p in x])
  q = ((xl / np.array(ec.RADII))**2).sum(1)
  for scn, direct in ((alone, q < 1),
                      (ec.common_scene()[0], (((x / np.array(ec.RADII))**2).sum(1) < 1) & np.all((x > ec.SLAB[0]) & (x < ec.SLAB[1]), axis=1)),
                      (ec.cut_scene()[0], (((x / np.array(ec.RADII))**2).sum(1) > 1) & np.all((x > ec.CUBE[0]) & (x < ec.CUBE[1]), axis=1))):
    got, near = _member(scn, x)
    keep = near > 10 * ec.DIST_TOL
    assert keep.sum() > 19900 and np.array_equal(got[keep], direct[keep]) and 1000 < direct.sum() < 19500
  # ---- the host builders: a structure other than the flat loop, boxes around the surface, refusals
  for scn in (alone, ec.common_scene()[0], ec.cut_scene()[0]):
    info = _native.build_check(scn, lim)
    assert info['structure'] in ('grid', 'bvh') and info['primitives'] == scn.n_prims and info['dead_primitives'] == 0
  many, _ = ec.lattice_scene()
  assert many.n_prims == 75 and _native.build_check(many, lim)['structure'] in ('grid', 'bvh')
  # facets beside an ellipsoid: the binary tree (the mesh kernel's eight-wide tree does not know the kind)
  def with_mesh(extra):
    return ec.vacuum(lambda d: [make.makeTessellated(d, make.makeSphere(d, 'S', 5.0, base=(100, 0, 0)), 16)] + extra(d))[0]
  assert _native.build_check(with_mesh(lambda d: []), lim)['structure'] == 'wide-bvh'
  assert _native.build_check(with_mesh(lambda d: [ec.ellipsoid(d, 'E', ec.RADII)]), lim)['structure'] == 'bvh'
  s = rng.normal(size=(10000, 3))
  s = s / np.linalg.norm(s, axis=1)[:, None] * np.array(ec.RADII)
  lo, hi = geometry.world_aabb(alone.prim_to_world[0], *geometry.local_bounds(geometry.ELLIPSOID, alone.prim_params[0]))
  w = np.array([P * p for p in s])
  assert np.all(w >= lo) and np.all(w <= hi) and np.all(hi - lo < 2 * np.sqrt(3) * 50.0 + 1e-9)
  flo, fhi = geometry.face_local_bounds(geometry.ELLIPSOID, alone.prim_params[0], 0)
  assert np.array_equal(flo, -np.array(ec.RADII)) and np.array_equal(fhi, np.array(ec.RADII))
  capped = copy.copy(alone)
  capped.prim_flags = np.asarray(alone.prim_flags) | (0b110 << 8)          # the cap faces of a cylinder: not on this kind
  with pytest.raises(_native.NativeError, match='unsupported.*no caps'):
    _native.build_check(capped, lim)
  for bad in ((0.0, 20.0, 50.0), (30.0, -1.0, 50.0), (30.0, 20.0, float('nan'))):
    sb = copy.copy(alone)
    sb.prim_params = np.array([list(bad) + [0.0]])
    with pytest.raises(_native.NativeError, match='invalid argument'):
      _native.build_check(sb, lim)


def test_compile_tessellate_and_refusals(native_lib):
  from freecad.optics_design_workbench_amd import _native
  from freecad.optics_design_workbench_amd.freecad_elements import surface_fans, surface_source
  lim = bake.Limits(dist_tol=1e-6)
  beside = ec.vacuum(lambda d: [ec.ellipsoid(d, 'E', ec.RADII), make.makeParaboloid(d, 'P', 10.0, 5.0, base=(100, 0, 0))])[0]
  for scn, rare in ((ec.vacuum(lambda d: [ec.ellipsoid(d, 'E', ec.RADII, **ec.PLACEMENTS[1])])[0], 2), (ec.cut_scene()[0], 2), (beside, 3)):
    header, code_bytes = _native.compile_check(scn, lim, 'structure')              # (arch: gfx950)
    assert code_bytes > 10000 and f'static constexpr int rare() {{ return {rare}; }}' in header
  pr = project('lensesAndMirrors')
  header, _ = _native.compile_check(pr.scene, pr.limits, 'structure')
  assert 'static constexpr int rare() { return 0; }' in header
  # ---- tessellation: on the surface, outward gradient normals, convex; as a mesh in a document
  radii = np.array(ec.RADII)
  v, tri, vn = geometry.tessellate(geometry.ELLIPSOID, ec.RADII + (0.0,), 48)
  assert np.abs(((v / radii)**2).sum(1) - 1.0).max() < 1e-12
  g = v / radii**2
  assert np.abs(vn - g / np.linalg.norm(g, axis=1)[:, None]).max() < 1e-12
  assert geometry.mesh_convexity(v, tri) > 0
  doc = Document()
  mesh = make.makeTessellated(doc, ec.ellipsoid(doc, 'E', ec.RADII, **ec.PLACEMENTS[1]), 24)
  assert len(mesh.Triangles) > 500
  # ---- refused by name
  doc, _ = ec.document([('Vacuum', lambda d: [ec.ellipsoid(d, 'E', ec.RADII)], {})])
  with pytest.raises(UnsupportedGeometry, match='ellipsoid'):
    surface_source.faceArea(geometry.ELLIPSOID, ec.RADII + (0.0,), 0)
  src = doc.addObject('App::LinkGroupPython', 'Surf', Proxy={'module': 'freecad.optics_design_workbench.freecad_elements.surface_source',
                                                               'class': 'SurfaceSourceProxy', 'state': {}},
                      ActiveSurfaces=[(doc.E, ['Face1'])], PowerDensity='1', Wavelength=500.0, ThetaDomain='0, pi/4')
  with pytest.raises(UnsupportedGeometry, match='ellipsoid'):
    surface_source.bakeSurfaceSource(doc, src)
  with pytest.raises(UnsupportedGeometry, match='ellipsoid'):
    surface_fans._primitive_faces(geometry.ELLIPSOID, ec.RADII + (0.0,), Placement(), ['Face1'], 1e-6)
