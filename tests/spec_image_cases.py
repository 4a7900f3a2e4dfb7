"""Scenes and the operations written out for the value image of the compiled kernels (tests/test_spec_image.py,
tests/test_gpu_spec_image.py): what odw_build.h's spec_image_build must produce, in numpy float64, and the fused
multiply-add the device performs where one expression holds a product and a sum, exactly (rational arithmetic, one
rounding)."""
import types
from fractions import Fraction

import numpy as np

from freecad.optics_design_workbench_amd.freecad_elements import make
from freecad.optics_design_workbench_amd.scene import Document, bake, geometry

f64 = np.float64


def fma(a, b, c):
  """round(a * b + c) with ONE rounding (Fraction -> float rounds correctly)"""
  return f64(float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))))


def quat(axis, deg):
  a = np.asarray(axis, float)
  a = a / np.linalg.norm(a)
  h = np.radians(deg) / 2
  return tuple(np.r_[a * np.sin(h), np.cos(h)])


def baked(doc, record_all=True, **source_props):
  from freecad.optics_design_workbench_amd.freecad_elements import point_source
  src = make.makePointSource(doc, **source_props)
  sc = bake.bakeScene(doc, src)
  if record_all:
    sc.group_record = np.ones_like(sc.group_record)
  return types.SimpleNamespace(scene=sc, limits=bake.bakeLimits(doc, src), source=point_source.bakeSource(doc, src))


def zoo(rs, tol='1e-6', n_each=3):
  """every primitive kind with constants of its own, random sizes and placements (general rotations, axis-aligned
  frames, far offsets), thin boxes among them"""
  doc = Document()
  elems = []
  for k in range(n_each):
    general = dict(base=tuple(rs.uniform(-50, 50, 3)), quat=quat(rs.normal(size=3), rs.uniform(0, 360)))
    aligned = dict(base=tuple(rs.uniform(-50, 50, 3)))
    far = dict(base=(1e7 + rs.uniform(0, 1), -3e6, 2e5 + rs.uniform(0, 1)))
    pl = (general, aligned, far)[k % 3]
    elems.append(make.makeBox(doc, f'B{k}', *rs.uniform(0.5, 30, 3), **pl))
    elems.append(make.makeBox(doc, f'T{k}', rs.uniform(5, 30), rs.uniform(5, 30), 10.0 ** rs.uniform(-9, -3), **pl))   # thin
    elems.append(make.makeCylinder(doc, f'C{k}', rs.uniform(0.5, 20), rs.uniform(0.5, 30), **pl))
    elems.append(make.makeCone(doc, f'K{k}', rs.uniform(0.5, 10), rs.uniform(0.5, 10), rs.uniform(1, 30), **pl))
    elems.append(make.makeTorus(doc, f'O{k}', rs.uniform(8, 30), rs.uniform(0.5, 6), **pl))
    elems.append(make.makeSphere(doc, f'S{k}', rs.uniform(0.5, 20), **pl))
    elems.append(make.makeParaboloid(doc, f'P{k}', rs.uniform(1, 20), rs.uniform(1, 10), **pl))
  make.makeMirror(doc, elems[::2])
  make.makeLens(doc, elems[1::2], RefractiveIndex=1.0 + rs.uniform(0.2, 0.9))
  make.makeSimulationSettings(doc, DistanceTolerance=tol)
  return baked(doc)


def constant_records(pr):
  """(kind, 4 parameters, tolerance) of every primitive of a baked scene whose intersection derives constants"""
  sc = pr.scene
  keep = [p for p in range(len(sc.prim_type)) if expected_derived(int(sc.prim_type[p]), sc.prim_params[p], 1e-6)]
  rec = np.zeros((len(keep), 6), f64)
  rec[:, 0] = np.asarray(sc.prim_type)[keep]
  rec[:, 1:5] = np.asarray(sc.prim_params, f64)[keep]
  rec[:, 5] = pr.limits.dist_tol
  return keep, rec


def expected_derived(kind, par, tol):
  """the constants of one primitive: the operation sequences of intersect_prim (odw_kernels.hip)"""
  par = np.asarray(par, f64)
  tol = f64(tol)
  if kind == geometry.BOX:
    return [par[0] + tol, par[1] + tol, par[2] + tol]
  if kind == geometry.TORUS:
    R1, R2 = par[0], par[1]
    rin = fma(R1 - R2, f64(0.9999999), f64(-1e-9))
    return [fma(R1 + R2, f64(1.0000001), f64(1e-9)), fma(R2, f64(1.0000001), f64(1e-9)), rin, rin * rin]
  if kind in (geometry.CYLINDER, geometry.CONE, geometry.PARABOLOID):
    parab = kind == geometry.PARABOLOID
    R1 = f64(0.0) if parab else par[0]
    R2 = par[0] if kind == geometry.CYLINDER else (par[2] if parab else par[1])
    H = par[2] if kind == geometry.CONE else par[1]
    return [H + tol, R1 * R1 * (f64(1.0) - f64(1e-9)), (R1 + tol) * (R1 + tol), (R2 + tol) * (R2 + tol)]
  return []


def bits(a):
  return np.asarray(a, f64).view(np.uint64)


def lens_train(n_lenses, radius=30.0, tol='1e-6', tilt=12.0):
  """n biconvex lenses (sphere ^ sphere ^ cylinder each) along the z axis, a tilted mirror box beside the axis and a
  recording screen behind them: 3 n + 2 primitives"""
  doc = Document()
  lenses = []
  for j in range(n_lenses):
    z = 30.0 + 14.0 * j
    a = make.makeSphere(doc, f'A{j}', radius, base=(0, 0, z + radius - 2.0))
    b = make.makeSphere(doc, f'B{j}', radius, base=(0, 0, z - radius + 2.0))
    c = make.makeCylinder(doc, f'C{j}', 8.0, 6.0, base=(0, 0, z - 3.0))
    lenses.append(make.makeCommon(doc, [a, b, c], f'L{j}'))
  make.makeLens(doc, lenses, RefractiveIndex=1.5)
  make.makeMirror(doc, [make.makeBox(doc, 'M', 6, 40, 30, base=(11.0, -20.0, 20.0), quat=quat((0, 1, 0), tilt))])
  z_end = 30.0 + 14.0 * n_lenses + 20.0
  make.makeAbsorber(doc, [make.makeBox(doc, 'S', 160, 160, 1, base=(-80, -80, z_end))], RecordHits=True)
  make.makeSimulationSettings(doc, DistanceTolerance=tol)
  return baked(doc)


SMALL = dict(lens_z=30.0, torus_z=15.0, box_lo=(-30.0, -5.0, 40.0), box_size=(10.0, 10.0, 10.0), cyl_at=(25.0, 0.0, 40.0),
             cyl_r=4.0, cyl_h=10.0, screen_z=80.0)


def small_scene(radius=30.0, tol='1e-6', torus=(6.0, 1.5)):
  """8 primitives: one biconvex lens on the z axis, a torus in front of it (the beam goes through its hole), a tilted
  mirror box beside the axis, an axis-aligned box and an upright cylinder (absorbers) and a screen"""
  g = SMALL
  doc = Document()
  z = g['lens_z']
  a = make.makeSphere(doc, 'A', radius, base=(0, 0, z + radius - 2.0))
  b = make.makeSphere(doc, 'B', radius, base=(0, 0, z - radius + 2.0))
  c = make.makeCylinder(doc, 'C', 8.0, 6.0, base=(0, 0, z - 3.0))
  make.makeLens(doc, [make.makeCommon(doc, [a, b, c], 'L')], RefractiveIndex=1.5)
  make.makeMirror(doc, [make.makeBox(doc, 'M', 6, 40, 30, base=(11.0, -20.0, 20.0), quat=quat((0, 1, 0), 12.0)),
                        make.makeTorus(doc, 'O', torus[0], torus[1], base=(0, 0, g['torus_z']))])
  make.makeAbsorber(doc, [make.makeBox(doc, 'X', *g['box_size'], base=g['box_lo']),
                          make.makeCylinder(doc, 'Y', g['cyl_r'], g['cyl_h'], base=g['cyl_at']),
                          make.makeBox(doc, 'S', 160, 160, 1, base=(-80, -80, g['screen_z']))], RecordHits=True)
  make.makeSimulationSettings(doc, DistanceTolerance=tol)
  return baked(doc, PowerDensity='exp(-theta^2/0.02)', ThetaDomain='0, pi/8', ThetaResolutionNumericMode='2e3')


def unit(d):
  d = np.asarray(d, f64)
  return d / np.linalg.norm(d, axis=1)[:, None]      # (an exact 0 stays an exact 0)


def rays_zero_components(rs, n, zeros):
  """directions with `zeros` exact zero components; origins around the bench"""
  o = np.c_[rs.uniform(-35, 35, n), rs.uniform(-25, 25, n), rs.uniform(-5, 0, n)]
  d = np.c_[rs.normal(0, 0.15, n), rs.normal(0, 0.15, n), np.ones(n)]
  k = rs.randint(0, 3, n)
  if zeros == 1:
    d[k == 0, 0] = 0.0
    d[k == 1, 1] = 0.0
    side = k == 2                                     # travelling sideways: dz = 0
    phi = rs.uniform(0, 2 * np.pi, n)
    d[side] = np.c_[np.cos(phi), np.sin(phi), np.zeros(n)][side]
    o[side, 2] = rs.uniform(0, 90, side.sum())
  else:
    axes = np.eye(3)[k] * rs.choice([-1.0, 1.0], n)[:, None]
    d = axes + 0.0                                    # (no -0)
    o = np.c_[rs.uniform(-40, 40, n), rs.uniform(-25, 25, n), rs.uniform(-5, 90, n)]
  return o, unit(d)


def rays_special_origins(rs, n, boxes):
  """origins with coordinates exactly 0, and origins lying on a plane of a primitive's box (`boxes`: odw_spec_image's)"""
  o = np.c_[rs.uniform(-35, 35, n), rs.uniform(-25, 25, n), rs.uniform(-5, 60, n)]
  d = np.c_[rs.normal(0, 0.3, n), rs.normal(0, 0.3, n), rs.choice([-1.0, 1.0], n)]
  k = rs.randint(0, 8, n)
  for a in range(3):
    o[k == a, a] = 0.0
  o[k == 3] = 0.0
  on = k >= 4
  which = rs.randint(0, len(boxes), n)
  plane = rs.randint(0, 6, n)
  idx = np.nonzero(on)[0]
  o[idx, plane[idx] % 3] = boxes[which[idx], plane[idx]]
  g = SMALL                                           # ... and on the faces of the axis-aligned box themselves
  face = k == 7
  o[face, 0] = g['box_lo'][0] + rs.choice([0.0, g['box_size'][0]], face.sum())
  return o, unit(d)


def rays_grazing(rs, n, tol):
  """rays along box edges and cylinder rims, within +-1.5 tol of them"""
  g = SMALL
  delta = rs.uniform(-1.5, 1.5, n) * tol
  k = rs.randint(0, 6, n)
  o = np.zeros((n, 3))
  d = np.tile([0.0, 0.0, 1.0], (n, 1))
  x0, y0, z0 = g['box_lo']
  sx, sy, sz = g['box_size']
  # 0: along +z past the box's x edge; 1: past its y edge
  o[k == 0] = np.c_[x0 + rs.choice([0.0, sx], n) + delta, rs.uniform(y0, y0 + sy, n), np.zeros(n)][k == 0]
  o[k == 1] = np.c_[rs.uniform(x0, x0 + sx, n), y0 + rs.choice([0.0, sy], n) + delta, np.zeros(n)][k == 1]
  # 2: along +x over the box's top / bottom face (its z edges)
  m = k == 2
  o[m] = np.c_[np.full(n, x0 - 20.0), rs.uniform(y0, y0 + sy, n), z0 + rs.choice([0.0, sz], n) + delta][m]
  d[m] = [1.0, 0.0, 0.0]
  # 3: along +z onto the upright cylinder's cap rim; 4: along +y tangent to its side
  cx, cy, cz = g['cyl_at']
  phi = rs.uniform(0, 2 * np.pi, n)
  r = g['cyl_r'] + delta
  o[k == 3] = np.c_[cx + r * np.cos(phi), cy + r * np.sin(phi), np.zeros(n)][k == 3]
  m = k == 4
  o[m] = np.c_[cx + rs.choice([-1.0, 1.0], n) * r, np.full(n, cy - 30.0), rs.uniform(cz, cz + g['cyl_h'], n)][m]
  d[m] = [0.0, 1.0, 0.0]
  # 5: along +z at the rim of the lens's cylinder (radius 8)
  r8 = 8.0 + delta
  o[k == 5] = np.c_[r8 * np.cos(phi), r8 * np.sin(phi), np.zeros(n)][k == 5]
  return o, unit(d)


def rays_bench(rs, n):
  """a beam through the torus's hole and the lens, and a fan onto everything else"""
  o = np.c_[rs.normal(0, 2.0, n), rs.normal(0, 2.0, n), np.zeros(n)]
  d = np.c_[rs.normal(0, 0.05, n), rs.normal(0, 0.05, n), np.ones(n)]
  wide = rs.rand(n) < 0.5
  d[wide] = np.c_[rs.normal(0, 0.4, n), rs.normal(0, 0.3, n), np.ones(n)][wide]
  return o, unit(d)
