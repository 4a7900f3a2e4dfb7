"""Scenes and rays for the compiled kernels' wave-uniform path inside an isolated solid (odw_kernels.hip: nearest() /
spec_uniform): a wave whose live lanes have all just entered the same isolated lens searches that lens's primitives
alone, without box screens; every other wave runs the general loop.  Whether a solid is isolated is a matter of the
boxes' VALUES (odw_build.h: compute_boxes), so it travels in the value image as one word -- bit s = solid s is isolated
-- and never in the header.  Built with the helpers of spec_image_cases; shared by tests/test_spec_isolated_build.py
(CPU: headers, the mask word, the oracle's rows) and tests/test_gpu_spec_isolated.py (compiled rows against generic
rows as byte strings).

The bench: rays start near z = 0 and travel along +z through lens A (z = 28 .. 32) and lens B (z = 48 .. 52), are sent
back by a mirror at z = 70, pass both lenses again and end on the screen behind the start (z = -10).  A lens is
Common(sphere, cylinder): a spherical front (R = 30), the cylinder's wall (r = 8) and its flat back; both operands
share one box."""
import re

import numpy as np

import spec_image_cases as cases
from freecad.optics_design_workbench_amd.freecad_elements import make
from freecad.optics_design_workbench_amd.scene import Document

N = 20000
SEED = 0x0D15EA5E
TOL = 1e-6
LENS_R, RIM = 30.0, 8.0
Z_A, Z_B = 28.0, 48.0                     # front vertices of the two lenses
THICK = 4.0
NEAR, AWAY = RIM + 5e-6, RIM + 1.0        # x of the side mirror's face: its box within 4 distTol of lens B's, and clear of it


def _lens(doc, name, z, concave=False):
  if concave:
    # Cut(cylinder, sphere): the sphere (centre on the axis in front of the lens) bites a dip into the front
    cyl = make.makeCylinder(doc, name + 'c', RIM, THICK + 1.0, base=(0, 0, z))
    tool = make.makeSphere(doc, name + 's', LENS_R, base=(0, 0, z + 2.0 - LENS_R))
    return make.makeCut(doc, cyl, tool, name)
  sph = make.makeSphere(doc, name + 's', LENS_R, base=(0, 0, z + LENS_R))
  cyl = make.makeCylinder(doc, name + 'c', RIM, THICK + 1.0, base=(0, 0, z - 1.0))
  return make.makeCommon(doc, [sph, cyl], name)


def bench(side_mirror=None, concave=False, **lens):
  """mirror, lens A, lens B, screen; side_mirror: x of the face of a second mirror box beside lens B (None: none)"""
  doc = Document()
  make.makeMirror(doc, [make.makeBox(doc, 'M', 40, 40, 2, base=(-20, -20, 70.0))] +
                  ([make.makeBox(doc, 'N', 6, 40, 20, base=(side_mirror, -20, Z_B - 8.0))] if side_mirror is not None else []))
  if concave:
    lenses = [_lens(doc, 'A', Z_A, concave=True)]
  else:
    lenses = [_lens(doc, 'A', Z_A), _lens(doc, 'B', Z_B)]
  make.makeLens(doc, lenses, **dict(dict(RefractiveIndex=1.5), **lens))
  make.makeAbsorber(doc, [make.makeBox(doc, 'S', 160, 160, 1, base=(-80, -80, -11.0))], RecordHits=True)
  make.makeSimulationSettings(doc, DistanceTolerance='1e-6')
  return cases.baked(doc)


def coherent():
  return bench()


def concave():
  return bench(concave=True)


def not_isolated():
  return bench(side_mirror=NEAR)


def flip():
  """(away, near): one structure; lens B is isolated in the first and not in the second"""
  return bench(side_mirror=AWAY), bench(side_mirror=NEAR)


def batch():
  """three scenes of one structure: lens B isolated in scenes 0 and 2, not in scene 1"""
  return [bench(side_mirror=x) for x in (AWAY, NEAR, AWAY + 0.5)]


def chroma():
  return bench(**make.N_BK7)


def fresnel():
  return bench(Fresnel='Split')


# ---- rays ------------------------------------------------------------------------------------------------------------
def rays_beam(seed=41, n=N, sigma=1.5):
  """a narrow beam along +z from z = 0: every ray takes the same path, waves stay together"""
  rs = np.random.RandomState(seed)
  o = np.c_[rs.normal(0, sigma, n), rs.normal(0, sigma, n), np.zeros(n)]
  d = np.c_[rs.normal(0, 0.01, n), rs.normal(0, 0.01, n), np.ones(n)]
  return o, cases.unit(d)


def rays_mixed(seed=42, n=N):
  """neighbouring ray indices alternate: enters lens A / starts between the lenses and enters lens B / passes beside both"""
  o, d = rays_beam(seed, n)
  k = np.arange(n) % 3
  o[k == 1, 2] = 40.0
  o[k == 2, 0] += 14.0
  return o, d


def rays_inside(seed=43, n=N):
  """origins inside lens A"""
  o, d = rays_beam(seed, n)
  o[:, 2] = Z_A + 2.5
  return o, d


def rays_fan(seed=44, n=N):
  """a wide fan onto the concave lens: rays cross the dip, leave through the concave face, some meet the lens again"""
  rs = np.random.RandomState(seed)
  o = np.c_[rs.normal(0, 3.0, n), rs.normal(0, 3.0, n), np.zeros(n)]
  d = np.c_[rs.normal(0, 0.12, n), rs.normal(0, 0.12, n), np.ones(n)]
  return o, cases.unit(d)


EDGE_OFFSETS = (0.0, 0.5, -0.5, 2.0, -2.0)      # of distTol
# rays of rays_edges() that enter lens A and whose next segment does not end on it, counted on the CPU oracle
# (tests/test_spec_isolated_build.py holds the oracle to it): what the retry after an empty short search is for
EDGE_PASS_BY = 1432


def rays_edges(seed=45, n=N):
  """rays aimed at the rim circle of lens A's front face (where the sphere meets the cylinder's wall) at radial offsets of
  0, +-0.5 and +-2 distTol -- along the axis, and tilted outward by 20 degrees, so that a ray accepted on the face just
  beyond the wall travels on outside the cylinder --, and rays grazing the cylinder's wall across the axis"""
  rs = np.random.RandomState(seed)
  phi = rs.uniform(0, 2 * np.pi, n)
  delta = np.asarray(EDGE_OFFSETS)[np.arange(n) % len(EDGE_OFFSETS)] * TOL
  kind = (np.arange(n) // len(EDGE_OFFSETS)) % 3
  r = RIM + delta
  z_rim = Z_A + LENS_R - np.sqrt(LENS_R ** 2 - r ** 2)
  er = np.c_[np.cos(phi), np.sin(phi), np.zeros(n)]
  target = er * r[:, None] + np.c_[np.zeros(n), np.zeros(n), z_rim]
  tilt = np.where(kind == 1, np.radians(20.0), 0.0)
  d = er * np.sin(tilt)[:, None] + np.c_[np.zeros(n), np.zeros(n), np.cos(tilt)]
  o = target - d * (z_rim / d[:, 2])[:, None]                 # back to z = 0
  # grazing: along +y, tangent to the wall at x = +-r, at a height where the wall exists
  g = kind == 2
  side = np.where(rs.rand(n) < 0.5, -1.0, 1.0)
  o[g] = np.c_[side * r, np.full(n, -30.0), rs.uniform(Z_A + 1.5, Z_A + THICK - 0.5, n)][g]
  d[g] = [0.0, 1.0, 0.0]
  return o, cases.unit(d)


# ---- what the library reports ----------------------------------------------------------------------------------------
def header_word(header, name):
  """`static constexpr int <name> = <v>` of a header"""
  m = re.search(r'\b%s = (-?\d+)' % name, header)
  assert m, name
  return int(m.group(1))


def mask_word(native, pr):
  """(the mask word of the scene's value image, the header of its kernel).  The word lies behind the image's doubles
  (Spec::iso = their count, Spec::IMG one more); odw_spec_image reports the doubles and, given room for one word more,
  writes the mask behind them as the kernel finds it"""
  import ctypes as C
  header, _ = native.compile_check(pr.scene, pr.limits, 'structure')
  at = header_word(header, 'iso')
  doubles = native.spec_image(pr.scene, pr.limits)['image']
  assert at == len(doubles) >= 4 and header_word(header, 'IMG') == at + 1
  d, keep = native.scene_desc(pr.scene)
  lim = native.LimitsDesc(float(pr.limits.max_ray_length), int(pr.limits.max_intersections), float(pr.limits.dist_tol),
                          float(pr.limits.power_tol))
  pd = C.POINTER(C.c_double)
  f = native.lib().odw_spec_image
  f.argtypes = [C.POINTER(native.SceneDescCoef), C.POINTER(native.LimitsDesc), pd, C.c_uint64, C.POINTER(C.c_uint64),
                C.POINTER(C.c_int32), C.c_uint64, pd, C.POINTER(C.c_int32)]
  whole = np.full(at + 1, -1.0, np.float64)
  size = C.c_uint64(0)
  native.check(None, f(C.byref(d), C.byref(lim), whole.ctypes.data_as(pd), whole.size, C.byref(size), None, 0, None, None), 'odw_spec_image')
  assert int(size.value) == at and whole[:at].tobytes() == doubles.tobytes()
  return int(whole[at:at + 1].view(np.uint64)[0]), header


def expected_mask(native, pr):
  """compute_boxes' rule from the boxes the library reports: a solid is isolated when the union of its live
  primitives' boxes keeps more than 4 distTol clear of every other solid's along some axis"""
  sc = pr.scene
  boxes = native.spec_image(sc, pr.limits)['boxes']
  solid = np.asarray(sc.prim_solid)
  live = boxes[:, 0] < 1e29
  ids = sorted(set(int(s) for s in solid[live]))
  lo = {s: boxes[live & (solid == s), :3].min(axis=0) for s in ids}
  hi = {s: boxes[live & (solid == s), 3:].max(axis=0) for s in ids}
  gap = 4.0 * float(pr.limits.dist_tol)
  mask = 0
  for s in ids:
    alone = all(np.any((lo[s] - hi[t] > gap) | (lo[t] - hi[s] > gap)) for t in ids if t != s)
    if alone and s < 64:
      mask |= 1 << s
  return mask


def lens_solids(pr):
  """solid ids of the lens group's primitives"""
  sc = pr.scene
  lens_groups = [g for g in range(len(sc.group_type)) if int(sc.group_type[g]) == 1]
  return sorted(set(int(s) for s, g in zip(sc.prim_solid, sc.prim_group) if int(g) in lens_groups))


def passes_by(rows, pr):
  """rays with a row that enters the lens group and whose next row (if any) is not on the lens group: the segment
  behind the entry hit does not end on the lens"""
  sc = pr.scene
  lens = [g for g in range(len(sc.group_type)) if int(sc.group_type[g]) == 1]
  ray = (rows['tag'] & np.uint64(0xFFFFFFFFFF)).astype(np.int64)
  order = np.argsort(ray, kind='stable')
  ray, tag = ray[order], rows['tag'][order]
  group = ((tag >> np.uint64(48)) & np.uint64(0x7FFF)).astype(np.int64)
  entering = (tag >> np.uint64(63)).astype(bool)
  on_lens = np.isin(group, lens)
  nxt_same_ray = np.r_[ray[1:] == ray[:-1], False]
  nxt_on_lens = np.r_[on_lens[1:], False] & nxt_same_ray
  return int(np.count_nonzero(on_lens & entering & ~nxt_on_lens))
