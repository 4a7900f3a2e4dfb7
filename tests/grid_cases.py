"""Scenes, rays and closed forms that hold the grid kernel (csrc/odw_grid.hip): tests/test_grid_cases.py checks them
against the CPU oracle, tests/test_gpu_grid.py traces them on the device.

Every scene is one Vacuum group around solids that never trim each other: a ray goes straight through and records
where it enters and where it leaves each solid, so the expected rows are the sorted crossings of a line with spheres
(the textbook quadratic), boxes (the slab rule) and ellipsoids (ellipsoid_cases.ellipsoid_interval).  Spheres and boxes are
worked out in numpy.longdouble and rounded to float64 at the end.

A ray is EXCLUDED from the comparison with the closed form -- the mask is returned and counted by the tests, never
applied silently -- when rounding may decide what it records:
  two of its crossings lie closer than 1e-3 mm, a sphere's discriminant is below 1e-4 in size (grazing), a box is met
  only after growing it by 1e-5 mm or no longer after shrinking it by as much (grazing), a crossing lies within 1e-3 mm
  of the origin, or a segment measures max_ray_length to within 1e-3 mm."""
import functools

import numpy as np

import ellipsoid_cases as ec
from freecad.optics_design_workbench_amd.freecad_elements import make

LD = np.longdouble
NEAR = 1e-3                 # mm: crossings closer than this to each other or to the origin
GRAZING = 1e-4              # mm^2: discriminant (unit direction) of a grazing line
BOX_GRAZING = 1e-5          # mm: a line this close to an edge of a box grazes it (faces are widened by the tolerance, 1e-6)
RING_BYTES = 16 * 64 * 7 * 8      # the ray rings of a grid block: 16 waves x 64 rays x 7 doubles
PITCH, RADIUS = 10.0, 2.0          # of the 5 x 4 x 4 lattice
SHAPE = (5, 4, 4)
ZEROS = (0.0, -0.0, 1e-17, 1e-200)


def tables_in_lds(info):
  """from odw_build_check's figures: are the cells (and items) of the grid staged in LDS?  A block's dynamic LDS is
  planes + wave words + rings, plus 4 bytes per cell and the items only where they are staged"""
  return info['grid_lds_bytes'] >= 4 * info['grid_cells'] + RING_BYTES


def sphere_records(info):
  """from the same figures, where the tables are staged: do the items take 48 bytes each (the records of the SPHERES
  instantiations) and not 4 (primitive numbers)?  Where the tables stay in global memory the figures do not tell: there
  the kind follows from build_grid's rule alone (every primitive an untrimmed sphere)"""
  assert tables_in_lds(info)
  # (planes and wave words, which the figures leave out, take 2064 bytes and 8 per plane: fewer than the records must)
  assert 44 * info['grid_items'] > 2064 + 8 * (info['grid_cells'] + 5), info
  return info['grid_lds_bytes'] >= 4 * info['grid_cells'] + RING_BYTES + 48 * info['grid_items']


# ---- scenes -------------------------------------------------------------------------------------------------------------
class Case:
  """sc, lim: the baked scene and limits; solids: [('sphere', centre, r) | ('box', lo, hi) | ('ellipsoid', centre, radii)];
  cells, items, in_lds: what odw_build_check has to report"""

  def __init__(self, solids, cells, items, in_lds, **settings):
    self.solids, self.cells, self.items, self.in_lds = solids, cells, items, in_lds

    def elems(doc):
      out = []
      for i, (kind, a, b) in enumerate(solids):
        if kind == 'sphere':
          out.append(make.makeSphere(doc, f'S{i}', float(b), base=tuple(float(v) for v in a)))
        elif kind == 'box':
          out.append(ec.centred_box(doc, f'B{i}', a, b))
        else:
          out.append(ec.ellipsoid(doc, f'E{i}', tuple(float(v) for v in b), base=tuple(float(v) for v in a)))
      return out
    self.sc, self.lim = ec.vacuum(elems, **settings)

  @property
  def spheres(self):
    return all(s[0] == 'sphere' for s in self.solids)

  @property
  def oracle_knows(self):
    return all(s[0] != 'ellipsoid' for s in self.solids)          # (the CPU oracle has no ellipsoid)


LATTICE = np.array([[PITCH * i, PITCH * j, PITCH * k] for i in range(SHAPE[0]) for j in range(SHAPE[1]) for k in range(SHAPE[2])])
STAGGERED = np.array([[6.0 * i + 3 * (j % 2), 6.0 * j + 3 * (k % 2), 6.0 * k + 3 * (i % 2)]
                      for i in range(SHAPE[0]) for j in range(SHAPE[1]) for k in range(SHAPE[2])])


def _spheres(centres, radii):
  return [('sphere', np.asarray(c, float), float(r)) for c, r in zip(centres, radii)]


def _lattice():
  return Case(_spheres(LATTICE, np.full(len(LATTICE), RADIUS)), 80, 80, True)


def _mixed():
  """the lattice with a cube of side 2 r in place of every third sphere: the same boxes, so the same planes"""
  solids = _spheres(LATTICE, np.full(len(LATTICE), RADIUS))
  for i in range(1, len(solids), 3):
    solids[i] = ('box', LATTICE[i] - RADIUS, LATTICE[i] + RADIUS)
  return Case(solids, 80, 80, True)


def _cloud():
  rng = np.random.default_rng(3)
  centres = rng.uniform(-30, 30, (90, 3))
  return Case(_spheres(centres, rng.uniform(1, 9, 90)), 80, 390, True)


def _staggered():
  return Case(_spheres(STAGGERED, np.full(len(STAGGERED), 2.5)), 80, 441, True)


def _big():
  idx = [(i, j, k) for i in range(13) for j in range(13) for k in range(13)]
  return Case(_spheres(PITCH * np.array(idx, float), [2 + 0.001 * (i % 7) for i, j, k in idx]), 2197, 2197, False)


def _seventy():
  """70 small solids far apart, spheres / cubes / ellipsoids in turn: a plane in nearly every gap, so tens of thousands of
  cells for 70 items (the half-widths, uniform in 1 .. 3 mm per axis, are this file's choice: 32 x 32 x 38 cells)"""
  rng = np.random.default_rng(5)
  centres = rng.uniform(-200, 200, (70, 3))
  half = rng.uniform(1, 3, (70, 3))
  solids = []
  for i, (c, h) in enumerate(zip(centres, half)):
    solids.append([('sphere', c, h[0]), ('box', c - h, c + h), ('ellipsoid', c, h)][i % 3])
  return Case(solids, SEVENTY_CELLS, 70, False, MaxRayLength=5000.0)


SEVENTY_CELLS = 32 * 32 * 38
_MAKERS = dict(lattice=_lattice, mixed=_mixed, cloud=_cloud, staggered=_staggered, big=_big, seventy=_seventy)
SCENES = tuple(_MAKERS)


@functools.lru_cache(maxsize=None)
def case(name):
  return _MAKERS[name]()


# ---- the planes build_grid cuts (csrc/odw_build.h), from the solids' boxes ---------------------------------------------------
def planes(solids, dist_tol=ec.DIST_TOL):
  """the three plane tables of the grid over `solids`: one plane in the middle of every gap between the boxes (2 distTol
  of slack) projected on the axis, slabs wider than twice the width of an even division cut evenly.  A restatement in
  Python: a value may be an ulp off the library's, which is why the aimed rays come at the neighbouring values too"""
  lo, hi = [], []
  for kind, a, b in solids:
    a, b = np.asarray(a, float), np.asarray(b, float)
    lo.append(a - b if kind != 'box' else a)
    hi.append(a + b if kind != 'box' else b)
  lo, hi = np.array(lo) - 2 * dist_tol, np.array(hi) + 2 * dist_tol
  ext = np.maximum(hi.max(0) - lo.min(0), 1e-9)
  target = 1.0 / np.cbrt(len(solids) / ext.prod())
  out = []
  for a in range(3):
    order = np.argsort(lo[:, a], kind='stable')
    pad = 1e-6 * (1.0 + ext[a])
    b, cover = [lo[:, a].min() - pad], hi[order[0], a]
    for k in order[1:]:
      if lo[k, a] > cover:
        b.append(0.5 * (cover + lo[k, a]))
      cover = max(cover, hi[k, a])
    b.append(hi[:, a].max() + pad)
    cut = [b[0]]
    for k in range(1, len(b)):
      w = b[k] - b[k - 1]
      parts = int(min(128.0, np.floor(w / target + 0.5))) if w > 2.0 * target else 1
      cut += [b[k] if j == parts else b[k - 1] + w * j / parts for j in range(1, parts + 1)]
    assert len(cut) - 1 <= 128
    out.append(np.array(cut))
  return out


def ulps(v, span=2):
  """v and its neighbours up to `span` ulp on either side"""
  out = [float(v)]
  for sign in (-1, 1):
    w = float(v)
    for _ in range(span):
      w = float(np.nextafter(w, sign * np.inf))
      out.append(w)
  return sorted(out)


# ---- closed forms ---------------------------------------------------------------------------------------------------------
def _unit(d):
  d = np.asarray(d, LD)
  return d / np.sqrt((d * d).sum(-1))[:, None]


def _box_ld(o, d, lo, hi):
  with np.errstate(divide='ignore', invalid='ignore'):
    ta, tb = (np.asarray(lo, LD) - o) / d, (np.asarray(hi, LD) - o) / d
  tn, tf = np.fmin(ta, tb).max(-1), np.fmax(ta, tb).min(-1)
  return tn, tf, tn < tf


def crossings(o, d, solids):
  """-> (ray index, parameter t) of every crossing of the lines o + t d / |d| with the solids' surfaces, t of either sign,
  and the mask of the rays that graze a solid"""
  o, d = np.asarray(o, LD), _unit(d)
  n = len(o)
  ray, t, grazing = [], [], np.zeros(n, bool)
  for kind, a, b in solids:
    if kind == 'sphere':
      oc = o - np.asarray(a, LD)
      bh, cc = (oc * d).sum(-1), (oc * oc).sum(-1) - LD(b) * LD(b)
      disc = bh * bh - cc
      grazing |= np.abs(disc) < GRAZING
      k = np.nonzero(disc > 0)[0]
      sq = np.sqrt(disc[k])
      t0, t1 = -bh[k] - sq, -bh[k] + sq
    elif kind == 'box':
      t0, t1, hit = _box_ld(o, d, a, b)
      grazing |= _box_ld(o, d, np.asarray(a) - BOX_GRAZING, np.asarray(b) + BOX_GRAZING)[2] != _box_ld(o, d, np.asarray(a) + BOX_GRAZING, np.asarray(b) - BOX_GRAZING)[2]
      k = np.nonzero(hit)[0]
      t0, t1 = t0[k], t1[k]
    else:
      t0, t1 = ec.ellipsoid_interval(np.asarray(o - np.asarray(a, LD), float), np.asarray(d, float), b)
      k = np.nonzero(np.isfinite(t0))[0]
      t0, t1 = t0[k].astype(LD), t1[k].astype(LD)
    ray += [k, k]
    t += [t0, t1]
  return np.concatenate(ray), np.concatenate(t), grazing


def expected(o, d, solids, max_ray_length=1000.0):
  """-> (points per ray as float64 (k, 3) in the order the ray meets them, excluded rays).  A crossing counts while it lies
  ahead (t > 0) and no more than max_ray_length beyond the one before it (or the origin): the ray escapes there"""
  o, d = np.asarray(o, float), np.asarray(d, float)
  ray, t, excluded = crossings(o, d, solids)
  excluded = excluded.copy()
  np.logical_or.at(excluded, ray[np.abs(t) < NEAR], True)
  order = np.lexsort((t, ray))
  ray, t = ray[order], t[order]
  starts = np.searchsorted(ray, np.arange(len(o) + 1))
  ol, dl = np.asarray(o, LD), _unit(d)
  want = []
  for k in range(len(o)):
    ts = t[starts[k]:starts[k + 1]]
    ts = ts[ts > 0]
    if len(ts) > 1 and np.diff(ts).min() < NEAR:
      excluded[k] = True
    gaps = np.diff(np.r_[LD(0), ts])
    if np.any(np.abs(gaps - max_ray_length) < NEAR):
      excluded[k] = True
    far = np.nonzero(gaps > max_ray_length)[0]
    if len(far):
      ts = ts[:far[0]]
    want.append(np.asarray(ol[k] + ts[:, None] * dl[k], float).reshape(-1, 3))
  return want, excluded


def expected_for(c, o, d):
  return expected(o, d, c.solids, float(c.lim.max_ray_length))


def held(rows, o, d, want, excluded, label, by_name=()):
  """every ray that is not excluded records exactly its expected points, each within ec.TOL -> (worst, crossings)"""
  got = ec.per_ray(rows, o, d)
  worst, crossings = 0.0, 0
  for k, (g, w) in enumerate(zip(got, want)):
    if excluded[k] or k in by_name:
      continue
    assert len(g) == len(w), (label, k, o[k], d[k], g, w)
    crossings += len(w)
    if len(w):
      worst = max(worst, float(np.abs(g - w).max()))
  print(f'{label}: {len(o)} rays, {crossings} crossings, {int(excluded.sum())} excluded, worst {worst:.3e} mm')
  assert worst < ec.TOL, label
  return worst, crossings


# ---- rays -------------------------------------------------------------------------------------------------------------------
def random_set(name):
  """the random rays of a scene: 2000 lines through it (seed 11); for the cloud also 500 rays that start inside it (12).
  The 70 solids fill a millionth of their cube: there every line passes within 3 mm (per axis) of a solid's centre"""
  if name == 'seventy':
    o, d = ec.random_lines(2000, seed=11, span=3.0, back=100.0)
    return o + np.array([s[1] if s[0] != 'box' else 0.5 * (s[1] + s[2]) for s in case(name).solids])[np.arange(2000) % 70], d
  span, back = dict(lattice=(25.0, 60.0), mixed=(25.0, 60.0), cloud=(35.0, 200.0), staggered=(16.0, 200.0), big=(65.0, 150.0),
                    seventy=(3.0, 100.0))[name]
  o, d = ec.random_lines(2000, seed=11, span=span, back=back)
  centre = dict(lattice=(20.0, 15.0, 15.0), mixed=(20.0, 15.0, 15.0), staggered=(13.5, 10.5, 10.5), big=(60.0, 60.0, 60.0)).get(name, (0.0, 0.0, 0.0))
  return o + np.array(centre), d


def inside_starts():
  return ec.random_lines(500, seed=12, span=30.0, back=0.0)


def _rows(rays):
  o, d = zip(*rays)
  return np.array(o, float), np.array(d, float)


def axis_parallel(zero=0.0):
  """both senses along the three axes: through a row of centres, between rows, 1.999 mm beside a row (inside r = 2) and
  2 + 1e-9 mm beside it (outside).  The other two direction components are `zero`"""
  rays = []
  for a in range(3):
    b, c = (a + 1) % 3, (a + 2) % 3
    for s in (1.0, -1.0):
      for u, v in ((10.0, 20.0), (14.0, 16.0), (10.0 + 1.999, 20.0), (10.0, 20.0 + RADIUS + 1e-9)):
        o, d = np.zeros(3), np.full(3, zero)
        o[a], o[b], o[c] = (-50.0 if s > 0 else PITCH * (SHAPE[a] - 1) + 50.0), u, v
        d[a] = s
        rays.append((o, d))
  return _rows(rays)


AXIS_GRAZING = np.tile([False, False, False, True], 6)         # the 2 + 1e-9 rays of axis_parallel: nothing recorded
AXIS_CHORD = np.tile([False, False, True, False], 6)           # the 1.999 rays: the full chord of every sphere of the row


def in_plane(solids):
  """rays that lie in a plane of the grid: per axis an inner plane and its neighbours within 2 ulp, along either other axis
  and along their diagonal"""
  rays = []
  for a, table in enumerate(planes(solids)):
    b, c = (a + 1) % 3, (a + 2) % 3
    for p in ulps(table[len(table) // 2]):
      for db, dc in ((1.0, 0.0), (0.0, -1.0), (1.0, 0.7)):
        o, d = np.zeros(3), np.zeros(3)
        o[a], o[b], o[c] = p, 12.3 - 60.0 * db, 11.1 - 60.0 * dc
        d[b], d[c] = db, dc
        rays.append((o, d / np.linalg.norm(d)))
  return _rows(rays)


def diagonals():
  """along lines where two planes of the lattice meet and through points where three meet: (+-1, +-1, 0) / sqrt 2 and its
  permutations, (+-1, +-1, +-1) / sqrt 3, through (15, 15, 15) and through a point of the next layer of centres"""
  dirs = []
  for a in range(3):
    for s in (1.0, -1.0):
      for r in (1.0, -1.0):
        e = np.zeros(3)
        e[(a + 1) % 3], e[(a + 2) % 3] = s, r
        dirs.append(e / np.sqrt(2.0))
  dirs += [np.array([s, r, q]) / np.sqrt(3.0) for s in (1.0, -1.0) for r in (1.0, -1.0) for q in (1.0, -1.0)]
  rays = []
  for e in dirs:
    for p in ((15.0, 15.0, 15.0), tuple(np.where(e == 0, 10.0, 15.0)) if np.any(e == 0) else (15.0, 15.0, 5.0)):
      rays.append((np.array(p) - 40.0 * e, e))
  return _rows(rays)


def origins(solids=None):
  """where a ray may start: outside the grid entering through a face, an edge, a corner; outside and parallel to a face
  (one with a zero component, beyond the extent); pointing away; on the outermost plane (and within 2 ulp of it); in a
  cell outside its sphere; inside a sphere; 1000 mm away"""
  px, py, pz = planes(solids or case('lattice').solids)
  n = lambda v: np.asarray(v, float) / np.linalg.norm(v)
  rays = [((-30.0, 12.0, 13.0), n((1.0, 0.1, 0.05))),                                     # a face
          ((px[0] - 20.0, py[0] - 20.0, 10.0), n((1.0, 1.0, 0.0))),                       # an edge
          ((px[0] - 20.0, py[0] - 20.0, pz[0] - 20.0), n((1.0, 1.0, 1.0))),               # a corner
          ((px[-1] + 20.0, py[-1] + 20.0, pz[0] - 20.0), n((-1.0, -1.0, 1.0))),           # the opposite corner
          ((-30.0, -10.0, 13.0), (1.0, 0.0, 0.0)),                                        # parallel, beyond the extent
          ((-30.0, -10.0, 13.0), n((1.0, 0.0, 0.2))),
          ((-30.0, -10.0, 13.0), n((1.0, -0.01, 0.0))),
          ((20.0, 10.0, 45.0), (0.0, 1.0, 0.0)),
          ((-30.0, 12.0, 13.0), (-1.0, 0.0, 0.0)),                                        # pointing away
          ((-30.0, 12.0, 13.0), n((-1.0, -0.3, 0.2))),
          ((20.0, 50.0, 10.0), n((0.1, 1.0, 0.0)))]
  for x in ulps(px[0]) + ulps(px[-1]):                                                     # on the outermost planes
    rays += [((x, -20.0, 13.0), (0.0, 1.0, 0.0)), ((x, 10.5, 11.0), (1.0, 0.0, 0.0)), ((x, 10.5, 11.0), (-1.0, 0.0, 0.0)),
             ((x, 12.0, 13.0), n((0.5 if x < 0 else -0.5, 0.2, 0.1)))]
  for y in ulps(py[-1]):
    rays += [((10.5, y, 11.0), (0.0, -1.0, 0.0)), ((-20.0, y, -20.0), n((1.0, 0.0, 1.0)))]
  for d in ((1.0, 0.0, 0.0), n((1.0, 1.0, 1.0)), n((-0.3, 0.2, 1.0)), (0.0, 0.0, -1.0)):
    rays += [((14.0, 13.0, 12.0), d), ((10.5, 10.2, 9.8), d), ((20.0, 20.0, 21.0), d)]     # empty space; inside spheres
  rays += [((-990.0, 10.0, 10.0), (1.0, 0.0, 0.0))]
  for d in (n((1.0, 0.2, -0.1)), n((-0.3, 1.0, 0.4)), n((0.2, 0.1, -1.0))):
    rays.append((np.array([20.0, 10.0, 10.0]) - 950.0 * d, d))
  return _rows(rays)


def length_limit(limit=1000.0):
  """rays whose first sphere lies 1 mm inside the length limit (they record) and 1 mm beyond it (nothing, escaped)"""
  n = lambda v: np.asarray(v, float) / np.linalg.norm(v)
  inside, beyond = [], []
  for c, d in (((0.0, 10.0, 10.0), (1.0, 0.0, 0.0)), ((40.0, 20.0, 10.0), (-1.0, 0.0, 0.0)), ((10.0, 0.0, 20.0), (0.0, 1.0, 0.0)),
               ((0.0, 10.0, 10.0), n((1.0, 0.2, 0.1))), ((10.0, 30.0, 30.0), n((0.1, -0.7, -1.0))), ((40.0, 30.0, 0.0), n((-1.0, -0.5, 0.8)))):
    for margin, rays in ((-1.0, inside), (1.0, beyond)):
      rays.append((np.array(c) - (limit + RADIUS + margin) * np.asarray(d), d))
  o, d = _rows(inside + beyond)
  return o, d, np.r_[np.zeros(len(inside), bool), np.ones(len(beyond), bool)]


def overlap_starts():
  """rays that start inside two overlapping spheres of the cloud, at the middle of the lens the two have in common"""
  solids = case('cloud').solids
  c, r = np.array([s[1] for s in solids]), np.array([s[2] for s in solids])
  rays = []
  for i in range(len(c)):
    for j in range(i + 1, len(c)):
      gap = np.linalg.norm(c[j] - c[i])
      if gap < r[i] + r[j] - 1.0 and gap > abs(r[i] - r[j]) + 1.0 and len(rays) < 60:
        u = (c[j] - c[i]) / gap
        p = c[i] + u * 0.5 * (gap + r[i] - r[j])
        for d in (u, -u, np.cross(u, [0.3, -0.5, 0.8]) / np.linalg.norm(np.cross(u, [0.3, -0.5, 0.8]))):
          rays.append((p, d))
  return _rows(rays)


def aimed_sets(name='lattice'):
  """{set: (origins, directions)} of the aimed rays of the 5 x 4 x 4 lattices"""
  solids = case(name).solids
  sets = {f'axis[{z!r}]': axis_parallel(z) for z in ZEROS}
  sets['in-plane'] = in_plane(solids)
  sets['diagonals'] = diagonals()
  sets['origins'] = origins(solids)
  sets['length-limit'] = length_limit(float(case(name).lim.max_ray_length))[:2]
  return sets


# ---- the grid kernel's own interactions: a bench of 13 primitives ---------------------------------------------------------
# Stations 100 mm apart along x above one absorbing floor; every ray meets at most three curved surfaces.
BENCH_GROUPS = ('mirror', 'lens', 'reflection', 'transmission', 'vacuum', 'perfect', 'floor')


def bench(faceted=False, **settings):
  """-> (scene, limits): a mirror of reflectivity 0.8, a ball lens and two glass blocks of absorbing glass, a reflection
  and a transmission grating (one slab of it inside a glass block: met from inside a medium), a vacuum ball, two pairs of
  facing mirrors (reflectivity 1: the cap on intersections; 0.8: the power limit), an absorber under everything.
  faceted: every solid but the floor as a mesh -- the boxes of 12 facets, the lens ball of 24 segments with smooth normals,
  the vacuum ball of 24 segments with flat ones (tests/mesh_cases.py)"""
  from freecad.optics_design_workbench_amd.scene import Document, bake
  doc = Document()
  box = lambda name, lo, hi: ec.centred_box(doc, name, lo, hi)
  ball = lambda name, r, base, smooth: make.makeSphere(doc, name, r, base=base)
  if faceted:
    from tree_cases import _cube_mesh
    box = lambda name, lo, hi: make.makeMesh(doc, *_cube_mesh(lo, hi), name=name)
    ball = lambda name, r, base, smooth: make.makeTessellated(doc, make.makeSphere(doc, name, r, base=base), 24, smooth=smooth)
  make.makeMirror(doc, [box('M', (-15, -15, 50), (15, 15, 52)), box('P0', (790, -15, 10), (792, 15, 50)), box('P1', (808, -15, 10), (810, 15, 50))],
                  Reflectivity=0.8, RecordHits=True)
  make.makeLens(doc, [ball('Ball', 8.0, (100.0, 0.0, 30.0), True), box('Cube', (195, -5, 25), (205, 5, 35)),
                      box('Block', (485, -15, 20), (515, 15, 60))], RefractiveIndex=1.5, AbsorptionLength='40.0', RecordHits=True)
  make.makeGrating(doc, [box('GR', (285, -15, 50), (315, 15, 52))], RecordHits=True, GratingType='Reflection',
                   GratingLinesPerMillimeter=600.0, GratingLinesOrientation=np.array([1.0, 0.0, 0.0]))
  make.makeGrating(doc, [box('GT', (385, -15, 50), (415, 15, 52)), box('GI', (490, -10, 40), (510, 10, 42))], RecordHits=True,
                   GratingType='Transmission', RefractiveIndex=1.5, GratingLinesPerMillimeter=300.0,
                   GratingLinesOrientation=np.array([0.0, 1.0, 0.0]))
  make.makeVacuum(doc, [ball('V', 5.0, (600.0, 0.0, 30.0), False)])
  make.makeMirror(doc, [box('F0', (690, -15, 10), (692, 15, 50)), box('F1', (708, -15, 10), (710, 15, 50))], Reflectivity=1.0,
                  RecordHits=True, name='PerfectMirrors')
  make.makeAbsorber(doc, [ec.centred_box(doc, 'Floor', (-100, -100, -42), (900, 100, -40))])
  make.makeSimulationSettings(doc, **dict(dict(DistanceTolerance='1e-6', MaxIntersections=6.0), **settings))
  src = make.makePointSource(doc)
  return bake.bakeScene(doc, src), bake.bakeLimits(doc, src)


def bench_variant(sc, lim, variant):
  """the bench as the interaction tests run it: 'capped' as it is, 'power-limit' with PowerTolerance 0.6, 'sequential'
  with a sequence whose third step leaves the mirrors out -> (scene, limits)"""
  import copy
  import dataclasses
  assert variant in ('capped', 'power-limit', 'sequential')
  if variant == 'power-limit':
    lim = dataclasses.replace(lim, power_tol=0.6)
  if variant == 'sequential':
    sc = copy.copy(sc)
    every = (1 << len(sc.group_type)) - 1
    sc.seq_enabled, sc.seq_mask = 1, np.array([every, every, every & ~1, every], np.uint64)
  return sc, lim


def bench_figures(rows, cnt, station, variant):
  """what the stations of the bench record, whichever kernel traced them and whether its solids are faceted or not"""
  per_ray = np.bincount((rows['tag'] & np.uint64(0xFFFFFFFFFFFF)).astype(np.int64), minlength=len(station))
  assert cnt['grating_in_medium'] == (station == 'in-medium').sum() == 100
  assert (per_ray[station == 'inside-ball'] == 1).all()
  if variant != 'sequential':
    assert (per_ray[station == 'tir'] == 4).all()                  # in, the side face (reflected totally), out, the floor
    assert (per_ray[station == 'perfect'] == 6).all() and cnt['capped'] == (200 if variant == 'capped' else 100)
    assert (per_ray[station == 'lossy'] == (6 if variant == 'capped' else 3)).all()
    assert len(np.unique(rows['power'])) > 300                        # (the absorbing glass moves the power)
  else:
    assert cnt['capped'] == 0 and per_ray.max() <= 4


def bench_rays():
  """-> (origins, directions, station of every ray)"""
  rng = np.random.default_rng(21)
  O, D, S = [], [], []

  def fan(station, origin, axis, spread, n, jitter=0.0):
    d = np.asarray(axis, float) + rng.uniform(-spread, spread, (n, 3))
    O.append(np.asarray(origin, float) + rng.uniform(-jitter, jitter, (n, 3)) * [1.0, 1.0, 0.0])
    D.append(d / np.linalg.norm(d, axis=1)[:, None])
    S.extend([station] * n)
  fan('mirror', (0, 0, 0), (0, 0, 1), 0.2, 200)
  fan('ball', (100, 0, 0), (0, 0, 1), 0.02, 300, jitter=6.0)
  fan('inside-ball', (100, 1, 30), (0.3, 0.2, 1), 0.5, 50)
  fan('tir', (189, 0, 44), (0.8, 0, -0.6), 0.02, 100)
  fan('reflection', (300, 0, 0), (0, 0, 1), 0.2, 200)
  fan('transmission', (400, 0, 0), (0, 0, 1), 0.2, 200)
  fan('in-medium', (500, 0, 0), (0, 0, 1), 0.1, 100)
  fan('vacuum', (600, 0, 0), (0, 0, 1), 0.1, 200)
  fan('perfect', (700, 0, 30), (1, 0.01, 0.02), 0.01, 100)
  fan('lossy', (800, 0, 30), (1, 0.01, 0.02), 0.01, 100)
  return np.vstack(O), np.vstack(D), np.array(S)


def cloud_project():
  """-> (scene, baked source, limits): the cloud around a point source at its middle that emits into the whole sphere"""
  from freecad.optics_design_workbench_amd.freecad_elements import point_source
  from freecad.optics_design_workbench_amd.scene import bake
  solids = case('cloud').solids
  doc, src = ec.document([('Vacuum', lambda d: [make.makeSphere(d, f'S{i}', r, base=tuple(float(v) for v in c)) for i, (_, c, r) in enumerate(solids)], {})],
                         source=dict(PowerDensity='1', ThetaDomain='0, pi'))
  return bake.bakeScene(doc, src), point_source.bakeSource(doc, src), bake.bakeLimits(doc, src)
