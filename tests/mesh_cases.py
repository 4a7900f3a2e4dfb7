"""What holds the mesh kernel (odw_mesh_kernel of csrc/odw_mesh.hip: the eight-wide tree with quantised child boxes, the
float32 leaf filter, its own copy of the interaction code): one scene, its ray sets and a reference that shares no code
with the kernels or the oracle.  tests/test_mesh_cases.py checks every set against the CPU oracle, tests/test_gpu_mesh.py
traces them through the mesh kernel.

  gallery        one Vacuum group (a ray goes straight through and records where it enters and where it leaves) around a
                 tessellated ball (strictly convex: normal cones and the skip rule are armed), a torus (not convex: up to
                 four crossings), a needle (a ball squeezed to 3 % and 20 %: sliver facets, still strictly convex), a cube
                 of 12 triangles and an analytic sphere: 4204 facets, 4205 primitives -- an eight-wide tree of three and
                 more levels with several leaf groups per solid.  far_gallery(): everything moved by tree_cases.T;
  reference      facet_crossings(): Moeller-Trumbore of every ray against every facet in numpy, in the unmoved frame --
                 screened in float64, decided in long double, the analytic sphere's roots added, crossings closer than
                 1e-9 mm merged (a vertex or a shared edge is ONE crossing).  The far sets are the same crossings plus T;
  ray sets       random lines from every octant; rays AIMED at vertices, edge points and centroids of facets at 0, 60 and
                 80 degrees; the random lines from 1000 mm further back; axis-parallel rays with tiny off-axis components;
                 origins on and just before a facet and inside the solids; first crossings 1e-3 mm inside and beyond
                 MaxRayLength;
  faceted bench  grid_cases.bench(faceted=True): the 13 primitives of the interaction bench with every solid but the
                 floor a mesh.

No exclusion rule was needed: on every set and both placements the oracle and the device record exactly the reference's
crossings, so no ray of any set is taken out of a comparison."""
import functools

import numpy as np

import ellipsoid_cases as ec
import grid_cases as gc
import tree_cases as tc
from freecad.optics_design_workbench_amd.freecad_elements import make, point_source
from freecad.optics_design_workbench_amd.scene import bake, geometry

LD = np.longdouble
T = tc.T
MERGE = 1e-9                 # mm: crossings closer than this are one (a vertex, a shared edge)
SCREEN = 1e-7                # barycentric margin of the float64 screen
DECIDE = 1e-12               # ... of the long double decision
BALL_C, BALL_R = np.array([-25.0, 0.0, 0.0]), 12.0
TORUS_C, TORUS_R, TORUS_r = np.array([20.0, 5.0, 0.0]), 14.0, 4.0
NEEDLE_C, NEEDLE_SCALE = np.array([0.0, -30.0, 10.0]), np.array([1.0, 0.03, 0.2])
CUBE_HALF = 4.0
CUBE_C = np.array([-4.0, 25.0, -30.0]) + CUBE_HALF      # (the 8 mm cube has its lowest corner at (-4, 25, -30))
SPHERE_C, SPHERE_R = np.array([0.0, 0.0, 35.0]), 6.0
SOLIDS = ('ball', 'torus', 'needle', 'cube')


@functools.lru_cache(maxsize=None)
def meshes():
  """{solid: (vertices, triangles)} in the unmoved frame"""
  out = {}
  v, tri, _ = geometry.tessellate(geometry.SPHERE, (BALL_R, 0, 0, 0), 48)
  out['ball'] = (v + BALL_C, tri)
  v, tri, _ = geometry.tessellate(geometry.TORUS, (TORUS_R, TORUS_r, 0, 0), 32)
  out['torus'] = (v + TORUS_C, tri)
  v, tri, _ = geometry.tessellate(geometry.SPHERE, (15.0, 0, 0, 0), 32)
  out['needle'] = (v * NEEDLE_SCALE + NEEDLE_C, tri)
  v, tri = tc._cube_mesh(CUBE_C - CUBE_HALF, CUBE_C + CUBE_HALF)
  out['cube'] = (v, tri)
  return out


@functools.lru_cache(maxsize=None)
def facets():
  """-> (corners (n, 3, 3) of every facet in the unmoved frame, in the order of SOLIDS, first facet of every solid + n)"""
  p = [v[tri] for v, tri in (meshes()[s] for s in SOLIDS)]
  return np.concatenate(p), np.cumsum([0] + [len(q) for q in p])


def facets_of(solid):
  p, first = facets()
  k = SOLIDS.index(solid)
  return p[first[k]:first[k + 1]]


class Gallery:
  """sc, lim, source: the baked scene, limits and point source (at the origin, into the whole sphere); shift: what every
  vertex and the sphere are moved by"""

  def __init__(self, shift, limit):
    self.shift = np.zeros(3) + np.asarray(shift, float)

    def elems(doc):
      out = [make.makeMesh(doc, v + self.shift, tri, name=s) for s, (v, tri) in ((s, meshes()[s]) for s in SOLIDS)]
      return out + [make.makeSphere(doc, 'S', SPHERE_R, base=tuple(float(x) for x in SPHERE_C + self.shift))]
    doc, src = ec.document([('Vacuum', elems, {})], source=dict(PowerDensity='1', ThetaDomain='0, pi'), MaxRayLength=limit)
    self.sc, self.lim = bake.bakeScene(doc, src), bake.bakeLimits(doc, src)
    self.sc.group_record = np.ones_like(self.sc.group_record)
    self.source = point_source.bakeSource(doc, src)


@functools.lru_cache(maxsize=None)
def gallery(shift=0, limit=1000.0):
  return Gallery(shift, limit)


def far_gallery(limit=1000.0):
  return gallery(tuple(T), limit)


# ---- the reference -----------------------------------------------------------------------------------------------------------
def _mt(o, d, p, real):
  """Moeller-Trumbore of rays (rows of o, d) against facets (rows of p), pairwise -> u, v, t, det in `real`"""
  o, d, p = np.asarray(o, real), np.asarray(d, real), np.asarray(p, real)
  e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
  pv = np.cross(d, e2)
  det = (e1 * pv).sum(-1)
  with np.errstate(divide='ignore', invalid='ignore'):
    inv = 1 / det
    tv = o - p[:, 0]
    u = (tv * pv).sum(-1) * inv
    qv = np.cross(tv, e1)
    return u, (d * qv).sum(-1) * inv, (e2 * qv).sum(-1) * inv, det


def _crossings(o, d, limit, chunk=512):
  """-> per ray the parameters t (long double) of its crossings, sorted, merged within MERGE, cut where a gap exceeds `limit`"""
  o = np.asarray(o, float)
  unit = np.asarray(gc._unit(d), float)
  p, _ = facets()
  # the screen: Moeller-Trumbore with its triple products regrouped per ray (m = o x d) and per facet, so that every ray
  # meets every facet in five matrix products: det = -d . N, u det = e2 . m - d . (e2 x v0), v det = -e1 . m - d . (v0 x e1),
  # t det = (o - v0) . N.  (Rounding: 1e-16 |o| / |edge|, far inside the margin.)
  v0, e1, e2 = p[:, 0], p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
  N = np.cross(e1, e2)
  m = np.cross(o, unit)
  ray, facet = [], []
  for k in range(0, len(o), chunk):
    dd, mm = unit[k:k + chunk], m[k:k + chunk]
    det = -(dd @ N.T)
    with np.errstate(divide='ignore', invalid='ignore'):
      inv = 1 / det
      u = (mm @ e2.T - dd @ np.cross(e2, v0).T) * inv
      v = (-(mm @ e1.T) - dd @ np.cross(v0, e1).T) * inv
      t = (o[k:k + chunk] @ N.T - (v0 * N).sum(-1)) * inv
      keep = (det != 0) & (u >= -SCREEN) & (v >= -SCREEN) & (u + v <= 1 + SCREEN) & (t > 0)
    r, f = np.nonzero(keep)
    ray.append(r + k)
    facet.append(f)
  ray, facet = np.concatenate(ray), np.concatenate(facet)
  ol, dl = np.asarray(o, LD), gc._unit(d)
  u, v, t, _ = _mt(ol[ray], dl[ray], p[facet], LD)
  keep = (u >= -DECIDE) & (v >= -DECIDE) & (u + v <= 1 + DECIDE) & (t > LD(ec.DIST_TOL))
  ray, t = ray[keep], t[keep]
  # the analytic sphere
  oc = ol - np.asarray(SPHERE_C, LD)
  bh = (oc * dl).sum(-1)
  disc = bh * bh - ((oc * oc).sum(-1) - LD(SPHERE_R) * LD(SPHERE_R))
  k = np.nonzero(disc > 0)[0]
  sq = np.sqrt(disc[k])
  for root in (-bh[k] - sq, -bh[k] + sq):
    ok = root > LD(ec.DIST_TOL)
    ray, t = np.r_[ray, k[ok]], np.r_[t, root[ok]]
  order = np.lexsort((t, ray))
  ray, t = ray[order], t[order]
  starts = np.searchsorted(ray, np.arange(len(o) + 1))
  out = []
  for k in range(len(o)):
    ts = t[starts[k]:starts[k + 1]]
    if len(ts) > 1:
      ts = ts[np.r_[True, np.diff(ts) >= MERGE]]                          # (a run of facets at one point: its first t)
    far = np.nonzero(np.diff(np.r_[LD(0), ts]) > limit)[0]
    out.append(ts[:far[0]] if len(far) else ts)
  return out


def facet_crossings(o, d, limit=1000.0):
  """the points (float64, (k, 3) per ray, in the order the ray meets them) at which the rays o + t d / |d| cross the
  gallery's facets and its sphere, in the unmoved frame: t > DistanceTolerance, no crossing more than `limit` beyond the
  one before it (the ray escapes there)"""
  ol, dl = np.asarray(o, LD), gc._unit(d)
  return [np.asarray(ol[k] + ts[:, None] * dl[k], float).reshape(-1, 3) for k, ts in enumerate(_crossings(o, d, limit))]


def nothing_excluded(o):
  """the mask grid_cases.held takes: no ray of any set here is taken out"""
  return np.zeros(len(o), bool)


# ---- ray sets: (origins, directions) in the unmoved frame, ray numbers in index order -----------------------------------------
def random_set():
  return ec.random_lines(4000, seed=11, span=40.0, back=200.0)


def back_set():
  o, d = random_set()
  return o - tc.BACK * d, d


def _frame(p):
  """of facets p (n, 3, 3): outward unit normal, and the edge v0 v1 turned by 1 rad in the facet's plane"""
  n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
  n /= np.linalg.norm(n, axis=1)[:, None]
  e = p[:, 1] - p[:, 0]
  e /= np.linalg.norm(e, axis=1)[:, None]
  return n, np.cos(1.0) * e + np.sin(1.0) * np.cross(n, e)


@functools.lru_cache(maxsize=None)
def aimed_set():
  """-> (origins, directions, the aimed points, on an edge or a vertex): 60 seeded facets each of ball, torus and needle,
  four points per facet (v0, the middle of v0 v1, 1/4 of v1 v2, the centroid), each met from outside, 50 mm away, at 0, 60
  and 80 degrees from the facet's normal"""
  rng = np.random.default_rng(17)
  O, D, P, E = [], [], [], []
  for solid in ('ball', 'torus', 'needle'):
    p = facets_of(solid)
    p = p[np.sort(rng.choice(len(p), 60, replace=False))]
    n, w = _frame(p)
    points = (p[:, 0], 0.5 * (p[:, 0] + p[:, 1]), p[:, 1] + 0.25 * (p[:, 2] - p[:, 1]), p.mean(1))
    for j, x in enumerate(points):
      for deg in (0.0, 60.0, 80.0):
        a = np.radians(deg)
        d = -np.cos(a) * n + np.sin(a) * w
        O.append(x - 50.0 * d); D.append(d); P.append(x); E.append(np.full(len(x), j < 3))
  return np.vstack(O), np.vstack(D), np.vstack(P), np.concatenate(E)


def tiny_sets():
  """{set: (origins, directions)}: per axis and sense, rays along the axis through the centre of the cube's face and 1e-3 mm
  inside each of the face's edges, and through the ball's centre; the two off-axis components are `z` of tree_cases.TINY"""
  sets = {}
  for z in tc.TINY:
    rays = []
    for a in range(3):
      b, c = (a + 1) % 3, (a + 2) % 3
      for s in (1.0, -1.0):
        h = CUBE_HALF - 1e-3
        for centre, (u, v) in [(CUBE_C, uv) for uv in ((0.0, 0.0), (h, 0.0), (-h, 0.0), (0.0, h), (0.0, -h))] + [(BALL_C, (0.0, 0.0))]:
          o, d = centre.copy(), np.full(3, z)
          o[a] -= 50.0 * s
          o[b] += u
          o[c] += v
          d[a] = s
          rays.append((o, d))
    sets[f'tiny[{z!r}]'] = gc._rows(rays)
  return sets


START_STEPS = (0.0, 0.5e-6, 3e-6, 1e-3)


@functools.lru_cache(maxsize=None)
def starts_set():
  """-> (origins, directions, the facet's centroid (NaN: none), is it recorded): origins at the centroid of 100 facets and
  0.5e-6, 3e-6 and 1e-3 mm before it along an inward direction (its own facet lies that far down the ray: recorded when
  that is more than DistanceTolerance); 200 origins inside the ball and 200 inside the torus' tube, isotropic directions"""
  rng = np.random.default_rng(19)
  p, _ = facets()
  p = p[np.sort(rng.choice(len(p), 100, replace=False))]
  n, w = _frame(p)
  u = -n + 0.3 * w
  u /= np.linalg.norm(u, axis=1)[:, None]
  c = p.mean(1)
  O = [c - s * u for s in START_STEPS]
  D = [u] * len(START_STEPS)
  P = [c] * len(START_STEPS)
  R = [np.full(len(c), s > ec.DIST_TOL) for s in START_STEPS]
  iso = rng.normal(size=(400, 3))
  iso /= np.linalg.norm(iso, axis=1)[:, None]
  r = rng.normal(size=(200, 3))
  inside_ball = BALL_C + 10.0 * rng.uniform(0, 1, (200, 1))**(1 / 3) * r / np.linalg.norm(r, axis=1)[:, None]
  phi = rng.uniform(0, 2 * np.pi, 200)
  r = rng.normal(size=(200, 3))
  inside_tube = (TORUS_C + TORUS_R * np.column_stack([np.cos(phi), np.sin(phi), np.zeros(200)])
                 + 3.0 * rng.uniform(0, 1, (200, 1))**(1 / 3) * r / np.linalg.norm(r, axis=1)[:, None])
  O += [inside_ball, inside_tube]
  D.append(iso)
  P.append(np.full((400, 3), np.nan))
  R.append(np.zeros(400, bool))
  return np.vstack(O), np.vstack(D), np.vstack(P), np.concatenate(R)


@functools.lru_cache(maxsize=None)
def length_limit_set(limit=1000.0):
  """-> (origins, directions, the aimed points, beyond): rays along the inward normal of 30 facets of the ball, aimed at the
  centroid, from limit - 1e-3 mm away (recorded) and from limit + 1e-3 mm away (nothing: the ray escapes).  Facets behind
  which (seen from the ball) the line meets nothing else"""
  p = facets_of('ball')
  n, _ = _frame(p)
  c = p.mean(1)
  free = np.array([len(w) == 0 for w in facet_crossings(c + 1e-3 * n, n, limit=4.0 * limit)])
  pick = np.nonzero(free)[0][::max(1, int(free.sum()) // 30)][:30]
  assert len(pick) == 30
  c, n = c[pick], n[pick]
  return (np.vstack([c + (limit - 1e-3) * n, c + (limit + 1e-3) * n]), np.vstack([-n, -n]), np.vstack([c, c]),
          np.r_[np.zeros(30, bool), np.ones(30, bool)])


def sets(limit=1000.0):
  """{set: (origins, directions, gallery limit)} of everything that is held row by row"""
  out = {'random': random_set() + (limit,), 'aimed': aimed_set()[:2] + (limit,), 'back': back_set() + (tc.FAR_LIMIT,)}
  out.update({k: v + (limit,) for k, v in tiny_sets().items()})
  out['starts'] = starts_set()[:2] + (limit,)
  out['length-limit'] = length_limit_set(limit)[:2] + (limit,)
  return out


@functools.lru_cache(maxsize=None)
def expected(name):
  """the reference's crossings of set `name` (unmoved frame), worked out once"""
  o, d, limit = sets()[name]
  return tuple(facet_crossings(o, d, limit))


def placed(name, far):
  """-> (gallery, origins, directions, expected points per ray) of a set on the gallery or the far gallery"""
  o, d, limit = sets()[name]
  want = expected(name)
  if far:
    return far_gallery(limit), o + T, d, [w + T for w in want]
  return gallery(0, limit), o, d, list(want)


def aimed_once(rows, o, d, points, label):
  """the aimed point is recorded exactly once among its ray's rows"""
  got = ec.per_ray(rows, o, d)
  for k, g in enumerate(got):
    assert len(g) and (np.abs(g - points[k]).max(1) < ec.TOL).sum() == 1, (label, k, o[k], d[k], points[k], g)


# ---- the faceted bench -----------------------------------------------------------------------------------------------------------
def faceted_bench(variant):
  """grid_cases.bench(faceted=True) in the variants of test_gpu_tree.py::test_interactions -> (scene, limits)"""
  return gc.bench_variant(*gc.bench(faceted=True), variant)


# ---- ties between facets (intersect_tri of csrc/odw_kernels.hip, nearest_skipping of the oracle) ---------------------------------
def wedges(n=40, swapped=False, seed=23):
  """n wedges of two facets A and B that share an edge, 30 mm apart along x, each met by one ray aimed at a point of the
  shared edge from the side on which A faces the ray and B faces away: the two t differ by rounding alone.
  -> (scene, limits, origins, directions, the aimed points); swapped: B is listed before A in every mesh"""
  rng = np.random.default_rng(seed)
  O, D, P, solids = [], [], [], []
  for k in range(n):
    base = np.array([30.0 * k, 0.0, 0.0])
    a, b = base + rng.uniform(-1, 1, 3), base + np.array([0.0, 4.0, 0.0]) + rng.uniform(-1, 1, 3)    # the shared edge
    roof = base + np.array([3.0, 2.0, 2.0]) + rng.uniform(-0.5, 0.5, 3)                              # A: b, a, roof
    back = base + np.array([3.0, 2.0, -2.0]) + rng.uniform(-0.5, 0.5, 3)                             # B: a, b, back
    v = np.array([a, b, roof, back])
    tri = np.array([[1, 0, 2], [0, 1, 3]])
    nA, nB = (np.cross(v[t[1]] - v[t[0]], v[t[2]] - v[t[0]]) for t in tri)
    x = a + rng.uniform(0.2, 0.8) * (b - a)
    d = np.array([0.3, 0.1, -1.0]) / np.linalg.norm([0.3, 0.1, -1.0])
    assert d @ nA < 0 < d @ nB                          # A faces the ray, B faces away from it
    solids.append((v, tri[::-1] if swapped else tri))
    O.append(x - 50.0 * d); D.append(d); P.append(x)
  sc, lim = ec.vacuum(lambda doc: [make.makeMesh(doc, v, tri, name=f'W{k}') for k, (v, tri) in enumerate(solids)])
  return sc, lim, np.array(O), np.array(D), np.array(P)


def facet_on_a_box(offset):
  """a box in a Mirror group whose top face lies at z = 0, and in a Vacuum group a patch of two facets `offset` mm above
  that face, met by rays from above (the patch first when offset > 0) -> (scene, limits, origins, directions)"""
  def patch(doc):
    v = np.array([[-5.0, -5.0, offset], [5.0, -5.0, offset], [5.0, 5.0, offset], [-5.0, 5.0, offset]])
    return [make.makeMesh(doc, v, np.array([[0, 1, 2], [0, 2, 3]]), name='Patch')]
  sc, lim = ec.baked([('Mirror', lambda doc: [ec.centred_box(doc, 'B', (-8, -8, -3), (8, 8, 0))], {}), ('Vacuum', patch, {})])
  rng = np.random.default_rng(29)
  x = np.column_stack([rng.uniform(-4, 4, (64, 2)), np.zeros(64)])
  d = np.column_stack([rng.uniform(-0.3, 0.3, (64, 2)), -np.ones(64)])
  d /= np.linalg.norm(d, axis=1)[:, None]
  return sc, lim, x - 20.0 * d, d


def first_rows(rows, o):
  """-> per ray its first row, the rows of a ray standing in the order it recorded them (index into rows; -1: none)"""
  ray = (rows['tag'] & np.uint64(0xFFFFFFFFFFFF)).astype(np.int64)
  out = np.full(len(o), -1)
  which, at = np.unique(ray, return_index=True)
  out[which] = at
  return out
