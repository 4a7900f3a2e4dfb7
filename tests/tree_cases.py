"""What the binary-tree kernel (odw_trace_kernel<true, ...>, nearest<BVH = true> of csrc/odw_kernels.hip) needs beyond the
scenes, rays and closed forms of tests/grid_cases.py: tests/test_tree_cases.py checks the sets below against the CPU
oracle, tests/test_gpu_tree.py traces them through the tree.

  far placement      the two lattices with every solid and every origin moved by T = (3000, -7000, 11000) mm: the walk
                     culls with (float)start, (float)(1 / d) and float32 boxes, and neither the box edges (c +- 2 +- slack)
                     nor the origins are float32 numbers there.  The second random set, whose origins lie a further 1000 mm
                     back along -d, is traced in the same scene under MaxRayLength = 2000 mm, so that it still reaches
                     the solids (the aimed sets keep the limit they are aimed at, 1000 mm);
  tiny components    on the moved lattice, rays through the centres of a row of spheres and 1.999 mm beside it, the off-axis
                     direction components from grid_cases.ZEROS and +-1e-40, +-1e-30: the reciprocal of 1e-40 overflows
                     float32 (and not float64), that of 1e-30 comes within 1e8 of its end, a zero's is infinite and
                     (lo - o) * inf is NaN where the rounded origin meets an edge;
  facets             the mixed lattice with every cube a mesh of 12 triangles: the expected rows are the box rule's.  Rays
                     through the centres of the faces, and through the points at 1/4 and 3/4 of the diagonal of a face,
                     the edge its two triangles share: one crossing there;
  segment chains     in a vacuum case the segments of a ray run from its origin through its expected crossings in order;
                     the closing segment (from the last crossing, max_ray_length long) is taken from the oracle."""
import functools

import numpy as np

import ellipsoid_cases as ec
import grid_cases as gc
from freecad.optics_design_workbench_amd.freecad_elements import make

T = np.array([3000.0, -7000.0, 11000.0])
FAR_LIMIT = 2000.0                  # MaxRayLength of the moved scenes that take the second random set
BACK = 1000.0                       # the second random set starts this much further away
TINY = gc.ZEROS + (1e-40, -1e-40, 1e-30, -1e-30)
SEG_RAY = np.uint64(0xFFFFFFFFFF)   # the ray of a segment row's tag (40 bits; then 12 of ordinal, 12 of medium + 1)


def _moved(solids, by):
  return [(kind, np.asarray(a, float) + by, (np.asarray(b, float) + by) if kind == 'box' else b) for kind, a, b in solids]


@functools.lru_cache(maxsize=None)
def far_case(name, limit=1000.0):
  """the lattice / the mixed lattice moved by T (grid figures as grid_cases counts them: the same planes, moved)"""
  assert name in ('lattice', 'mixed')
  return gc.Case(_moved(gc.case(name).solids, T), 80, 80, True, MaxRayLength=limit)


def far_sets(name):
  """{set: (origins, directions)} of far_case(name): the aimed sets of grid_cases and its random set, moved by T"""
  sets = dict(gc.aimed_sets(name), random=gc.random_set(name))
  return {k: (o + T, d) for k, (o, d) in sets.items()}


def far_back_set(name):
  """of far_case(name, FAR_LIMIT): the random set from 1000 mm further back.

  The CPU oracle is no yardstick at ec.TOL on this set.  Like the reference (ray.py:348-349) it takes a ray's direction in
  a primitive's frame as the difference of two transformed points, xf(start + d) - xf(start): numbers of 11000 mm, an ulp
  of 1.8e-12 mm each, so the local direction is off by a few 1e-12 and a crossing 1050 mm down the ray by a few 1e-9 mm
  (measured: 2.5e-9 mm on the lattice, 7.2e-9 mm on the mixed lattice; on the first random set, 100 mm down the ray,
  4e-10).  The kernels rotate the direction itself.  So on this set the device is held to the closed form within ec.TOL,
  and to the oracle in rows, tags and counters only; the oracle's own distance is printed."""
  o, d = gc.random_set(name)
  return o - BACK * d + T, d


COORD_ULPS = 16.0                   # roundings of coordinate-sized numbers a crossing may have gone through (see below)
BUDGET = 0.5 * ec.TOL               # of the tolerance, for what conditioning makes of them


def ill_conditioned(c, o, d):
  """-> the rays of a far-placed random set that float64 itself cannot hold to ec.TOL, by the closed form alone.

  Far from the origin a coordinate of 11000 mm carries an ulp of 1.8e-12 mm.  Whoever computes a crossing in float64
  rounds coordinate-sized numbers a handful of times (start - centre or the local frame, start + t d, the reference's
  frame changes there and back): COORD_ULPS = 16 ulp of the largest coordinate is allowed for that chain, e.  The kernels
  and the oracle solve a sphere by the textbook quadratic t = -b - sqrt(b^2 - c) with b = oc . d, c = |oc|^2 - r^2: b^2
  and c are each rounded once at their own size, L^2 for a ray that starts L mm away, and cancel -- 2 ulp(L^2) more on
  the discriminant, q.  A discriminant off by 2 r e + q moves the root by (2 r e + q) / (2 sqrt(disc)): near-grazing
  lines amplify it.  A box face (slab rule, t = (lo - o) / d_a) moves the point by e / |d_a|: shallow lines amplify it.
  A ray is excluded when either exceeds BUDGET = TOL / 2.  (grid_cases' own rule, disc < 1e-4, is sized for scenes at
  the origin met from 200 mm away; it stays in force beside this one.)"""
  LD = gc.LD
  ol, dl = np.asarray(o, LD), gc._unit(d)
  e = COORD_ULPS * float(np.spacing(np.abs(o).max()))
  out = np.zeros(len(o), bool)
  for kind, a, b in c.solids:
    if kind == 'sphere':
      oc = ol - np.asarray(a, LD)
      bh, oo = (oc * dl).sum(-1), (oc * oc).sum(-1)
      disc = np.asarray(bh * bh - (oo - LD(b) * LD(b)), float)
      q = 2.0 * np.spacing(np.maximum(np.asarray(bh * bh, float), np.asarray(oo, float)))
      with np.errstate(invalid='ignore'):
        out |= (disc > 0) & ((2.0 * float(b) * e + q) > BUDGET * 2.0 * np.sqrt(np.where(disc > 0, disc, 1.0)))
    elif kind == 'box':
      with np.errstate(divide='ignore', invalid='ignore'):
        ta, tb = (np.asarray(a, LD) - ol) / dl, (np.asarray(b, LD) - ol) / dl
      near, far = np.fmin(ta, tb), np.fmax(ta, tb)
      hit = near.max(-1) < far.min(-1)
      rows = np.arange(len(o))
      through = np.abs(np.asarray(dl, float))
      shallow = np.minimum(through[rows, near.argmax(-1)], through[rows, far.argmin(-1)])
      out |= hit & (e > BUDGET * shallow)
    else:
      raise ValueError(kind)
  return out


def same_crossings(rows, o, d, want, excluded, label):
  """every ray that is not excluded records as many points as the closed form says -> the worst distance (printed, not held)"""
  got = ec.per_ray(rows, o, d)
  worst = 0.0
  for k, (g, w) in enumerate(zip(got, want)):
    if excluded[k]:
      continue
    assert len(g) == len(w), (label, k, o[k], d[k], g, w)
    if len(w):
      worst = max(worst, float(np.abs(g - w).max()))
  print(f'{label}: {len(o)} rays, {int(excluded.sum())} excluded, the rows of the closed form, worst {worst:.3e} mm')
  return worst


def far_expected(c, o, d):
  """expected_for of a far random set: its exclusions and the ill-conditioned rays"""
  want, excluded = gc.expected_for(c, o, d)
  return want, excluded | ill_conditioned(c, o, d)


def tiny_sets():
  """{set: (origins, directions)} on the moved lattice: per axis and sense, through the centres of a row and 1.999 mm beside
  it; the two off-axis components are `z`"""
  sets = {}
  for z in TINY:
    rays = []
    for a in range(3):
      b, c = (a + 1) % 3, (a + 2) % 3
      for s in (1.0, -1.0):
        for u, v in ((10.0, 20.0), (10.0 + 1.999, 20.0)):
          o, d = np.zeros(3), np.full(3, z)
          o[a], o[b], o[c] = (-50.0 if s > 0 else gc.PITCH * (gc.SHAPE[a] - 1) + 50.0), u, v
          d[a] = s
          rays.append((o + T, d))
    sets[f'tiny[{z!r}]'] = gc._rows(rays)
  return sets


# ---- facets: every cube of the mixed lattice as 12 triangles -----------------------------------------------------------------
# the corners of a face seen from outside, counter-clockwise: (-, -), (+, -), (+, +), (-, +) along the axes (a + 1, a + 2)
# on the upper side, mirrored on the lower one; its triangles (0, 1, 2) and (0, 2, 3) share the diagonal 0 -- 2
def _cube_mesh(lo, hi):
  lo, hi = np.asarray(lo, float), np.asarray(hi, float)
  v = np.array([[(hi if (k >> a) & 1 else lo)[a] for a in range(3)] for k in range(8)])
  tri = []
  for a in range(3):
    b, c = (a + 1) % 3, (a + 2) % 3
    for side in (0, 1):
      q = [(side << a) | (sb << b) | (sc << c) for sb, sc in ((0, 0), (1, 0), (1, 1), (0, 1))]
      if not side:
        q = [q[0], q[3], q[2], q[1]]                 # (seen from below: the other sense, the same diagonal)
      tri += [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
  return v, np.array(tri)


class FacetCase:
  """the attributes of grid_cases.Case the tests use; solids: the closed form's (spheres and boxes)"""
  oracle_knows, spheres = True, False

  def __init__(self, solids):
    self.solids = solids

    def elems(doc):
      out = []
      for i, (kind, a, b) in enumerate(solids):
        if kind == 'sphere':
          out.append(make.makeSphere(doc, f'S{i}', float(b), base=tuple(float(x) for x in a)))
        else:
          out.append(make.makeMesh(doc, *_cube_mesh(a, b), name=f'M{i}'))
      return out
    self.sc, self.lim = ec.vacuum(elems)


@functools.lru_cache(maxsize=None)
def facet_case():
  return FacetCase(gc.case('mixed').solids)


def _through(points, normals, tilts):
  """rays that meet `points` (on faces with the outward `normals`) coming from outside, 30 mm away, tilted by `tilts`"""
  d = -np.asarray(normals, float) + np.asarray(tilts, float)
  d /= np.linalg.norm(d, axis=1)[:, None]
  return np.asarray(points, float) - 30.0 * d, d


def _faces():
  """(centre, outward normal, half diagonal (towards corner 2), tilt in the face's plane) of every face of every cube"""
  out = []
  for kind, lo, hi in gc.case('mixed').solids:
    if kind != 'box':
      continue
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    for a in range(3):
      b, c = (a + 1) % 3, (a + 2) % 3
      for side in (-1.0, 1.0):
        n, p, diag, tilt = np.zeros(3), mid.copy(), np.zeros(3), np.zeros(3)
        n[a] = side
        p[a] += side * half[a]
        diag[b], diag[c] = half[b], half[c]
        tilt[b], tilt[c] = 0.13, -0.07
        out.append((p, n, diag, tilt))
  return out


def face_centres():
  p, n, _, tilt = zip(*_faces())
  return _through(p, n, tilt)


def face_diagonals():
  """through the points at 1/4 and 3/4 of the edge the two triangles of a face share -> (origins, directions, the points)"""
  p, n, tilt = [], [], []
  for mid, normal, diag, tl in _faces():
    for f in (-0.5, 0.5):
      p.append(mid + f * diag)
      n.append(normal)
      tilt.append(tl)
  o, d = _through(p, n, tilt)
  return o, d, np.array(p)


def facet_sets():
  return {'random': gc.random_set('mixed'), 'face centres': face_centres(), 'face diagonals': face_diagonals()[:2]}


# ---- segment chains ---------------------------------------------------------------------------------------------------------------
def seg_fields(segs):
  """-> (ray, ordinal) of segment rows"""
  tag = segs['tag']
  return (tag & SEG_RAY).astype(np.int64), ((tag >> np.uint64(40)) & np.uint64(0xFFF)).astype(np.int64)


def held_segments(segs, ref, o, d, want, excluded, label, by_name=(), limit=1000.0, ref_points=True, ref_kept_only=False):
  """the segment rows of a vacuum case against the chain origin -> crossings (closed form) and against the oracle's rows
  `ref`: tags equal, p1 / p2 within ec.TOL of both; every ray that is not excluded has one segment per crossing, from
  the point before it, and a closing one of the length limit along its direction -> worst distance"""
  worst = 0.0
  if ref is not None:                                                        # (None: a scene the oracle does not know)
    assert np.array_equal(segs['tag'], ref['tag']), label
    # (points: every row; ref_kept_only: those of the rays that are not excluded -- the far random sets)
    kept = ~np.asarray(excluded)[seg_fields(segs)[0]] if ref_kept_only else np.ones(len(segs), bool)
    if ref_points and kept.any():                                            # (not on far_back_set: see there)
      worst = float(max(np.abs(segs['p1'] - ref['p1'])[kept].max(), np.abs(segs['p2'] - ref['p2'])[kept].max()))
  assert np.array_equal(segs['power'], np.ones(len(segs))), label
  ray, ordinal = seg_fields(segs)
  order = np.lexsort((ordinal, ray))
  assert np.array_equal(order, np.arange(len(segs))), label                 # sorted by (ray, ordinal)
  starts = np.searchsorted(ray, np.arange(len(o) + 1))
  unit = d / np.linalg.norm(d, axis=1)[:, None]
  chained = 0
  for k in range(len(o)):
    s = segs[starts[k]:starts[k + 1]]
    if excluded[k] or k in by_name:
      continue
    chain = np.vstack([o[k][None, :], want[k]])
    assert len(s) == len(chain), (label, k, len(s), len(chain))
    assert np.array_equal(ordinal[starts[k]:starts[k + 1]], np.arange(len(chain))), (label, k)
    worst = max(worst, float(np.abs(s['p1'] - chain).max()), float(np.abs(s['p2'][:-1] - chain[1:]).max()) if len(chain) > 1 else 0.0)
    # the closing segment: the oracle's (asserted above), which runs max_ray_length along the direction
    worst = max(worst, float(np.abs(s['p2'][-1] - (chain[-1] + limit * unit[k])).max()))
    chained += len(chain)
  print(f'{label}: {len(segs)} segments, {chained} held by the chain, worst {worst:.3e} mm')
  assert worst < ec.TOL, label
  return worst
