"""Scenes and closed forms of the conicoid tests (tests/test_conicoid.py, tests/test_gpu_conicoid.py).  The CPU oracle
does not know primitive kind 8, so every expectation is worked out here with numpy in float64: a line against
x^2 + y^2 + (1 + K) z^2 = 2 R z, 0 <= z <= H as the interval it spends inside that convex solid, against a box by the
slab rule, booleans of the two by interval arithmetic along the line; the hyperbolic mirror and the aberration-free
lens by the vector laws of reflection and refraction.  A second reading of the documents (`feature_member`: point
membership straight from the features, the part of tests/csg_reference.py these documents need plus the conicoid)
holds the bake."""
import numpy as np

from ellipsoid_cases import (DIST_TOL, PLACEMENTS, POWER_TOL, TOL, baked, box_distance, box_interval, centred_box, document,  # noqa: F401
                             per_ray, point_line_distance, random_lines, to_world, vacuum)
from freecad.optics_design_workbench_amd.freecad_elements import make

R0 = 10.0
# (conic constant, height): one sheet of a hyperboloid, the paraboloid, a prolate cap, a spherical cap, an oblate cap
# (the last up to 0.8 of its half, H <= R / (1 + K) = 5)
CASES = [(-2.25, 8.0), (-1.0, 8.0), (-0.5, 8.0), (0.0, 8.0), (1.0, 4.0)]
IDS = ['hyperboloid', 'paraboloid', 'prolate', 'spherical', 'oblate']
RIM_TOL = 1e-6             # a crossing closer to the rim circle than this may be left out
TANGENT_CHORD = 3e-4       # a chord of a line that is tangent within 1e-9 mm: sqrt(8 r 1e-9) for r up to 11 mm


def rim_of(R, K, H):
  return np.sqrt(2.0 * R * H - (1.0 + K) * H * H)


def sag(rho, R, K):
  return rho * rho / (R + np.sqrt(R * R - (1.0 + K) * rho * rho))


def conicoid(doc, name, R, K, H, **kw):
  return make.makeConicoid(doc, name, R, K, H, **kw)


# ---- closed forms -------------------------------------------------------------------------------------------------
def q_of(x, R, K):
  x = np.asarray(x, float)
  return x[..., 0]**2 + x[..., 1]**2 + (1.0 + K) * x[..., 2]**2 - 2.0 * R * x[..., 2]


def member(x, R, K, H):
  x = np.asarray(x, float)
  return (q_of(x, R, K) < 0) & (x[..., 2] > 0) & (x[..., 2] < H)


def distance(x, R, K, H):
  """the kernels' trimming distance: max(q / (2 |g|), z - H, -z), g = (x, y, (1 + K) z - R)"""
  x = np.asarray(x, float)
  g = np.sqrt(x[..., 0]**2 + x[..., 1]**2 + ((1.0 + K) * x[..., 2] - R)**2)
  return np.maximum(np.maximum(0.5 * q_of(x, R, K) / np.maximum(g, 1e-150), x[..., 2] - H), -x[..., 2])


def rim_distance(x, R, K, H):
  """distance of the points x from the circle in which the conic surface meets the cap"""
  x = np.asarray(x, float)
  return np.hypot(np.hypot(x[..., 0], x[..., 1]) - rim_of(R, K, H), x[..., 2] - H)


def conicoid_interval(o, d, R, K, H):
  """the parameters t0 <= t1 between which the lines o + t d (rows, the conicoid's frame) are inside the solid (it is
  convex: one interval); NaN where they miss.  Candidates are the roots of the quadric (none, one for a line along an
  asymptote, two) and the planes z = 0 and z = H; a piece between two neighbours is inside if its middle is."""
  o, d = np.atleast_2d(np.asarray(o, float)), np.atleast_2d(np.asarray(d, float))
  kk = 1.0 + K
  t0, t1 = np.full(len(o), np.nan), np.full(len(o), np.nan)
  for i, (p, u) in enumerate(zip(o, d)):
    a = u[0] * u[0] + u[1] * u[1] + kk * u[2] * u[2]
    b = p[0] * u[0] + p[1] * u[1] + (kk * p[2] - R) * u[2]
    c = p[0] * p[0] + p[1] * p[1] + kk * p[2] * p[2] - 2.0 * R * p[2]
    ts = []
    if abs(a) <= 1e-14 * (u[0] * u[0] + u[1] * u[1] + abs(kk) * u[2] * u[2]):
      if b != 0:
        ts.append(-c / (2.0 * b))
    elif b * b - a * c > 0:
      w = -(b + np.copysign(np.sqrt(b * b - a * c), b))
      ts += [w / a] + ([c / w] if w != 0 else [])
    if u[2] != 0:
      ts += [(0.0 - p[2]) / u[2], (H - p[2]) / u[2]]
    ts = sorted(ts)
    inside = [bool(member(p + 0.5 * (ta + tb) * u, R, K, H)) and tb > ta for ta, tb in zip(ts[:-1], ts[1:])]
    if any(inside):
      first, last = inside.index(True), len(inside) - 1 - inside[::-1].index(True)
      assert all(inside[first:last + 1])                       # (convex)
      t0[i], t1[i] = ts[first], ts[last + 1]
  return t0, t1


def minus(A, B):
  """intervals of A (a list of (t0, t1)) outside the interval B"""
  out = []
  for a0, a1 in A:
    if not np.isfinite(B[0]) or B[1] <= a0 or B[0] >= a1:
      out.append((a0, a1))
      continue
    if B[0] > a0:
      out.append((a0, B[0]))
    if B[1] < a1:
      out.append((B[1], a1))
  return out


def feature_member(obj):
  """membership of points (the coordinates of obj's container) in the solid obj, read straight from the features:
  Part::Box, Part::Cylinder, the conicoid, Part::MultiCommon, Part::MultiFuse, Part::Cut"""
  inv = obj.Placement.inverse().m
  local = lambda p: p @ inv[:3, :3].T + inv[:3, 3]
  t = obj.TypeId
  if t == 'Part::Box':
    L = np.array([obj.Length, obj.Width, obj.Height], float)
    return lambda p: np.all((local(p) > 0) & (local(p) < L), axis=1)
  if t == 'Part::Cylinder':
    return lambda p: (local(p)[:, 0]**2 + local(p)[:, 1]**2 < float(obj.Radius)**2) & (local(p)[:, 2] > 0) & (local(p)[:, 2] < float(obj.Height))
  if t == 'Part::FeaturePython' and obj.ProxyClass == 'Conicoid':
    return lambda p: member(local(p), float(obj.VertexRadius), float(obj.ConicConstant), float(obj.Height))
  kids = [feature_member(c) for c in (obj.Shapes if t.startswith('Part::Multi') else (obj.Base, obj.Tool))]
  if t == 'Part::MultiCommon':
    return lambda p: np.logical_and.reduce([k(local(p)) for k in kids])
  if t == 'Part::MultiFuse':
    return lambda p: np.logical_or.reduce([k(local(p)) for k in kids])
  assert t == 'Part::Cut', t
  return lambda p: kids[0](local(p)) & ~kids[1](local(p))


# ---- scene 1: the explicit lines of the crossings test ----------------------------------------------------------------
def crossing_lines(K, H, R=R0):
  """(origins, directions, expected points per line, excluded lines) in the conicoid's own frame; every origin lies
  clear of the surface, so a line records the ends of its interval that lie ahead"""
  rim = rim_of(R, K, H)
  O, D = [], []

  def add(o, d):
    d = np.asarray(d, float)
    O.append(np.asarray(o, float)); D.append(d / np.linalg.norm(d))

  def through(p, d, back):
    d = np.asarray(d, float) / np.linalg.norm(d)
    add(np.asarray(p, float) - back * d, d)

  # along the axis, both ways; parallel to it
  add([0, 0, -100.0], [0, 0, 1]); add([0, 0, 100.0], [0, 0, -1])
  for fu, fv in ((0.5, 0.0), (0.0, -0.6), (0.3, 0.4), (-0.65, 0.65)):
    add([fu * rim, fv * rim, -80.0], [0, 0, 1])
  add([0.2 * rim, -0.1 * rim, 90.0], [0, 0, -1])
  # through the vertex, slanted
  for u in ((1, 0, 1), (1, -2, 3), (-3, 1, 2.5), (0.2, 0.1, 1), (2, 1, 0.5)):
    through([0, 0, 0], u, 50.0)
  # chords: across the axis and beside it, level and slanted
  for p, u in (([0, 0, 0.3 * H], (1, 0, 0)), ([0, 0.2 * rim, 0.7 * H], (1, 0, 0)), ([0.1 * rim, 0, 0.5 * H], (0, 1, 0)),
               ([0, 0, 0.5 * H], (1, 1, 0.2)), ([0.2 * rim, -0.1 * rim, 0.6 * H], (-1, 2, 0.3)), ([0, 0.3 * rim, 0.8 * H], (3, 1, -0.4))):
    through(p, u, 70.0)
  # through the rim -+ 1e-6: a level line across the axis 1e-6 below the cap (its two crossings lie more than 1e-6 from
  # the rim circle), and a line in the cap's plane, along the rim's tangent, 1e-6 outside it (nothing)
  through([0, 0, H - 1e-6], (1, 0, 0), 60.0)
  through([0, 0, H - 1e-6], (0, -1, 0), 60.0)
  through([rim + 1e-6, 0, H], (0, 1, 0), 60.0)
  through([0, -(rim + 1e-6), H], (1, 0, 0), 60.0)
  # a level line that clears the surface by 1e-9 mm (nothing) beside one 1e-6 mm inside (its chord): at half height
  # the surface's normal makes the angle with the level plane whose cosine is rho / |g|
  zc = 0.5 * H
  rc = np.sqrt(2.0 * R * zc - (1.0 + K) * zc * zc)
  cosn = rc / np.hypot(rc, (1.0 + K) * zc - R)
  through([rc + TOL / cosn, 0, zc], (0, 1, 0), 60.0)
  through([rc - DIST_TOL / cosn, 0, zc], (0, 1, 0), 60.0)
  # rays that start inside: three leave through the cap (all such a line meets ahead), three through the surface
  inside = [([0, 0, 0.5 * H], (0, 0, 1)), ([0.2 * rim, 0.1 * rim, 0.7 * H], (0.1, -0.2, 1)), ([-0.1 * rim, 0, 0.4 * H], (0.3, 0.2, 1)),
            ([0, 0, 0.5 * H], (0, 0, -1)), ([0.1 * rim, 0.1 * rim, 0.6 * H], (1, 0.5, -0.2)), ([0, -0.2 * rim, 0.5 * H], (-1, -1, -1))]
  for p, u in inside:
    add(p, u)
  n_special = 0
  if K < -1.0:
    # along an asymptote direction (the leading coefficient vanishes up to rounding), steeper than it (negative: the
    # second root lies on the other sheet), and two lines aimed through the absent sheet, below z = 2 R / (1 + K)
    s = 1.0 / np.sqrt(-(1.0 + K))
    through([0, 0, 0.5 * H], (s, 0, 1), 60.0)
    through([0.1 * rim, 0, 0.4 * H], (-0.6 * s, 0.5 * s, 1), 60.0)
    through([0, 0, 0.5 * H], (0.3 * s, 0, 1), 60.0)
    through([0, 0, 2.0 * R / (1.0 + K) - 4.0], (1, 0, 0), 60.0)
    add([3.0 * R, 0, -80.0], [0, 0, 1])
    n_special = 5
  O, D = np.array(O), np.array(D)
  t0, t1 = conicoid_interval(O, D, R, K, H)
  want, excluded = [], np.zeros(len(O), bool)
  for k in range(len(O)):
    ts = [t for t in (t0[k], t1[k]) if np.isfinite(t) and t > 0]
    pts = np.array([O[k] + t * D[k] for t in ts]).reshape(-1, 3)
    want.append(pts)
    excluded[k] = bool(len(pts) and rim_distance(pts, R, K, H).min() < RIM_TOL) or (np.isfinite(t0[k]) and t1[k] - t0[k] < TANGENT_CHORD)
    if np.isfinite(t0[k]):
      assert abs(t0[k]) > 1e-3 and abs(t1[k]) > 1e-3               # (no origin on the surface)
  first_inside = len(O) - n_special - len(inside)
  counts = dict(lines=len(O), none=sum(len(w) == 0 for w in want), one=sum(len(w) == 1 for w in want), first_inside=first_inside,
                special=n_special)
  return O, D, want, excluded, counts


# ---- scene 2: booleans with a box --------------------------------------------------------------------------------------
K2, H2 = CASES[0]
BLOCK = (np.array([-20.0, -20.0, -6.0]), np.array([20.0, 20.0, 5.0]))      # Cut(block, conicoid): a cavity open at the top
DRILL = (np.array([-3.0, -4.0, -2.0]), np.array([5.0, 2.0, 20.0]))         # Cut(conicoid, drill): a square hole
HALF = (np.array([-30.0, -30.0, -5.0]), np.array([4.0, 30.0, 6.0]))        # Common(conicoid, half)
TRIMS = ['cut-block', 'cut-conicoid', 'common']


def trim_scene(case, kind='Vacuum', **props):
  if case == 'cut-block':
    elems = lambda d: [make.makeCut(d, centred_box(d, 'B', *BLOCK), conicoid(d, 'C', R0, K2, H2))]
  elif case == 'cut-conicoid':
    elems = lambda d: [make.makeCut(d, conicoid(d, 'C', R0, K2, H2), centred_box(d, 'B', *DRILL))]
  else:
    elems = lambda d: [make.makeCommon(d, [conicoid(d, 'C', R0, K2, H2), centred_box(d, 'B', *HALF)])]
  return baked([(kind, elems, props)])


def trim_member(case, x):
  c = member(x, R0, K2, H2)
  lo, hi = {'cut-block': BLOCK, 'cut-conicoid': DRILL, 'common': HALF}[case]
  b = np.all((x > lo) & (x < hi), axis=-1)
  return {'cut-block': b & ~c, 'cut-conicoid': c & ~b, 'common': c & b}[case]


def trim_distance(case, x):
  """the distance rule of the result: max over a conjunction, the tool's distance negated"""
  c = distance(x, R0, K2, H2)
  b = box_distance(x, *{'cut-block': BLOCK, 'cut-conicoid': DRILL, 'common': HALF}[case])
  return {'cut-block': np.maximum(b, -c), 'cut-conicoid': np.maximum(c, -b), 'common': np.maximum(c, b)}[case]


def trim_lines(case):
  o, d = random_lines(2000, seed={'cut-block': 21, 'cut-conicoid': 22, 'common': 23}[case], span=12.0, back=100.0)
  return o, d


def trim_expected(case, o, d):
  """-> (expected points per line, excluded lines)"""
  box = {'cut-block': BLOCK, 'cut-conicoid': DRILL, 'common': HALF}[case]
  c0, c1 = conicoid_interval(o, d, R0, K2, H2)
  b0, b1 = box_interval(o, d, *box)
  want, excluded = [], np.zeros(len(o), bool)
  for k in range(len(o)):
    C, B = (c0[k], c1[k]), (b0[k], b1[k])
    if case == 'cut-block':
      pieces = minus([B] if np.isfinite(B[0]) else [], C)
    elif case == 'cut-conicoid':
      pieces = minus([C] if np.isfinite(C[0]) else [], B)
    else:
      pieces = [(max(C[0], B[0]), min(C[1], B[1]))] if np.isfinite(C[0]) and np.isfinite(B[0]) and max(C[0], B[0]) < min(C[1], B[1]) else []
    # (a crossing of one operand within 10 distTol of the other's surface lies at a trimming edge; pieces and chords
    #  shorter than 1e-3 mm are grazing; crossings near the rim circle)
    for t, other in ((C[0], 'box'), (C[1], 'box'), (B[0], 'con'), (B[1], 'con')):
      if np.isfinite(t):
        x = o[k] + t * d[k]
        sd = box_distance(x, *box) if other == 'box' else distance(x, R0, K2, H2)
        excluded[k] |= abs(sd) < 10 * DIST_TOL
        if other == 'box':
          excluded[k] |= rim_distance(x, R0, K2, H2) < 10 * RIM_TOL
    for t0, t1 in pieces + [C, B]:
      if np.isfinite(t0) and t1 - t0 < 1e-3:
        excluded[k] = True
    ts = [t for piece in pieces for t in piece]
    want.append(np.array([o[k] + t * d[k] for t in ts]).reshape(-1, 3))
  return want, excluded


# ---- scenes 3 and 4: the hyperbolic mirror, the aberration-free lens -----------------------------------------------------
MIRROR = dict(R=10.0, K=-2.25, H=8.0)
E = 1.5                                              # sqrt(-K)
F_INNER = np.array([0.0, 0.0, 10.0 / (E + 1.0)])     # inside the sheet
F_OUTER = np.array([0.0, 0.0, -10.0 / (E - 1.0)])    # the other sheet's
LENS = dict(n=1.5, f=40.0, R=20.0, K=-2.25, H=6.0)   # R = f (n - 1), K = -n^2


def normal(x, R, K):
  g = np.stack([x[:, 0], x[:, 1], (1.0 + K) * x[:, 2] - R], axis=1)
  return g / np.linalg.norm(g, axis=1)[:, None]


def cone_directions(n, half_angle, axis, seed):
  """n unit vectors within half_angle of +-z (axis = +-1), uniform over the cap"""
  rng = np.random.default_rng(seed)
  cz = 1.0 - rng.uniform(0, 1, n) * (1.0 - np.cos(half_angle))
  phi = rng.uniform(0, 2 * np.pi, n)
  s = np.sqrt(1.0 - cz * cz)
  return np.stack([s * np.cos(phi), s * np.sin(phi), axis * cz], axis=1)


def mirror_convex_rays(n=4100):
  """rays from 30 mm below, aimed at the inner focus: they meet the sheet from outside"""
  u = cone_directions(n, np.radians(50.0), 1.0, 31)
  return F_INNER - 30.0 * u, u


def mirror_concave_rays(n=4100):
  """rays that leave the inner focus downwards, into the cavity's wall"""
  u = cone_directions(n, np.radians(75.0), -1.0, 32)
  return np.tile(F_INNER, (n, 1)), u


def mirror_reference(o, d, concave):
  """numpy's own reflection: -> (hit points, reflected directions, distance of the outer focus from the reflected lines)"""
  t0, t1 = conicoid_interval(o, d, **MIRROR)
  x = o + (t1 if concave else t0)[:, None] * d
  nn = normal(x, MIRROR['R'], MIRROR['K'])
  r = d - 2.0 * (d * nn).sum(1)[:, None] * nn
  return x, r, point_line_distance(F_OUTER, x, x + r)


def lens_rays(n=4100):
  rng = np.random.default_rng(33)
  rim = rim_of(LENS['R'], LENS['K'], LENS['H'])
  rho, phi = 0.95 * rim * np.sqrt(rng.uniform(0, 1, n)), rng.uniform(0, 2 * np.pi, n)
  return np.stack([rho * np.cos(phi), rho * np.sin(phi), np.full(n, 50.0)], axis=1), np.tile([0.0, 0.0, -1.0], (n, 1))


def lens_reference(o, d):
  """through the cap undeviated, out of the glass at the hyperboloid by Snell's law in vector form: -> (points where
  the rays leave, directions after, distance of (0, 0, -f) from the lines after)"""
  x = np.stack([o[:, 0], o[:, 1], sag(np.hypot(o[:, 0], o[:, 1]), LENS['R'], LENS['K'])], axis=1)
  nn = normal(x, LENS['R'], LENS['K'])                          # outward: the side the ray leaves into
  mu = LENS['n'] / 1.0
  ci = (d * nn).sum(1)
  ct = np.sqrt(1.0 - mu * mu * (1.0 - ci * ci))
  r = mu * d + (ct - mu * ci)[:, None] * nn
  return x, r, point_line_distance([0.0, 0.0, -LENS['f']], x, x + r)


def conic_lens_member(x, radius1, conic1, radius2, conic2, thickness, diameter):
  """the defining inequality of make.makeConicLens: rho <= diameter / 2, sag1(rho) <= z <= thickness + sag2(rho)"""
  rho = np.hypot(x[:, 0], x[:, 1])
  def s(r, k):
    if np.isinf(r):
      return np.zeros_like(rho)
    with np.errstate(invalid='ignore'):
      return rho * rho / (r * (1.0 + np.sqrt(1.0 - (1.0 + k) * rho * rho / (r * r))))
  with np.errstate(invalid='ignore'):
    return (rho < diameter / 2) & (x[:, 2] > s(radius1, conic1)) & (x[:, 2] < thickness + s(radius2, conic2))


def conic_lens_margin(x, radius1, conic1, radius2, conic2, thickness, diameter):
  """a lower bound of the distance of x from the lens's boundary, good enough to leave out the points near it"""
  eps = 1e-4
  out = np.ones(len(x), bool)
  for dx in ((eps, 0, 0), (-eps, 0, 0), (0, eps, 0), (0, -eps, 0), (0, 0, eps), (0, 0, -eps)):
    out &= conic_lens_member(x + np.array(dx), radius1, conic1, radius2, conic2, thickness, diameter) == \
           conic_lens_member(x, radius1, conic1, radius2, conic2, thickness, diameter)
  return out
