"""Point-source ray generation held to exact arithmetic: what the tests of the generation side share (host only).

Two observations carry everything here.  (1) With the identity tables phi_edges = phi_cdf = t_edges = t_cdf = [0, 1]
the inverse cdf returns 1 * (u - 0) + 0 = u, so a sampler shows its uniforms; an independent numpy Philox4x32-10
(below, held to the Random123 known answers) says what they must be.  (2) The host therefore knows every ray's
uniforms ahead of the launch, and a table whose cdf knots are some rays' own u -- or the double next to it -- puts
chosen rays exactly on a knot, one ulp below it and one ulp above it, with edge values of the test's choosing (an angle
of exactly pi / 2, say).  No entry point of its own is needed.

References: `exact_inverse` (the piecewise-linear inverse in numpy.longdouble, at 200 bits in mpmath for the rays on
or beside a knot), `exact_row` (a full argmin over the mid-points), `exact_ray` (longdouble) / `exact_ray_mp`.
Cases are made once per process and never changed."""
import functools
import types

import mpmath
import numpy as np

L = np.longdouble
EPS = 2.0 ** -53
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0.0])

# ---------------------------------------------------------------- Philox4x32-10 (Salmon et al., SC'11)
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
  """counter: four uint32 words (scalars or arrays of one shape), key: two words -> four uint32 arrays"""
  c0, c1, c2, c3 = (np.atleast_1d(np.asarray(w, dtype=np.uint64)) & _M32 for w in counter)
  k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
  for _ in range(10):
    p0 = np.uint64(0xD2511F53) * c0            # (32 x 32 bits: the product fits 64)
    p1 = np.uint64(0xCD9E8D57) * c2
    c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & _M32
    k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
  return tuple(w.astype(np.uint32) for w in (c0, c1, c2, c3))


def u53(a, b):
  """53-bit uniform in [0, 1) of two words (numpy's legacy construction): exact in float64"""
  hi = (np.asarray(a, dtype=np.uint64) >> np.uint64(5)).astype(np.float64)
  lo = (np.asarray(b, dtype=np.uint64) >> np.uint64(6)).astype(np.float64)
  return (hi * 67108864.0 + lo) / 9007199254740992.0


def uniforms(first, n, seed):
  """(u_phi, u_t) of rays first .. first + n - 1 of stream `seed`: counter (ray_lo, ray_hi, 0, 0), key (seed_lo, seed_hi)"""
  ray = np.arange(int(n), dtype=np.uint64) + np.uint64(int(first))
  w = philox4x32_10((ray & _M32, ray >> np.uint64(32), 0, 0), (int(seed) & 0xFFFFFFFF, int(seed) >> 32))
  return u53(w[0], w[1]), u53(w[2], w[3])


# ---------------------------------------------------------------- references
MAX_MP = 4096
mp200 = mpmath.mp.clone()
mp200.prec = 200


def _mp_to_long(x):
  hi = float(x)
  return L(hi) + L(float(x - hi))


def exact_inverse(cdf, edges, u):
  """the piecewise-linear inverse of the table at u: j = last knot with cdf[j] <= u, e_j + (e_j+1 - e_j)(u - c_j) /
  (c_j+1 - c_j).  -> namespace(value: longdouble -- worked out at 200 bits for the rays on or beside a knot (`near`,
  at most MAX_MP of them: `mp`) --, j, on_knot, scale = max(|e_j|, |e_j+1|))"""
  cdf, edges, u = (np.asarray(a, dtype=np.float64) for a in (cdf, edges, u))
  j = np.searchsorted(cdf, u, side='right') - 1
  assert j.min() >= 0 and j.max() < len(cdf) - 1
  cj, cn, ej, en = cdf[j], cdf[j + 1], edges[j], edges[j + 1]
  value = ej.astype(L) + (en.astype(L) - ej.astype(L)) * (u.astype(L) - cj.astype(L)) / (cn.astype(L) - cj.astype(L))
  on = cj == u
  near = on | (u == np.nextafter(cj, 2.0)) | (u == np.nextafter(cn, -1.0))
  mp = np.nonzero(near)[0][:MAX_MP]
  f = mp200.mpf
  for i in mp:
    value[i] = _mp_to_long(f(float(ej[i])) + (f(float(en[i])) - f(float(ej[i]))) * (f(float(u[i])) - f(float(cj[i]))) /
                           (f(float(cn[i])) - f(float(cj[i]))))
  return types.SimpleNamespace(value=value, j=j, on_knot=on, near=near, mp=mp, scale=np.maximum(np.abs(ej), np.abs(en)))


def exact_row(phi_edges, phi):
  """the theta row of every phi: argmin_i |mid_i - phi| over ALL cells, first minimum, mid_i in float64"""
  e = np.asarray(phi_edges, dtype=np.float64)
  mids = (e[1:] + e[:-1]) / 2
  return np.abs(mids[None, :] - np.asarray(phi, dtype=np.float64)[:, None]).argmin(axis=1)


def exact_ray(xform, focal_length, t, phi):
  """(origins, directions) [n, 3] in longdouble.  Finite focus: local direction (sin t sin phi, -sin t cos phi, cos t),
  local origin ((0, 0, 1) - direction) f; collimated: direction (0, 0, 1), origin (t cos phi, -t sin phi, 0); then
  origin -> R o + translation, direction -> R d, normalised"""
  m = np.asarray(xform, dtype=np.float64).reshape(3, 4).astype(L)
  t, phi = np.asarray(t, dtype=np.float64).astype(L), np.asarray(phi, dtype=np.float64).astype(L)
  sp, cp = np.sin(phi), np.cos(phi)
  zero, one = np.zeros_like(t), np.ones_like(t)
  if np.isfinite(focal_length):
    st, ct = np.sin(t), np.cos(t)
    d = np.stack([st * sp, -st * cp, ct], axis=1)
    o = (np.stack([zero, zero, one], axis=1) - d) * L(focal_length)
  else:
    d = np.stack([zero, zero, one], axis=1)
    o = np.stack([t * cp, -t * sp, zero], axis=1)
  go = o @ m[:, :3].T + m[:, 3]
  gd = d @ m[:, :3].T
  return go, gd / np.sqrt((gd * gd).sum(axis=1))[:, None]


def exact_ray_mp(xform, focal_length, t, phi):
  """exact_ray for one ray at 200 bits -> (origin, direction) as lists of mpf"""
  f = mp200.mpf
  m = [f(float(v)) for v in np.asarray(xform, dtype=np.float64).reshape(12)]
  t, phi = f(float(t)), f(float(phi))
  sp, cp = mp200.sin(phi), mp200.cos(phi)
  if np.isfinite(focal_length):
    st, ct = mp200.sin(t), mp200.cos(t)
    d = [st * sp, -st * cp, ct]
    o = [-d[0] * f(float(focal_length)), -d[1] * f(float(focal_length)), (1 - d[2]) * f(float(focal_length))]
  else:
    d = [f(0), f(0), f(1)]
    o = [t * cp, -t * sp, f(0)]
  go = [m[4 * r] * o[0] + m[4 * r + 1] * o[1] + m[4 * r + 2] * o[2] + m[4 * r + 3] for r in range(3)]
  gd = [m[4 * r] * d[0] + m[4 * r + 1] * d[1] + m[4 * r + 2] * d[2] for r in range(3)]
  norm = mp200.sqrt(gd[0] ** 2 + gd[1] ** 2 + gd[2] ** 2)
  return go, [v / norm for v in gd]


# ---------------------------------------------------------------- table makers
# A maker gets the uniforms of the rays on its axis (u), the number of cells of that axis' search guide (65536 for
# theta / radius, 256 for the azimuth: odw_capi.hip kGuide, kPhiGuide) and a generator -> (cdf, edges).
T_GUIDE, PHI_GUIDE = 1 << 16, 1 << 8


def _table(knots, edges=None, lo=-1.0, hi=2.0):
  cdf = np.concatenate([[0.0], np.sort(np.asarray(knots, dtype=np.float64)), [1.0]])
  assert cdf[1] >= 0.0 and cdf[-2] <= 1.0
  return cdf, (np.linspace(lo, hi, len(cdf)) if edges is None else np.asarray(edges, dtype=np.float64))


def on_below_above(values):
  """a third of the values as they are, a third moved to the double below, a third to the double above"""
  v = np.array(values, dtype=np.float64)
  v[1::3] = np.nextafter(v[1::3], -1.0)
  v[2::3] = np.nextafter(v[2::3], 2.0)
  return v[(v > 0.0) & (v < 1.0)]


def identity(u, guide, rng):
  return np.array([0.0, 1.0]), np.array([0.0, 1.0])


def two_knots(u, guide, rng):
  return np.array([0.0, 1.0]), np.array([-3.0, 7.5])


def knots_on_rays(u, which, plateau_every=50):
  """knots on, below and above the u of the rays `which`; every plateau_every-th knot twice (a cell of no density);
  edges spread over six decades"""
  k = on_below_above(u[np.asarray(which)])
  k = np.concatenate([k, k[::plateau_every]])
  return _table(k, np.geomspace(1e-3, 1e3, len(k) + 2))


def on_rays(u, guide, rng):
  return knots_on_rays(u, rng.choice(len(u), size=min(2048, len(u) // 8), replace=False))


def plateaus(u, guide, rng):
  """repeated cdf values at the start (0), in the middle (on a ray's u) and at the end (1 reached early)"""
  body = on_below_above(u[rng.choice(len(u), size=60, replace=False)])
  m = u[rng.integers(len(u))]
  k = np.concatenate([[0.0, 0.0], body, [m, m, m], [1.0, 1.0, 1.0]])
  return _table(k, lo=-2.0, hi=5.0)


def dense(u, guide, rng):
  """200001 knots: several per guide cell"""
  on = on_below_above(u[rng.choice(len(u), size=999, replace=False)])
  k = np.unique(np.concatenate([on, rng.random(199999 - len(on))]))
  k = k[(k > 0.0) & (k < 1.0)]
  assert len(k) == 199999
  return _table(k, lo=0.0, hi=np.pi / 4)


def _crammed(u, guide, rng, high):
  """all interior knots inside the guide cell next to 0 (or next to 1), some on the rays that fall into it"""
  w = 1.0 / guide
  inside = np.nonzero(u >= 1.0 - w)[0] if high else np.nonzero(u < w)[0]
  assert len(inside) >= 3, 'no rays in the crammed cell: more rays, or another seed'
  k = np.concatenate([on_below_above(u[inside[:300]]), (1.0 - w if high else 0.0) + w * rng.random(200)])
  return _table(k[(k > 0.0) & (k < 1.0)], lo=0.5, hi=3.5)


def crammed_low(u, guide, rng):
  return _crammed(u, guide, rng, False)


def crammed_high(u, guide, rng):
  return _crammed(u, guide, rng, True)


def at_guide_borders(u, guide, rng):
  """knots at k / guide and at the doubles beside it, k in {0, 1, guide / 2, guide - 1}, and on / beside the rays
  nearest to those borders"""
  k = []
  for b in (0, 1, guide // 2, guide - 1):
    x = b / guide
    k += [x, np.nextafter(x, 2.0), np.nextafter(x, -1.0)]
    k += list(on_below_above(u[np.argsort(np.abs(u - x))[:6]]))
  k = np.unique(k)
  return _table(k[(k > 0.0) & (k < 1.0)], lo=-1.0, hi=1.0)


MAKERS = dict(identity=(identity, 4096), two_knots=(two_knots, 4096), on_rays=(on_rays, 16384), plateaus=(plateaus, 16384),
              dense=(dense, 16384), crammed_low=(crammed_low, 1 << 18), crammed_high=(crammed_high, 1 << 18),
              at_guide_borders=(at_guide_borders, 16384))
SEEDS = (0x9E3779B97F4A7C15, 0xC0FFEE0012345678, 0x8000000000000001)        # (high words set)
FIRSTS = (0, (1 << 32) - 3, 1 << 40)


def _case(name, first, n, seed, t_edges, t_cdf, phi_edges, phi_cdf):
  u_phi, u_t = uniforms(first, n, seed)
  return types.SimpleNamespace(name=name, first=first, n=n, seed=seed, u_phi=u_phi, u_t=u_t, t_edges=t_edges,
                               t_cdf=np.atleast_2d(t_cdf), phi_edges=phi_edges, phi_cdf=phi_cdf)


@functools.lru_cache(maxsize=None)
def table_case(name):
  """one theta table and the azimuth table of the same maker, each on its own uniforms"""
  maker, n = MAKERS[name]
  i = sorted(MAKERS).index(name)
  first, seed = FIRSTS[i % 3], SEEDS[i % 3]
  u_phi, u_t = uniforms(first, n, seed)
  if name.startswith('crammed'):           # (the first window of n rays with a few of them in the theta guide's end cell)
    cell = (lambda u: u >= 1.0 - 1.0 / T_GUIDE) if name.endswith('high') else (lambda u: u < 1.0 / T_GUIDE)
    while cell(u_t).sum() < 3:
      first += n
      u_phi, u_t = uniforms(first, n, seed)
  rng = np.random.default_rng(1000 + i)
  t_cdf, t_edges = maker(u_t, T_GUIDE, rng)
  phi_cdf, phi_edges = maker(u_phi, PHI_GUIDE, rng)
  return _case(name, first, n, seed, t_edges, t_cdf, phi_edges, phi_cdf)


ROW_CASES = ('rows-2', 'rows-24', 'rows-100', 'rows-24-narrow')


@functools.lru_cache(maxsize=None)
def rows_case(name):
  """one theta table per azimuth cell: equidistant azimuth edges, t_edges = [0, 1, 2], row r has cdf [0, (r + 1) /
  (rows + 1), 1]: the value names the row.  The azimuth knots sit on rays' u_phi, so those rays' phi IS an interior
  edge: the tie between two rows.  'narrow': cells of 4096 ulp beside 1.0, where the rays of the smallest and the
  largest u_phi round to the first and to the last edge."""
  rows = int(name.split('-')[1])
  narrow = name.endswith('narrow')
  first, n, seed = (1 << 32) - 3, 1 << 16, SEEDS[1]
  u_phi, u_t = uniforms(first, n, seed)
  rng = np.random.default_rng(rows + narrow)
  pool = np.nonzero((u_phi > 0.25) & (u_phi < 0.75))[0] if narrow else np.arange(n)     # (narrow: wide end cells, slopes of < 4 w)
  knots = np.sort(u_phi[rng.choice(pool, size=rows - 1, replace=False)])
  if narrow:
    phi_edges = np.linspace(1.0, 1.0 + rows * 2.0 ** -40, rows + 1)
  else:
    phi_edges = np.linspace(0.0, 2 * np.pi, rows + 1)
  phi_cdf = np.concatenate([[0.0], knots, [1.0]])
  t_cdf = np.array([[0.0, (r + 1) / (rows + 1), 1.0] for r in range(rows)])
  return _case(name, first, n, seed, np.array([0.0, 1.0, 2.0]), t_cdf, phi_edges, phi_cdf)


def row_of_value(case, t):
  """the row each t names: the one row whose table gives this t at the ray's u_t (-1: none, -2: several)"""
  cand = np.stack([np.interp(case.u_t, c, case.t_edges) for c in case.t_cdf], axis=1)
  hit = cand == np.asarray(t)[:, None]
  return np.where(hit.sum(axis=1) == 1, hit.argmax(axis=1), np.where(hit.any(axis=1), -2, -1))


def host_draw(case):
  """(t, phi) by the documented contract: numpy.interp on the table, the row by exact_row"""
  phi = np.interp(case.u_phi, case.phi_cdf, case.phi_edges)
  if len(case.t_cdf) == 1:
    return np.interp(case.u_t, case.t_cdf[0], case.t_edges), phi
  row = exact_row(case.phi_edges, phi)
  t = np.empty_like(phi)
  for r in np.unique(row):
    t[row == r] = np.interp(case.u_t[row == r], case.t_cdf[r], case.t_edges)
  return t, phi


def source_of(case, xform=IDENTITY, focal_length=1.0):
  from freecad.optics_design_workbench_amd.distributions.random_number_generator import SamplerTables
  from freecad.optics_design_workbench_amd.freecad_elements.point_source import BakedSource
  return BakedSource(xform=np.asarray(xform, dtype=np.float64).reshape(12), focal_length=float(focal_length), wavelength=500.0,
                     power=1.0, tables=SamplerTables(case.t_edges, case.t_cdf, case.phi_edges, case.phi_cdf), name=case.name)


@functools.lru_cache(maxsize=None)
def geometric_case(rows):
  """azimuth edges [0, geomspace(0.01, 2 pi, 11)]: what the three-candidate window cannot serve.  rows: one theta table
  per cell (refused by the upload) or one for all (accepted: no row is looked for)"""
  first, n, seed = 7, 16384, SEEDS[0]
  u_phi, u_t = uniforms(first, n, seed)
  phi_edges = np.concatenate([[0.0], np.geomspace(0.01, 2 * np.pi, 11)])
  phi_cdf = np.concatenate([[0.0], on_below_above(np.sort(u_phi[:10])), [1.0]])
  cells = len(phi_edges) - 1
  t_cdf = np.array([[0.0, (r + 1) / (cells + 1), 1.0] for r in range(cells)]) if rows else np.array([[0.0, u_t[5], 1.0]])
  return _case('geometric', first, n, seed, np.array([0.0, 1.0, 2.0]), t_cdf, phi_edges, phi_cdf)


def check_inversion(case, t, phi, rows=None):
  """truth: within 8 * 2^-53 * max(|e_j|, |e_j+1|) of the exact inverse (three roundings in slope * (u - c_j), each
  2^-53 relative to at most 2 max|e|, and the final addition: 7), a ray on a knot gets the knot's edge itself"""
  for name, got, cdf, edges, u in (('phi', phi, case.phi_cdf, case.phi_edges, case.u_phi),) + tuple(
      ('t', t[rows == r], case.t_cdf[r], case.t_edges, case.u_t[rows == r]) for r in (np.unique(rows) if rows is not None else ())):
    ex = exact_inverse(cdf, edges, u)
    err = np.abs(np.asarray(got).astype(L) - ex.value).astype(np.float64)
    worst = (err / (EPS * np.maximum(ex.scale, 5e-324))).max()
    print(f'{case.name} {name}: {worst:.3f} x 2^-53 max|e|, {int(ex.on_knot.sum())} rays on a knot, {int(ex.near.sum())} on or beside one')
    assert np.all(err <= 8 * EPS * ex.scale), (case.name, name, worst)
    assert np.array_equal(np.asarray(got)[ex.on_knot], np.asarray(edges)[ex.j[ex.on_knot]])
  return True


# ---------------------------------------------------------------- ray cases
PI = np.pi
THETAS = (0.0, PI / 2, -PI / 2, PI, 5e-324, 1e-300, 1e-9, 64.0, -64.0, 63.9, -37.7)
PHIS = (0.0, PI / 2, PI, 3 * PI / 2, 2 * PI, 64.0, -64.0, 1.0)
RADII = (0.0, 5e-324, 1e-300, 1e-9, 1.0, 999.5, 1e3)
RAY_N = 1024


def _on_rays_with_values(u, values):
  """a table that gives ray i (i < len(values)) exactly values[i]: its knots are those rays' u, its edges their values
  (not sorted: numpy.interp and the kernels ask that of the cdf only); the rays between interpolate from one value
  to the next, all over the domain"""
  order = np.argsort(u[:len(values)])
  cdf = np.concatenate([[0.0], u[:len(values)][order], [1.0]])
  v = np.asarray(values, dtype=np.float64)[order]
  return cdf, np.concatenate([[v[0]], v, [v[-1]]])


@functools.lru_cache(maxsize=None)
def ray_case(finite):
  """every pair of THETAS (or RADII) x PHIS on a ray of its own, bit for bit"""
  first, n, seed = 5, RAY_N, SEEDS[2]
  u_phi, u_t = uniforms(first, n, seed)
  pairs = [(a, b) for a in (THETAS if finite else RADII) for b in PHIS]
  t_cdf, t_edges = _on_rays_with_values(u_t, [p[0] for p in pairs])
  phi_cdf, phi_edges = _on_rays_with_values(u_phi, [p[1] for p in pairs])
  c = _case('rays-finite' if finite else 'rays-collimated', first, n, seed, t_edges, t_cdf, phi_edges, phi_cdf)
  c.pairs = pairs
  return c


def rotation(axis, angle):
  a = np.asarray(axis, dtype=np.float64)
  a = a / np.linalg.norm(a)
  k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
  return np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)


def frame(r, t=(0.0, 0.0, 0.0)):
  return np.hstack([np.asarray(r, dtype=np.float64), np.asarray(t, dtype=np.float64).reshape(3, 1)]).reshape(12)


FRAMES = {
    'identity': IDENTITY,
    'quarter-z': frame([[0, -1, 0], [1, 0, 0], [0, 0, 1]], (0.25, 0.0, -1.5)),        # (entries 0, +1, -1: what the compiled path folds)
    'quarter-x': frame([[1, 0, 0], [0, 0, -1], [0, 1, 0]]),
    'half-x': frame(np.diag([1.0, -1.0, -1.0]), (0.0, 2.0, 0.0)),
    'general': frame(rotation((1.0, 2.0, 3.0), 0.7), (0.3, -0.2, 0.1)),
    'far': frame(rotation((2.0, -1.0, 0.5), 0.03), (1e5, -3e4, 7e4)),
    # (a rotation times 3: the one frame whose directions reach the second normalisation of make_ray away from length 1)
    'scaled': frame(3.0 * rotation((-1.0, 0.5, 2.0), 1.1), (0.5, 0.5, -0.5)),
}
FOCALS = (1.0, -1.0, 1e-3, 1e4, float('inf'))
RAY_SOURCES = [(fr, f) for fr in FRAMES for f in FOCALS]


def ray_scales(focal_length, t, origins):
  """what the error bounds of a ray are measured in: directions 1 + |origin|_inf (the direction is the difference of
  two points beside the origin), origins |origin|_inf + |f| (collimated: + the ray's radius)"""
  o = np.abs(np.asarray(origins, dtype=np.float64)).max(axis=1)
  return 1.0 + o, o + (abs(focal_length) if np.isfinite(focal_length) else np.abs(np.asarray(t, dtype=np.float64)))


def ray_ratios(focal_length, t, origins, dirs, exact_o, exact_d):
  """(direction, origin) error of every ray in units of 2^-53 times its scale"""
  sd, so = ray_scales(focal_length, t, np.asarray(exact_o, dtype=np.float64))
  ed = np.abs(np.asarray(dirs, dtype=np.float64).astype(L) - exact_d).max(axis=1).astype(np.float64)
  eo = np.abs(np.asarray(origins, dtype=np.float64).astype(L) - exact_o).max(axis=1).astype(np.float64)
  with np.errstate(invalid='ignore', divide='ignore'):
    return np.where(ed == 0, 0.0, ed / (EPS * sd)), np.where(eo == 0, 0.0, eo / (EPS * so))


# C_HOST: the largest error of the float64 host makeRay (freecad_elements/point_source.py) against exact_ray over
# RAY_SOURCES x the ray cases, in those units (measured: test_source_cases.py prints and bounds it).  The device may
# take four times that -- its reciprocal square roots are good to two ulp where the host's division and square root
# are correctly rounded, its sine and cosine to one ulp of 1.0 where libm's are below one ulp of the value.
C_HOST = 3.0       # (measured 2.78 on directions, 2.20 on origins)
C = 4 * C_HOST
