"""Hit clouds for the median tests (tests/test_median_cases.py, tests/test_gpu_medians.py), and the reference they are
held against: `numpy.median` of the projected coordinates -- nothing of the library's.

Synthetic clouds use the axis-aligned arrangement of test_polar_binning_decides_every_row_like_numpy: rows
P = (X, -Y, 0), planeNormal (0, 0, -1), xInPlaneVec (1, 0, 0), so that the device projects exactly (X, Y) (up to the
sign of a zero: the projection's last addend is +0.0).  `cases()` yields named clouds with what each coordinate claims
to be (`Coord.claims`); tests/test_median_cases.py holds every claim with numpy alone, so that a GPU test cannot pass
because a case silently stopped being the case.

The focus family: a point source that converges on (0, 0, 25) and an absorber box whose front face lies at
z = 25 + dz, built in code -- at dz = 0 every hit lies within rounding of one point and thousands of rows tie on
the median value (more than the batched chain ranks: `K_PHB_CAND`)."""
import collections

import numpy as np

K_PHB_CAND = 2048            # kPhbCand (csrc/odw_posthoc_batch.hip): median candidates the batched chain ranks
K_PH_SEL_MAX = 1 << 21       # kPhSelMax (csrc/odw_posthoc.hip): candidates the per-segment chain collects; more: the sort
TINY = 5e-324                # the smallest subnormal

PLANE_NORMAL = np.array([0.0, 0.0, -1.0])
X_IN_PLANE = np.array([1.0, 0.0, 0.0])


# ---- the reference --------------------------------------------------------------------------------------------------
def axes(planeNormal, xInPlaneVec):
  """in-plane unit axes as DeviceHits.histogram and DeviceHitsBatch._axes form them"""
  x = np.asarray(xInPlaneVec, dtype=np.float64)
  y = np.cross(planeNormal, xInPlaneVec)
  return x / np.linalg.norm(x), y / np.linalg.norm(y)


def dot3(P, e):
  """the device's projection: three products summed left to right, no contraction (not `P @ e`)"""
  return P[:, 0] * e[0] + P[:, 1] * e[1] + P[:, 2] * e[2]


def project(P, planeNormal, xInPlaneVec):
  ex, ey = axes(planeNormal, xInPlaneVec)
  return dot3(P, ex), dot3(P, ey)


def medians(x, y):
  with np.errstate(over='ignore'):
    return np.array([np.median(x), np.median(y)])


def middle(v):
  """the two middle elements numpy.median averages"""
  s = np.sort(v)
  return s[(len(s) - 1) // 2], s[len(s) // 2]


def tiesAtMiddle(v):
  """rows tied on the value at rank (m - 1) // 2"""
  return int(np.count_nonzero(v == middle(v)[0]))


def edgesAbout(x, y):
  """finite cartesian edges for (x - median, y - median): one edge exactly on the median (0.0: rows piled up on the
  median sit on an edge), the outermost ones bracket both clouds"""
  ox, oy = medians(x, y)
  dev = np.abs(np.r_[x - ox, y - oy])
  h = float(dev.max())
  if not (h > 0):
    h = 1.0
  q = float(np.median(dev))
  marks = {0.0, h, -h, h / 2, -h / 2}
  for f in (0.5, 1.0, 2.0):
    if 0 < q * f < h:
      marks |= {q * f, -q * f}
  return np.array(sorted(marks))


def histogram2d(x, y, origin, edges):
  with np.errstate(over='ignore', invalid='ignore'):       # (numpy takes differences of the edges: inf for +-1.7e308)
    return np.histogram2d(x - origin[0], y - origin[1], bins=[edges, edges])[0]


# ---- synthetic clouds -----------------------------------------------------------------------------------------------
Coord = collections.namedtuple('Coord', 'values claims')
Case = collections.namedtuple('Case', 'name X Y claimsX claimsY')

COUNTS = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 511, 512, 513, 4097)
BIG = (1 << 21) + 7


def rows(X, Y):
  """hit dictionary of the rows (X, -Y, 0) for Tracer.loadHits"""
  P = np.c_[X, -np.asarray(Y), np.zeros(len(X))]
  return dict(points=P, directions=np.tile([0.0, 0.0, 1.0], (len(X), 1)), powers=np.ones(len(X)),
              isEntering=np.ones(len(X), dtype=int))


def _normal(m, seed):
  v = np.random.default_rng(seed).normal(size=m)
  return Coord(v, dict(m=m, ties=1))


def _equal(m, value):
  return Coord(np.full(m, value), dict(m=m, ties=m, width=0.0))


def _two(n_lo, n_hi, seed, lo=-1.5, hi=2.5):
  """n_lo rows on one value, n_hi on another.  Half and half with an even count: the two middle elements differ, and
  they are the minimum and the maximum -- coarse bins 0 and 4095"""
  v = np.r_[np.full(n_lo, lo), np.full(n_hi, hi)]
  np.random.default_rng(seed).shuffle(v)
  mid = (lo, hi) if n_lo == n_hi else (lo, lo) if n_lo > n_hi else (hi, hi)
  return Coord(v, dict(m=n_lo + n_hi, ties=n_lo if n_lo >= n_hi else n_hi, middle=mid))


def _pile(copies, spread, seed):
  rng = np.random.default_rng(seed)
  v = np.r_[np.full(copies, 0.25), rng.uniform(-1, 1, spread)]
  rng.shuffle(v)
  return Coord(v, dict(m=copies + spread, ties=copies))


def _digits(m, seed):
  v = np.random.default_rng(seed).integers(0, 10, m).astype(np.float64)
  return Coord(v, dict(m=m, ties_above=m // 12, ties_below=m // 8))


def _outliers(seed):
  rng = np.random.default_rng(seed)
  v = np.r_[rng.uniform(0, 1e-9, 10_001), 1e300, -1e300]
  rng.shuffle(v)
  return Coord(v, dict(m=10_003, ties=1, width=2e300))


def _huge(seed):
  rng = np.random.default_rng(seed)
  v = np.r_[rng.normal(size=1001), [1.7e308] * 3, [-1.7e308] * 2]
  rng.shuffle(v)
  return Coord(v, dict(m=1006, ties=1, width=np.inf))


def _subnormal(m, seed):
  """k * 5e-324, k = 0 .. 7, over and over: the width is subnormal, 4096 / width overflows, width / 4096 underflows"""
  v = np.tile(np.arange(8) * TINY, (m + 7) // 8)[:m]
  np.random.default_rng(seed).shuffle(v)
  claims = dict(m=m, width='subnormal')
  if m % 8 == 0:
    claims.update(ties=m // 8, middle=(3 * TINY, 4 * TINY))
  return Coord(v, claims)


def _cauchy(m, seed):
  return Coord(np.random.default_rng(seed).standard_cauchy(m), dict(m=m, ties=1))


def _lognormal(m, seed):
  return Coord(np.random.default_rng(seed).lognormal(size=m), dict(m=m, ties=1))


def _zeros(seed):
  rng = np.random.default_rng(seed)
  v = np.r_[-rng.uniform(0.1, 1, 20), [-0.0] * 30, [0.0] * 31, rng.uniform(0.1, 1, 20)]
  rng.shuffle(v)
  return Coord(v, dict(m=101, ties=61, middle=(0.0, 0.0), signed_zeros=True))


def _sortRoute():
  v = np.full(BIG, 0.75)
  v[12345], v[BIG - 77] = -3.0, 8.0
  # (2^21 + 5 rows on one value: whatever the bins, those of the middle ranks hold more than kPhSelMax rows)
  return Coord(v, dict(m=BIG, ties=BIG - 2, ties_above=K_PH_SEL_MAX))


def _builders():
  """name -> function that builds (coordinate on X, coordinate on Y): different cases on the two coordinates of one
  cloud halve the launches"""
  out = collections.OrderedDict()
  fill = {5: lambda: _equal(5, 0.3), 4097: lambda: _equal(4097, -7.0),
          256: lambda: _two(128, 128, 21), 257: lambda: _two(129, 128, 22), 512: lambda: _two(257, 255, 23),
          64: lambda: _two(31, 33, 24), 2: lambda: _two(1, 1, 25), 3: lambda: _two(1, 2, 26)}
  for k, m in enumerate(COUNTS):
    out[f'normal-{m}'] = (lambda m=m, k=k: (_normal(m, 100 + k), fill[m]() if m in fill else _normal(m, 200 + k)))
  out['pile-3000+digits-3000'] = lambda: (_pile(2990, 10, 31), _digits(3000, 32))
  out['digits-100000+lognormal'] = lambda: (_digits(100_000, 33), _lognormal(100_000, 34))
  out['outliers+normal-10003'] = lambda: (_outliers(35), _normal(10_003, 36))
  out['huge+huge'] = lambda: (_huge(37), _huge(38))
  out['subnormal-1000+subnormal-1000'] = lambda: (_subnormal(1000, 39), _subnormal(1000, 40))
  out['subnormal-999+normal-999'] = lambda: (_subnormal(999, 49), _normal(999, 50))
  out['cauchy+cauchy'] = lambda: (_cauchy(100_003, 41), _cauchy(100_003, 42))
  out['zeros+normal-101'] = lambda: (_zeros(43), _normal(101, 44))
  # the one large case, and a tiny one behind it: what the large one left in the library's buffers must not show
  out['sort-route+normal-big'] = lambda: (_sortRoute(), _normal(BIG, 45))
  out['after-big-1'] = lambda: (_normal(1, 46), _equal(1, 2.0))
  out['after-big-4'] = lambda: (_two(2, 2, 47), _normal(4, 48))
  return out


_BUILDERS = _builders()
NAMES = list(_BUILDERS)
_CACHE = {}


def case(name):
  """the named cloud (built once; the large one is 2 x 16 MB of coordinates)"""
  if name not in _CACHE:
    cx, cy = _BUILDERS[name]()
    assert len(cx.values) == len(cy.values)
    for c in (cx, cy):
      c.values.setflags(write=False)
    _CACHE[name] = Case(name, cx.values, cy.values, cx.claims, cy.claims)
  return _CACHE[name]


def cases():
  for name in NAMES:
    yield case(name)


# ---- the focus family -----------------------------------------------------------------------------------------------
FOCUS_RAYS, FOCUS_SEED = 200_000, 5
FOCUS_DZ = (0.0, 1e-9, -1e-9, 1e-3, -1e-3)          # the first is the pile
HALF_DISC_DZ = (1e-3, -1e-3, 1e-9)                   # the source variant (PhiDomain 0 .. pi): its median is not the centre


def focusDocument(halfDisc=False):
  from freecad.optics_design_workbench_amd.freecad_elements import make
  from freecad.optics_design_workbench_amd.scene import Document
  doc = Document()
  make.makeAbsorber(doc, [make.makeBox(doc, 'Screen', 20, 20, 5, base=(-10, -10, 25))])
  make.makeSimulationSettings(doc, DistanceTolerance='1e-6')
  props = dict(FocalLength='25', ThetaDomain='0, pi/8', PowerDensity='1')
  if halfDisc:
    props['PhiDomain'] = '0, pi'
  make.makePointSource(doc, **props)
  return doc


def setDz(doc, dz):
  from freecad.optics_design_workbench_amd.scene.placement import Placement
  doc.Screen.Placement = Placement(base=(-10.0, -10.0, 25.0 + float(dz)))


def focusProjects(halfDisc=False, dzs=None):
  """one baked project per dz: the scenes differ in their numbers only"""
  from freecad.optics_design_workbench_amd import scenes
  doc = focusDocument(halfDisc)
  out = []
  for dz in (dzs if dzs is not None else (HALF_DISC_DZ if halfDisc else FOCUS_DZ)):
    setDz(doc, dz)
    out.append(scenes.bakeProject(doc))
  return out
