"""The varied-power scene of the power-map tests (tests/test_power_maps.py, tests/test_gpu_power_maps.py): a pair of
70 % mirrors that rays bounce between (powers 0.7^k) and an absorbing lens beside them (AbsorptionLength 3 mm: a
continuum of powers), all groups recording, explicit rays -- built the way tests/test_gpu_parity_geometry.py builds
its scenes.  No golden scene moves the power (Reflectivity 1, AbsorptionLength inf or 0 everywhere)."""
import numpy as np

from freecad.optics_design_workbench_amd.freecad_elements import make
from freecad.optics_design_workbench_amd.scene import Document, bake

QUANTUM = 2.0 ** 32          # ODW_POWER_QUANTUM_BITS = 32 (include/odw_trace.h)


def build(groups, settings=None):
  doc = Document()
  for kind, elems, props in groups:
    make.makeOpticalGroup(doc, kind, elems(doc), **props)
  make.makeSimulationSettings(doc, **(settings or {}))
  src = make.makePointSource(doc)
  sc = bake.bakeScene(doc, src)
  sc.group_record = np.ones_like(sc.group_record)
  return sc, bake.bakeLimits(doc, src)


def scene():
  """-> (scene, limits)"""
  return build([
      ('Mirror', lambda d: [make.makeBox(d, 'A', 50, 50, 1, base=(-25, -25, 10)),
                            make.makeBox(d, 'B', 50, 50, 1, base=(-25, -25, -11))], dict(Reflectivity=0.7)),
      ('Lens', lambda d: [make.makeBox(d, 'Abs', 20, 20, 6, base=(30, -10, -3))],
       dict(RefractiveIndex=1.4, AbsorptionLength='3.0')),
      ('Absorber', lambda d: [make.makeSphere(d, 'Shell', 150)], {}),
  ], settings=dict(MaxIntersections=13.0))


def rays(n, seed=7, first=0):
  """origins near the scene's centre, a third aimed at each mirror and at the lens.  Ray i depends on (seed, first + i)
  only through the position in one stream: rays(n)[a:b] are the rays of a shard"""
  rs = np.random.RandomState(seed)
  o = rs.normal(0, 1, (first + n, 3))
  o = o / np.linalg.norm(o, axis=1)[:, None] * 3.0
  targets = np.array([[0, 0, 10.0], [0, 0, -10.0], [33.0, 0, 0]])
  t = targets[rs.randint(0, 3, first + n)] + rs.normal(0, 6.0, (first + n, 3))
  d = t - o
  d = d / np.linalg.norm(d, axis=1)[:, None]
  return np.ascontiguousarray(o[first:]), np.ascontiguousarray(d[first:])


# the window leaves part of the mirrors (|x|, |y| up to 25) outside: the overflow counter is exercised
DETECTOR = dict(group=-1, origin=(0.25, -0.5, 0.0), ex=(1.0, 0.0, 0.0), ey=(0.0, 1.0, 0.0),
                x_lo=-20.0, x_hi=20.0, y_lo=-20.0, y_hi=20.0, nx=64, ny=48)


def quanta(power):
  """the weight of a hit (include/odw_trace.h): rint(clamp(power, 0, 2^20) * 2^32), NaN -> 0, as uint64"""
  p = np.asarray(power, dtype=np.float64)
  p = np.where(p > 0, np.minimum(p, 2.0 ** 20), 0.0)
  return np.rint(p * QUANTUM).astype(np.uint64)


def detector_bins(points, det=DETECTOR):
  """odw_detector_desc's rule (include/odw_trace.h): x = (p - origin) . ex, ix = floor((x - x_lo) * nx / (x_hi - x_lo)),
  the same for y -> (ix, iy, inside); products summed left to right, as the kernels do (the axes here are coordinate
  axes: the sums are exact either way)"""
  r = np.asarray(points, dtype=np.float64) - np.asarray(det['origin'], dtype=np.float64)
  ex, ey = det['ex'], det['ey']
  x = r[:, 0] * ex[0] + r[:, 1] * ex[1] + r[:, 2] * ex[2]
  y = r[:, 0] * ey[0] + r[:, 1] * ey[1] + r[:, 2] * ey[2]
  fx = np.floor((x - det['x_lo']) * (det['nx'] / (det['x_hi'] - det['x_lo'])))
  fy = np.floor((y - det['y_lo']) * (det['ny'] / (det['y_hi'] - det['y_lo'])))
  inside = (fx >= 0) & (fx < det['nx']) & (fy >= 0) & (fy < det['ny'])
  return fx.astype(np.int64), fy.astype(np.int64), inside


def planes(rows, det=DETECTOR):
  """(count plane, power plane in quanta, hits outside the window) of hit rows, with numpy"""
  ix, iy, inside = detector_bins(rows['point'], det)
  counts = np.zeros((det['nx'], det['ny']), dtype=np.uint64)
  power = np.zeros((det['nx'], det['ny']), dtype=np.uint64)
  np.add.at(counts, (ix[inside], iy[inside]), np.uint64(1))
  np.add.at(power, (ix[inside], iy[inside]), quanta(rows['power'][inside]))
  return counts, power, int((~inside).sum())
