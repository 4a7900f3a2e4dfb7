#!/usr/bin/env python3
"""Band maps up front against band maps post hoc (profiles/spectral_posthoc.md), on the bench of
scripts/bench_spectral_bands.py -- singlet + prism under a three-line point source, a 400 mm absorbing shell, K = 8 bands
(9 edges) --, 1e7 rays, compile = 'structure':
  a  the launch that fills 256 x 256 band planes up front (setDetector(det, bands=), maps only)
  b  the launch that records its rows, then deviceHits(shell).histogram(bands=EDGES, bins=[257 edges, 257 edges]): selection,
     plane search, projection + medians and the band bin apiece (256 x 256 bins, 9 planes: atomics in HBM)
  c  route b with 30 x 30 bins (9 planes of 900 bins: the LDS window), and the same forced to HBM (ODW_BIN_BANDS_HBM=1)
  d  the plain post-hoc bin of the same rows without bands (odw_hits_bin), 256 x 256 and 30 x 30
one process, interleaved, each case twice; device work is timed with HIP events on the tracer's stream (the calls wait for
their own work, so an event pair around a call brackets it), the host's plane search with the wall clock.
  bench_spectral_posthoc.py [rays per launch]"""
import ctypes as C
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from freecad.optics_design_workbench_amd import _native
from freecad.optics_design_workbench_amd.freecad_elements import make, point_source
from freecad.optics_design_workbench_amd.scene import Document, bake
from freecad.optics_design_workbench_amd.scene.placement import Placement
from freecad.optics_design_workbench_amd.simulation.tracer import Tracer

# (the bench of scripts/bench_spectral_bands.py, which runs when imported: its scene and constants, word for word)
SEED = 0x0D15EA5E
LINES = [(make.LINE_F, 1.0), (make.LINE_d, 2.0), (make.LINE_C, 1.0)]
EDGES = np.linspace(440.0, 700.0, 9)                # K = 8; F, d, C in bands 1, 4, 6
DET = dict(group=2, origin=(0.0, 0.0, 0.0), ex=(1.0, 0.0, 0.0), ey=(0.0, 1.0, 0.0), x_lo=-400.0, x_hi=400.0, y_lo=-400.0,
           y_hi=400.0, nx=256, ny=256)


def bench():
  """the singlet on the source's axis, the prism behind it (apex edge along y, face z = 30 towards the lens), a detector"""
  doc = Document()
  h = np.sin(np.radians(-60.0)), np.cos(np.radians(-60.0))       # quaternion of the turn by -120 degrees about y
  make.makeLens(doc, [make.makeCommon(doc, [make.makeSphere(doc, 'S1', 50.0, base=(0, 0, 50.0)),
                                            make.makeSphere(doc, 'S2', 50.0, base=(0, 0, -44.0))], name='Singlet')],
                name='Singlet_', RefractiveIndex=1.5168, **make.N_BK7)
  make.makeLens(doc, [make.makeCommon(doc, [make.makeBox(doc, 'PA', 60.0, 40.0, 60.0, base=(-40.0, -20.0, 30.0)),
                                            make.makeBox(doc, 'PB', 60.0, 40.0, 60.0, base=(20.0, -20.0, 30.0), quat=(0.0, h[0], 0.0, h[1]))],
                                      name='Prism')],
                name='Prism_', RefractiveIndex=1.62, Dispersion='Cauchy', DispersionCoefficients=[1.5950, 0.0105, 0.0002])
  make.makeAbsorber(doc, [make.makeSphere(doc, 'Shell', 400.0)], name='Detector_')
  make.makeSimulationSettings(doc, DistanceTolerance='1e-6')
  src = make.makePointSource(doc, placement=Placement(base=(0.0, 0.0, -50.0)), Wavelength=make.LINE_d, Spectrum=LINES)
  return bake.bakeScene(doc, src), bake.bakeLimits(doc, src), point_source.bakeSource(doc, src)


n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10_000_000
GROUP = DET['group']
hip = C.CDLL('libamdhip64.so')
hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
hip.hipEventSynchronize.argtypes = [C.c_void_p]
hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]


class Events:
  """ms of device time between entering and leaving the block, on the tracer's stream"""

  def __init__(self, tr):
    self.stream = C.c_void_p(tr.stream())
    self.a, self.b = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(self.a)) == 0 and hip.hipEventCreate(C.byref(self.b)) == 0

  def __enter__(self):
    assert hip.hipEventRecord(self.a, self.stream) == 0
    return self

  def __exit__(self, *exc):
    assert hip.hipEventRecord(self.b, self.stream) == 0 and hip.hipEventSynchronize(self.b) == 0
    ms = C.c_float(0)
    assert hip.hipEventElapsedTime(C.byref(ms), self.a, self.b) == 0
    self.ms = float(ms.value)


def upfront(tr, ev):
  tr.setDetector(DET, bands=EDGES)
  tr.reserveHits(0)
  tr.reset()
  with ev:
    tr.trace(0, n, SEED, record_hits=False, histogram=True)
  planes = tr.bandHistogram()
  assert np.array_equal(planes.sum(0), tr.histogram())
  return dict(launch_ms=ev.ms), planes


def posthoc(tr, ev, nbins, bands=True, force_hbm=False):
  """-> (ms per step, the planes)"""
  out = {}
  tr.setDetector(None)
  tr.reserveHits(2 * n + 1024)
  tr.reset()
  with ev:
    tr.trace(0, n, SEED, record_hits=True, histogram=False)
  out['launch_ms'] = ev.ms
  assert tr.counters()['hits_dropped'] == 0
  with ev:
    dh = tr.deviceHits(GROUP)
  out['select_ms'] = ev.ms
  t0 = time.perf_counter()
  normal, x_vec = dh.detectPlaneNormal()
  out['plane_search_wall_ms'] = (time.perf_counter() - t0) * 1e3
  ex = np.asarray(x_vec, dtype=np.float64)
  ey = np.cross(normal, x_vec)
  ex, ey = ex / np.linalg.norm(ex), ey / np.linalg.norm(ey)
  pd = C.POINTER(C.c_double)
  stats = np.zeros(8)
  with ev:
    tr._chk(tr._lib.odw_hits_project(tr._ctx, C.c_int32(0), ex.ctypes.data_as(pd), ey.ctypes.data_as(pd), stats.ctypes.data_as(pd)),
            'odw_hits_project')
  out['project_medians_ms'] = ev.ms
  origin = np.array([np.mean(stats[0:2]), np.mean(stats[4:6])])
  edges = [np.linspace(-400.0, 400.0, nbins + 1)] * 2
  if force_hbm:
    os.environ['ODW_BIN_BANDS_HBM'] = '1'
  try:
    if bands:
      with ev:
        got = dh._bandHistograms(EDGES, (_native.ROW_WL_SPECTRUM, SEED, 0, None), False, False, origin, edges, normal, x_vec)
      planes = np.array([h.hist for h in got.bands])
      assert got.noBand == 0 and np.array_equal(planes.sum(0), got.total.hist)
    else:
      counts = np.zeros(nbins * nbins, dtype=np.uint64)
      with ev:
        tr._chk(tr._lib.odw_hits_bin(tr._ctx, C.c_int32(0), origin.ctypes.data_as(pd), edges[0].ctypes.data_as(pd),
                                     C.c_int32(nbins + 1), edges[1].ctypes.data_as(pd), C.c_int32(nbins + 1),
                                     counts.ctypes.data_as(C.POINTER(C.c_uint64))), 'odw_hits_bin')
      planes = counts.reshape(nbins, nbins).astype(np.float64)
  finally:
    os.environ.pop('ODW_BIN_BANDS_HBM', None)
  out['bin_ms'] = ev.ms
  out['rows'] = len(dh)
  out['posthoc_chain_ms'] = out['select_ms'] + out['plane_search_wall_ms'] + out['project_medians_ms'] + out['bin_ms']
  out['total_ms'] = out['launch_ms'] + out['posthoc_chain_ms']
  return out, planes


sc, lim, src = bench()
cases = {'a_upfront_256': lambda tr, ev: upfront(tr, ev),
         'b_posthoc_bands_256': lambda tr, ev: posthoc(tr, ev, 256),
         'c_posthoc_bands_30_lds': lambda tr, ev: posthoc(tr, ev, 30),
         'c_posthoc_bands_30_hbm': lambda tr, ev: posthoc(tr, ev, 30, force_hbm=True),
         'd_posthoc_plain_256': lambda tr, ev: posthoc(tr, ev, 256, bands=False),
         'd_posthoc_plain_30': lambda tr, ev: posthoc(tr, ev, 30, bands=False)}
runs = {k: [] for k in cases}
planes = {}
with Tracer(0) as tr:
  tr.compileScene('structure')
  tr.setScene(sc); tr.setSource(src); tr.setLimits(lim)
  ev = Events(tr)
  for name in ('a_upfront_256', 'b_posthoc_bands_256'):       # warm-up: the kernels are bound, the buffers exist
    cases[name](tr, ev)
  for rep in range(2):
    for name, run in cases.items():
      ms, planes[name] = run(tr, ev)
      runs[name].append({k: round(v, 4) for k, v in ms.items()})
  info = tr.compiledInfo()
  assert info['chroma'] == 1 and info['bands'] == 1, info
# the two LDS / HBM routes give the same planes, and the band planes add up to the plain ones
assert np.array_equal(planes['c_posthoc_bands_30_lds'], planes['c_posthoc_bands_30_hbm'])
assert np.array_equal(planes['b_posthoc_bands_256'].sum(0), planes['d_posthoc_plain_256'])
assert np.array_equal(planes['c_posthoc_bands_30_lds'].sum(0), planes['d_posthoc_plain_30'])
best = {}
for name, reps in runs.items():
  key = 'launch_ms' if name.startswith('a_') else 'total_ms'
  best[name] = min(reps, key=lambda r: r[key])
a, b, d = best['a_upfront_256']['launch_ms'], best['b_posthoc_bands_256'], best['d_posthoc_plain_256']
print(json.dumps(dict(rays_per_launch=n, bands=len(EDGES) - 1, runs=runs, best=best,
                      b_over_a=round(b['total_ms'] / a, 4), b_over_d=round(b['total_ms'] / d['total_ms'], 4),
                      band_bin_over_plain_bin_256=round(b['bin_ms'] / d['bin_ms'], 4),
                      band_bin_over_plain_bin_30=round(best['c_posthoc_bands_30_lds']['bin_ms'] / best['d_posthoc_plain_30']['bin_ms'], 4))))
