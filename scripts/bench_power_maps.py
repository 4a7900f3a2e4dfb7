#!/usr/bin/env python3
"""What the detector's power plane costs (profiles/power_maps.md): bench.py's C3 workload -- lensesAndMirrors, 1e8 rays
per launch, hit rows + 1024 x 1024 histogram, compiled kernel -- count-only and with the power plane on, same build,
same process (one u64 atomic in HBM per weighted hit on a focused beam, no LDS window); then the post-hoc binning of
5e7 rows in HBM, `DeviceHits.histogram()` against `histogram(weights='powers')`, once each after one warm-up.
  bench_power_maps.py [rays per launch] [steps] [rows of the post-hoc part]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from freecad.optics_design_workbench_amd import scenes
from freecad.optics_design_workbench_amd.simulation.tracer import Tracer
n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
rows = int(float(sys.argv[3])) if len(sys.argv) > 3 else 50_000_000
SEED = 0x0D15EA5E
pr = scenes.bakeProject(os.path.join(ROOT, 'tests', 'golden', 'scenes', 'lensesAndMirrors.FCStd'))
det = scenes.planeDetector(pr.scene, 'OpticalAbsorberGroup', nx=1024, ny=1024, toward=pr.source.xform[[3, 7, 11]])
out = {}
with Tracer(0) as tr:
  tr.setScene(pr.scene); tr.setSource(pr.source); tr.setLimits(pr.limits)
  tr.compileScene('structure')
  tr.reserveHits(n + 1024)
  for power in (False, True, False, True):          # (twice each, interleaved: drift of the clock shows as a difference between the pairs)
    tr.setDetector(det, power=power)
    for w in range(3):
      tr.reset(); tr.trace((1 << 40) + w * n, n, SEED)
    tr.sync(); tr.reset()
    t0 = time.perf_counter()
    for s in range(steps):
      tr.resetHits(); tr.trace(s * n, n, SEED)
    tr.sync()
    ms = (time.perf_counter() - t0) / steps * 1e3
    out.setdefault('power_ms' if power else 'count_ms', []).append(round(ms, 4))
    if power:
      assert np.array_equal(tr.powerHistogramRaw(), tr.histogram() << np.uint64(32))       # (all powers are 1 in this scene)
  out['ratio_power_over_count'] = round(min(out['power_ms']) / min(out['count_ms']), 4)
  out['rays_per_s_count'] = round(n / min(out['count_ms']) * 1e3, 1)
  out['rays_per_s_power'] = round(n / min(out['power_ms']) * 1e3, 1)
  # post-hoc: rows in HBM
  tr.setDetector(None)
  tr.reserveHits(rows + rows // 8)
  tr.reset(); tr.trace(0, rows, SEED); tr.sync()
  dh = tr.deviceHits(None)
  plane = dh.detectPlaneNormal()
  kw = dict(planeNormal=plane[0], xInPlaneVec=plane[1], bins=256)
  dh.histogram(**kw)                                   # warm-up
  t0 = time.perf_counter(); H = dh.histogram(**kw); t_count = time.perf_counter() - t0
  t0 = time.perf_counter(); W = dh.histogram(weights='powers', **kw); t_power = time.perf_counter() - t0
  assert np.array_equal(W.powerQuanta, H.hist.astype(np.uint64) << np.uint64(32))
  out.update(posthoc_rows=len(dh), posthoc_count_ms=round(t_count * 1e3, 3), posthoc_power_ms=round(t_power * 1e3, 3))
print(json.dumps(dict(rays_per_launch=n, steps=steps, **out)))
