#!/usr/bin/env python3
"""What Fresnel reflection costs (profiles/fresnel.md): the singlet / prism bench of bench_spectral.py (monochromatic) and
a train of lenses (bench_lens_train.py's), every lens group with Fresnel '' / 'Loss' / 'Split', hit rows of the detector
only --
  plain-generic     no mode: the kernel the library picks without compilation (flat or grid)
  plain-compiled    no mode, the kernel compiled against the scene
  loss-compiled / split-compiled   the FRESNEL variant of the compiled kernel (like for like with plain-compiled)
  loss-tree / split-tree           the FRESNEL instantiation of the binary tree (a plain launch of scenes this small never
                                   takes the tree, so these rows have no like-for-like partner)
  lossQ-compiled / lossW-compiled / lossQ-tree / lossW-tree   'Loss' with a thin-film coating on every lens group: one
                                   quarter-wave layer (Q) and a three-layer broadband stack (W) (profiles/coating.md)
same build, same process, each twice and interleaved (drift of the clock shows as a difference between the pairs).
Under 'Split' a ray can take more segments than without: segments per ray are printed beside the times.
  bench_fresnel.py [rays per launch] [steps] [lenses of the train]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from freecad.optics_design_workbench_amd.freecad_elements import make, point_source
from freecad.optics_design_workbench_amd.scene import Document, bake
from freecad.optics_design_workbench_amd.scene.placement import Placement
from freecad.optics_design_workbench_amd.simulation.tracer import Tracer

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10_000_000
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
train = int(sys.argv[3]) if len(sys.argv) > 3 else 5
SEED = 0x0D15EA5E
COATINGS = dict(Q=[make.quarterWave(make.MGF2, 550.0)], W=[(1.38, 99.6), (2.0, 137.5), (1.62, 84.9)])


def singlet_prism(fresnel, coating=()):
  doc = Document()
  h = np.sin(np.radians(-60.0)), np.cos(np.radians(-60.0))       # quaternion of the turn by -120 degrees about y
  make.makeLens(doc, [make.makeCommon(doc, [make.makeSphere(doc, 'S1', 50.0, base=(0, 0, 50.0)),
                                            make.makeSphere(doc, 'S2', 50.0, base=(0, 0, -44.0))], name='Singlet')],
                name='Singlet_', RefractiveIndex=1.5168, Fresnel=fresnel, Coating=list(coating), **make.N_BK7)
  make.makeLens(doc, [make.makeCommon(doc, [make.makeBox(doc, 'PA', 60.0, 40.0, 60.0, base=(-40.0, -20.0, 30.0)),
                                            make.makeBox(doc, 'PB', 60.0, 40.0, 60.0, base=(20.0, -20.0, 30.0), quat=(0.0, h[0], 0.0, h[1]))],
                                      name='Prism')],
                name='Prism_', RefractiveIndex=1.62, Dispersion='Cauchy', DispersionCoefficients=[1.5950, 0.0105, 0.0002], Fresnel=fresnel,
                Coating=list(coating))
  make.makeAbsorber(doc, [make.makeSphere(doc, 'Shell', 400.0)], name='Detector_')
  make.makeSimulationSettings(doc, DistanceTolerance='1e-6')
  src = make.makePointSource(doc, placement=Placement(base=(0.0, 0.0, -50.0)), Wavelength=make.LINE_d)
  return bake.bakeScene(doc, src), bake.bakeLimits(doc, src), point_source.bakeSource(doc, src)


def lens_train(fresnel, k, coating=()):
  doc = Document()
  lenses = []
  for j in range(k):
    z = 30.0 + 12.0 * j
    a = make.makeSphere(doc, f'A{j}', 30.0, base=(0, 0, z + 28.0))
    b = make.makeSphere(doc, f'B{j}', 30.0, base=(0, 0, z - 28.0))
    c = make.makeCylinder(doc, f'C{j}', 6.0, 6.0, base=(0, 0, z - 3.0))
    lenses.append(make.makeCommon(doc, [a, b, c], f'L{j}'))
  make.makeLens(doc, lenses, RefractiveIndex=1.5, Fresnel=fresnel, Coating=list(coating))
  make.makeAbsorber(doc, [make.makeBox(doc, 'S', 60, 60, 1, base=(-30, -30, 30.0 + 12.0 * k + 20))], RecordHits=True)
  make.makeSimulationSettings(doc)
  src = make.makePointSource(doc, PowerDensity='exp(-theta**2/0.08**2)')
  return bake.bakeScene(doc, src), bake.bakeLimits(doc, src), point_source.bakeSource(doc, src)


def measure(tr, sc, lim, src):
  tr.setScene(sc); tr.setSource(src); tr.setLimits(lim); tr.setDetector(None)
  tr.reserveHits(2 * n + 1024)
  for w in range(2):
    tr.reset(); tr.trace((1 << 40) + w * n, n, SEED)
  tr.sync(); tr.reset()
  t0 = time.perf_counter()
  for s in range(steps):
    tr.resetHits(); tr.trace(s * n, n, SEED)
  tr.sync()
  ms = (time.perf_counter() - t0) / steps * 1e3
  cnt = tr.counters()
  assert cnt['traced_rays'] == steps * n and cnt['hits_dropped'] == 0, cnt
  return ms, cnt['segments'] / cnt['traced_rays'], cnt['recorded_hits'] / cnt['traced_rays']


for bench, make_scene in (('singlet-prism', singlet_prism), (f'train-{train}', lambda f, c=(): lens_train(f, train, c))):
  scenes = {f: make_scene(f) for f in ('', 'Loss', 'Split')}
  scenes.update({'Loss' + c: make_scene('Loss', layers) for c, layers in COATINGS.items()})
  rows = [('plain-generic', 'off', ''), ('plain-compiled', 'structure', ''), ('loss-compiled', 'structure', 'Loss'),
          ('split-compiled', 'structure', 'Split'), ('loss-tree', 'off', 'Loss'), ('split-tree', 'off', 'Split'),
          ('lossQ-compiled', 'structure', 'LossQ'), ('lossW-compiled', 'structure', 'LossW'), ('lossQ-tree', 'off', 'LossQ'),
          ('lossW-tree', 'off', 'LossW')]
  tracers = {name: Tracer(0) for name, _, _ in rows}
  out, per_ray = {}, {}
  try:
    for name, mode, _ in rows:
      tracers[name].compileScene(mode)
    for rep in range(2):
      for name, mode, f in rows:
        ms, segs, hits = measure(tracers[name], *scenes[f])
        out.setdefault(name + '_ms', []).append(round(ms, 4))
        per_ray[name] = dict(segments_per_ray=round(segs, 3), hits_per_ray=round(hits, 4))
    info = {name: tracers[name].compiledInfo() for name, _, _ in rows}
  finally:
    for t in tracers.values():
      t.close()
  best = {k[:-3]: min(v) for k, v in out.items()}
  out.update({'rays_per_s_' + k: round(n / v * 1e3, 1) for k, v in best.items()})
  for f in ('loss', 'split'):
    out[f'ratio_{f}_compiled_over_plain_compiled'] = round(best[f + '-compiled'] / best['plain-compiled'], 4)
    out[f'ratio_{f}_tree_over_plain_generic'] = round(best[f + '-tree'] / best['plain-generic'], 4)
    out[f'ratio_{f}_tree_over_{f}_compiled'] = round(best[f + '-tree'] / best[f + '-compiled'], 4)
  for c in COATINGS:
    out[f'ratio_loss{c}_compiled_over_loss_compiled'] = round(best[f'loss{c}-compiled'] / best['loss-compiled'], 4)
    out[f'ratio_loss{c}_tree_over_loss_tree'] = round(best[f'loss{c}-tree'] / best['loss-tree'], 4)
  out['compiled'] = {name: dict(mode=i['mode'], fresnel=i['fresnel']) for name, i in info.items()}
  print(json.dumps(dict(bench=bench, prims=len(scenes[''][0].prim_type), rays_per_launch=n, steps=steps, per_ray=per_ray, **out)), flush=True)
