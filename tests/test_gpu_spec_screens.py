"""Compiled kernels: the general loop's box screens on |1/d| and -(o/d) as values, and the flat entry faces of an
untrimmed box (odw_kernels.hip: spec_reciprocals, ray_box_centred(SpecBox, SpecRecip, .), intersect_prim<.., FLAT>).
Neither changes a computed value or which candidates reach consider_spec, so a compiled kernel's rows are the generic
flat kernel's (the binary tree's, for spectral and Fresnel launches) as byte strings, counters included; explicit rays,
2e4 per case (tests/spec_screens_cases.py; tests/test_spec_screens_build.py shows on the CPU oracle that every case
records its rows):

  (a) lensesAndMirrors with a coherent beam, and with neighbouring rays on three different paths;
  (b) lens trains with 7, with 13 and with 16 primitives that own a box (the image of the longest does not fit the
      kernel arguments; that of 13 still does);
  (c) direction components exactly 0 on one and on two axes, origins exactly on a box plane, rays along the edges of an
      axis-aligned box 0 and +-2 distTol off them;
  (d) rays leaving a convex lens whose sphere and cylinder share a box: the skipped solid with box_shared;
  (e) a scene in sequential mode, where the per-lane mask applies;
  (f) a batch of three scenes whose boxes differ (the BATCH variant keeps the screens and faces it had);
  (g) one Fresnel 'Split' launch and one spectral launch against the tree route."""
import numpy as np
import pytest

import spec_image_cases as cases
import spec_isolated_cases as ic
import spec_screens_cases as sc

pytestmark = pytest.mark.gpu

MIN_ROWS = 1000
LINES = (486.1327, 587.5618, 656.2725)


@pytest.fixture(scope='module')
def tracers(native_lib):
  from freecad.optics_design_workbench_amd.simulation.tracer import Tracer
  made = {}

  def get(mode):
    if mode not in made:
      made[mode] = Tracer(0)
      made[mode].compileScene(mode)
    return made[mode]
  yield get
  for tr in made.values():
    tr.close()


def run(tr, pr, o, d, wavelengths=None, seed=None):
  tr.setScene(pr.scene)
  tr.setLimits(pr.limits)
  tr.setDetector(None)
  tr.reserveHits(16 * len(o))
  if seed is not None:
    tr.setSurfaceSeed(seed)
  tr.reset()
  tr.traceRays(o, d, histogram=False, wavelengths=wavelengths)
  tr.sync()
  return dict(counters=tr.counters(), hits=tr.hits(), info=tr.compiledInfo())


def same_bytes(got, ref):
  assert got['counters'] == ref['counters']
  assert ref['counters']['hits_dropped'] == 0
  assert len(got['hits']) == len(ref['hits'])
  assert got['hits'].tobytes() == ref['hits'].tobytes()


def both(tracers, pr, o, d, **kw):
  ref = run(tracers('off'), pr, o, d, **kw)
  got = run(tracers('structure'), pr, o, d, **kw)
  assert ref['info']['mode'] == 0 and got['info']['mode'] == 1
  assert ref['counters']['traced_rays'] == len(o)
  assert ref['counters']['recorded_hits'] >= MIN_ROWS
  same_bytes(got, ref)
  return got


@pytest.mark.parametrize('mixed', [False, True])
def test_headline_scene(tracers, mixed):
  pr = sc.golden('lensesAndMirrors')
  both(tracers, pr, *sc.rays_headline(pr, mixed=mixed))


@pytest.mark.parametrize('n_own', [7, 13, 16])
def test_lens_trains(tracers, native_lib, n_own):
  from freecad.optics_design_workbench_amd import _native
  pr = sc.train(n_own)
  assert sc.own_boxes(_native, pr) == (n_own, n_own < 16)
  both(tracers, pr, *sc.rays_train())


@pytest.mark.parametrize('kind', sc.SPECIAL)
def test_special_rays(tracers, native_lib, kind):
  from freecad.optics_design_workbench_amd import _native
  pr = cases.small_scene()
  both(tracers, pr, *sc.special_rays(_native, pr, kind))


def test_leaving_a_lens_whose_operands_share_a_box(tracers):
  both(tracers, ic.coherent(), *sc.rays_leaving())


def source_rows(mode, pr, n):
  from freecad.optics_design_workbench_amd.simulation.tracer import Tracer
  with Tracer(0) as tr:
    tr.setScene(pr.scene)
    tr.setSource(pr.source)
    tr.setLimits(pr.limits)
    tr.setDetector(None)
    info = tr.compileScene(mode)
    assert info['mode'] == (1 if mode == 'structure' else 0), info
    tr.reserveHits(16 * n)
    tr.trace(0, n, sc.SEED)
    tr.sync()
    return dict(counters=tr.counters(), hits=tr.hits())


def test_sequential_mode(native_lib):
  pr = sc.golden('lensesAndMirrorsSequential')
  assert pr.scene.seq_enabled == 1
  ref, got = source_rows('off', pr, sc.N), source_rows('structure', pr, sc.N)
  assert ref['counters']['traced_rays'] == sc.N and ref['counters']['recorded_hits'] >= MIN_ROWS
  same_bytes(got, ref)


def test_batch_of_scenes_whose_boxes_differ(native_lib):
  from freecad.optics_design_workbench_amd.simulation.tracer import Tracer
  batch = sc.batch()
  rows = {}
  for mode in ('off', 'structure'):
    with Tracer(0) as tr:
      tr.compileScene(mode)
      tr.setLimits(batch[0].limits)
      tr.setSource(batch[0].source)
      tr.setSceneBatch([b.scene for b in batch])
      tr.reset()
      tr.traceBatch(0, sc.N, sc.SEED, 16 * sc.N)
      tr.sync()
      cnt = tr.counters()
      assert cnt['traced_rays'] == 3 * sc.N and cnt['hits_dropped'] == 0
      assert tr.compiledInfo()['mode'] == (1 if mode == 'structure' else 0)
      out = []
      for k in range(3):
        tr.batchSelect(k)
        hits = tr.hits()
        assert len(hits) >= MIN_ROWS
        out.append(hits.tobytes())
      tr.batchSelect(None)
      rows[mode] = (cnt, out)
  assert rows['structure'] == rows['off']


def test_spectral_launch(tracers):
  o, d = ic.rays_mixed()
  wl = np.asarray(LINES)[np.arange(len(o)) % len(LINES)]
  got = both(tracers, ic.chroma(), o, d, wavelengths=wl)
  assert got['info']['chroma'] == 1


def test_fresnel_split_launch(tracers):
  o, d = ic.rays_mixed()
  got = both(tracers, ic.fresnel(), o, d, seed=ic.SEED)
  assert got['info']['fresnel'] == 1
