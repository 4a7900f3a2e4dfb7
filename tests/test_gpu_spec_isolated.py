"""Compiled kernels: the wave-uniform path inside an isolated solid (odw_kernels.hip: nearest() / spec_uniform).  A wave
whose live lanes have all just entered the same isolated lens searches that lens's primitives alone -- no reciprocals,
no box screens, no predicates --, every other wave runs the general loop; which solids are isolated is read from one
word of the scene's value image.  The rule never changes a result: the compiled kernel's rows are the generic flat
kernel's (the binary tree's, for spectral and Fresnel launches) as byte strings, counters included, 2e4 explicit rays
per case (tests/spec_isolated_cases.py; tests/test_spec_isolated_build.py shows on the CPU oracle that every case
records its rows):

  * a coherent beam through mirror, two isolated lenses and screen -- every wave takes the path;
  * the same scene with neighbouring ray indices on different paths -- waves are mixed, the general loop runs with
    lanes that have just entered a lens;
  * rays onto the rim of a lens face and along its wall, 0, +-0.5 and +-2 distTol off: on the CPU oracle EDGE_PASS_BY
    of them enter the lens and pass it by -- the short search finds nothing and the segment is done again;
  * a concave lens (Cut(cylinder, sphere)): isolated, not convex;
  * a lens that is not isolated (a mirror's box within 4 distTol of its box): its bit is clear, the other lens's is set;
  * setScene moving that mirror away and back under the bound kernel: one kernel, the mask follows the scene;
  * a batch of three scenes whose masks differ (the BATCH variant carries the general loop alone: its rows must not
    depend on the masks its images hold);
  * a source inside a lens;
  * one spectral and one Fresnel 'Split' launch."""
import numpy as np
import pytest

import spec_isolated_cases as ic

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


CASES = dict(coherent=(ic.coherent, ic.rays_beam), mixed=(ic.coherent, ic.rays_mixed), edges=(ic.coherent, ic.rays_edges),
             concave=(ic.concave, ic.rays_fan), not_isolated=(ic.not_isolated, ic.rays_beam), inside=(ic.coherent, ic.rays_inside))


@pytest.mark.parametrize('name', sorted(CASES))
def test_rows_equal_the_generic_kernels(tracers, native_lib, name):
  from freecad.optics_design_workbench_amd import _native
  scene, rays = CASES[name]
  pr = scene()
  mask, _ = ic.mask_word(_native, pr)
  lenses = ic.lens_solids(pr)
  if name == 'not_isolated':
    assert (mask >> lenses[0]) & 1 and not (mask >> lenses[1]) & 1
  else:
    assert all((mask >> s) & 1 for s in lenses)
  got = both(tracers, pr, *rays())
  if name == 'edges':
    # (the oracle counts EDGE_PASS_BY = 1432 such rays, tests/test_spec_isolated_build.py; the device's arithmetic
    #  agrees with the oracle's to 1e-9 mm, not to the bit, and rays aimed exactly at an edge may fall either way:
    #  1559 on an MI355X -- the case holds them on the device too, which is what it is there for)
    assert ic.EDGE_PASS_BY > 0 and ic.passes_by(got['hits'], pr) > 0


def test_isolation_flips_under_a_bound_kernel(tracers, native_lib):
  from freecad.optics_design_workbench_amd import _native
  away, near = ic.flip()
  (mask_away, header_away), (mask_near, header_near) = ic.mask_word(_native, away), ic.mask_word(_native, near)
  lens_b = ic.lens_solids(away)[1]
  assert header_away == header_near and (mask_away >> lens_b) & 1 and not (mask_near >> lens_b) & 1
  o, d = ic.rays_beam()
  first = both(tracers, away, o, d)
  # isolated -> not isolated -> isolated again, the same kernel every time
  for pr in (near, away):
    got = run(tracers('structure'), pr, o, d)
    assert got['info']['mode'] == 1 and got['info']['cache'] == 1
    same_bytes(got, run(tracers('off'), pr, o, d))
  same_bytes(got, first)


def test_batch_with_masks_of_its_own_per_scene(native_lib):
  from freecad.optics_design_workbench_amd import _native
  from freecad.optics_design_workbench_amd.simulation.tracer import Tracer
  batch = ic.batch()
  lens_b = ic.lens_solids(batch[0])[1]
  assert [(ic.mask_word(_native, pr)[0] >> lens_b) & 1 for pr in batch] == [1, 0, 1]
  rows = {}
  for mode in ('off', 'structure'):
    with Tracer(0) as tr:
      tr.compileScene(mode)
      tr.setLimits(batch[0].limits)
      tr.setSource(batch[0].source)
      tr.setSceneBatch([b.scene for b in batch])
      tr.reset()
      tr.traceBatch(0, ic.N, ic.SEED, 16 * ic.N)
      tr.sync()
      cnt = tr.counters()
      assert cnt['traced_rays'] == 3 * ic.N and cnt['hits_dropped'] == 0
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
  pr = ic.chroma()
  o, d = ic.rays_beam()
  wl = np.asarray(LINES)[np.arange(len(o)) % len(LINES)]
  got = both(tracers, pr, o, d, wavelengths=wl)
  assert got['info']['chroma'] == 1


def test_fresnel_split_launch(tracers):
  pr = ic.fresnel()
  o, d = ic.rays_beam()
  got = both(tracers, pr, o, d, seed=ic.SEED)
  assert got['info']['fresnel'] == 1
