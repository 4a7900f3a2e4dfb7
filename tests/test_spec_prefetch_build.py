"""Compiled kernels ask for every primitive's box block one primitive ahead (odw_kernels.hip: spec_prims / spec_prim /
spec_box).  The offsets they ask for are checked where they are formed, by static_assert against the image's size: a
structure whose chain of blocks would step outside its image does not compile.  So every structure is compiled here,
without a GPU (`_native.compile_check` cross-compiles for gfx950): the golden scenes inside the compiled kernels'
domain, with the ray generation of their own source and without, and the hand-built structures of
tests/spec_prefetch_cases.py -- each of which is first shown to have the property it is there for, and to record rows
on the CPU oracle for the rays the GPU test sends."""
import numpy as np
import pytest

import spec_prefetch_cases as pc
from conftest import project

# every golden scene with a point source and a scene the flat loop takes (the others -- hugeArray, the surface and
# replay sources, the documents without a source -- are outside the compiled kernels' domain)
GOLDEN = ['GettingStarted', 'edmund-optics-lens', 'gaussian', 'global-placement-main', 'grating', 'lens-overlap', 'lensesAndMirrors',
          'lensesAndMirrorsSequential', 'minimal', 'mirror', 'mirror-diffuse', 'nested-structure', 'nesting', 'playground',
          'source-and-absorber']


def compiles(native, scene, limits, source=None):
  header, code_bytes = native.compile_check(scene, limits, 'structure', source=source)
  assert 'static constexpr int IMG = ' in header and 'static constexpr int box(int i)' in header
  assert code_bytes > 10000
  return header


@pytest.mark.parametrize('name', GOLDEN)
def test_golden_scenes_compile(native_lib, name):
  from freecad.optics_design_workbench_amd import _native
  proj = project(name)
  compiles(_native, proj.scene, proj.limits, source=proj.source)


@pytest.mark.parametrize('name', sorted(pc.SINGLE_SCENES))
def test_hand_built_structures_compile_and_record(native_lib, oracle, name):
  from freecad.optics_design_workbench_amd import _native
  pr = pc.SINGLE_SCENES[name]()
  pc.check_structure(name, pr, _native.spec_image(pr.scene, pr.limits))
  header = compiles(_native, pr.scene, pr.limits)
  if name == 'sequential':
    assert 'seq() { return true; }' in header
  # the rays of tests/test_gpu_spec_prefetch.py record enough rows in this scene
  o, d = pc.rays()
  res = oracle.trace_rays(pr.scene, pr.limits, o, d, flags=oracle.TRACE_RECORD_HITS, nthreads=0)
  assert res['counters']['traced_rays'] == pc.N and res['counters']['recorded_hits'] >= 1000


def test_batch_and_sweep_scenes_share_one_structure(native_lib, oracle):
  from freecad.optics_design_workbench_amd import _native
  first, second = pc.other_radii()
  headers = {compiles(_native, pr.scene, pr.limits) for pr in pc.batch() + [first, second]}
  assert len(headers) == 1                             # one kernel; the values differ
  assert not np.array_equal(_native.spec_image(first.scene, first.limits)['image'], _native.spec_image(second.scene, second.limits)['image'])
  o, d = pc.rays()
  for pr in (first, second):
    assert oracle.trace_rays(pr.scene, pr.limits, o, d, flags=oracle.TRACE_RECORD_HITS, nthreads=0)['counters']['recorded_hits'] >= 1000
  # (the batch generates its rays from the scenes' source)
  for pr in pc.batch():
    res = oracle.trace(pr.scene, pr.source, pr.limits, 0, pc.N, pc.SEED, flags=oracle.TRACE_RECORD_HITS, nthreads=0)
    assert res['counters']['recorded_hits'] >= 1000
