"""Compiled kernels on their value image (csrc/odw_build.h: spec_image_build; odw_kernels.hip: the SPEC paths): box
screens on centre and half extent, frames / parameters / derived constants / group constants read from the image, in
the kernel arguments or behind one pointer.

  * constants: the device expressions the image replaces, evaluated by a kernel of their own (tests/native/
    spec_constants_main.hip, compiled with the options of the compiled kernels) for a few hundred parameter sets, are the
    image's words bit for bit -- the contraction rule of the builder;
  * rows: the compiled kernel's rows are the generic flat kernel's as byte strings, 1e5 explicit rays per case: directions
    with one and with two exact zero components, origins at coordinate 0 and on box planes, rays grazing box edges and
    cylinder rims within +-1.5 distTol, a beam through a torus's hole and a lens beside a tilted mirror box; an image
    that fits the arguments (8 primitives) and one that does not (41); a batch of 3 scenes; and the same structure after
    setScene with other radii and after setLimits with another tolerance or ray length -- which a stale image fails."""
import dataclasses
import os
import subprocess

import numpy as np
import pytest

import spec_image_cases as cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 100000
SEED = 0x0D15EA5E


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


def run(tr, pr, o, d, upload=True):
  if upload:
    tr.setScene(pr.scene)
    tr.setLimits(pr.limits)
    tr.setDetector(None)
    tr.reserveHits(16 * len(o))
  tr.reset()
  tr.traceRays(o, d, histogram=False)
  tr.sync()
  return dict(counters=tr.counters(), hits=tr.hits(), info=tr.compiledInfo())


def same_bytes(got, ref):
  assert got['counters'] == ref['counters']
  assert ref['counters']['hits_dropped'] == 0
  assert len(got['hits']) == len(ref['hits'])
  assert got['hits'].tobytes() == ref['hits'].tobytes()


def both(tracers, pr, o, d, min_rows):
  ref = run(tracers('off'), pr, o, d)
  got = run(tracers('structure'), pr, o, d)
  assert ref['info']['mode'] == 0 and got['info']['mode'] == 1
  assert ref['counters']['traced_rays'] == len(o)
  assert ref['counters']['recorded_hits'] >= min_rows
  same_bytes(got, ref)
  return got


@pytest.fixture(scope='module')
def small():
  return cases.small_scene()


@pytest.fixture(scope='module')
def small_boxes(small, native_lib):
  from freecad.optics_design_workbench_amd import _native
  im = _native.spec_image(small.scene, small.limits)
  assert im['in_arguments'] and len(small.scene.prim_type) == 8
  return im['boxes']


def test_device_expressions_equal_the_image(native_lib, tmp_path):
  from freecad.optics_design_workbench_amd import _native
  records, want = [], []
  for seed, tol in ((11, '1e-6'), (12, '1e-3'), (13, '1e-9'), (14, '1e-6'), (15, '1e-4'), (16, '1e-6')):
    pr = cases.zoo(np.random.RandomState(seed), tol, n_each=9)
    im = _native.spec_image(pr.scene, pr.limits)
    keep, rec = cases.constant_records(pr)
    for p, r in zip(keep, rec):
      k = len(cases.expected_derived(int(r[0]), r[1:5], r[5]))
      w = np.zeros(4)
      w[:k] = im['image'][im['der'][p]:im['der'][p] + k]
      records.append(r)
      want.append((k, w))
  records = np.asarray(records, np.float64)
  assert len(records) >= 250
  exe = str(tmp_path / 'spec_constants_main')
  # the options odw_spec.hip hands the run-time compiler
  cmd = [_native.hipcc(), '--offload-arch=gfx950', '-std=c++17', '-O3', '-ffp-contract=on', '-o', exe,
         os.path.join(ROOT, 'tests', 'native', 'spec_constants_main.hip')]
  res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
  assert res.returncode == 0, res.stderr[-4000:]
  records.tofile(str(tmp_path / 'in.bin'))
  res = subprocess.run([exe, str(tmp_path / 'in.bin'), str(tmp_path / 'out.bin')], capture_output=True, text=True, timeout=60)
  assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-2000:])
  got = np.fromfile(str(tmp_path / 'out.bin'), np.float64).reshape(-1, 4)
  assert len(got) == len(records)
  for r, g, (k, w) in zip(records, got, want):
    assert cases.bits(g[:k]).tolist() == cases.bits(w[:k]).tolist(), (r, g, w)


@pytest.mark.parametrize('zeros', [1, 2])
def test_exact_zero_direction_components(tracers, small, zeros):
  o, d = cases.rays_zero_components(np.random.RandomState(20 + zeros), N, zeros)
  assert ((d == 0).sum(axis=1) >= zeros).sum() >= N * 2 // 3
  both(tracers, small, o, d, min_rows=N // 4)


def test_origins_at_zero_and_on_box_planes(tracers, small, small_boxes):
  o, d = cases.rays_special_origins(np.random.RandomState(23), N, small_boxes)
  assert (o == 0).any(axis=1).sum() > N // 4
  both(tracers, small, o, d, min_rows=N // 4)


def test_grazing_box_edges_and_cylinder_rims(tracers, small):
  tol = small.limits.dist_tol
  o, d = cases.rays_grazing(np.random.RandomState(24), N, tol)
  got = both(tracers, small, o, d, min_rows=N // 2)
  # the tolerance decides for a good part of these rays: some meet the grazed solid, some pass it by
  groups = (got['hits']['tag'] >> np.uint64(48)) & np.uint64(0x7FFF)
  assert len(np.unique(groups)) >= 2


def test_lens_mirror_box_and_torus_hole(tracers, small):
  o, d = cases.rays_bench(np.random.RandomState(25), N)
  got = both(tracers, small, o, d, min_rows=N)
  groups = set(np.unique((got['hits']['tag'] >> np.uint64(48)) & np.uint64(0x7FFF)).tolist())
  assert len(groups) == 3                      # lens, mirrors (box and torus), absorbers


def test_image_beyond_the_arguments(tracers, native_lib):
  from freecad.optics_design_workbench_amd import _native
  train = cases.lens_train(13)
  assert len(train.scene.prim_type) == 41 and not _native.spec_image(train.scene, train.limits)['in_arguments']
  rs = np.random.RandomState(26)
  o, d = cases.rays_bench(rs, N)
  first = both(tracers, train, o, d, min_rows=N)
  # other radii under the same structure, then another tolerance and ray length: the image in device memory follows
  other = cases.lens_train(13, radius=36.0)
  got = run(tracers('structure'), other, o, d)
  assert got['info']['cache'] == 1 and got['hits'].tobytes() != first['hits'].tobytes()
  same_bytes(got, run(tracers('off'), other, o, d))
  short = dataclasses.replace(other.limits, max_ray_length=150.0, dist_tol=1e-3)
  for mode in ('off', 'structure'):
    tracers(mode).setLimits(short)
  got2 = run(tracers('structure'), other, o, d, upload=False)
  assert got2['counters'] != got['counters']
  same_bytes(got2, run(tracers('off'), other, o, d, upload=False))


def test_set_scene_with_other_radii(tracers, small):
  """a sweep step: the bound kernel stays, the image must not"""
  rs = np.random.RandomState(27)
  o, d = cases.rays_bench(rs, N)
  o2, d2 = cases.rays_grazing(rs, N // 2, small.limits.dist_tol)
  o, d = np.r_[o[:N // 2], o2], np.r_[d[:N // 2], d2]
  tr = tracers('structure')
  before = run(tr, small, o, d)
  other = cases.small_scene(radius=24.0, torus=(7.0, 2.0))
  got = run(tr, other, o, d)
  assert got['info']['mode'] == 1 and got['info']['cache'] == 1          # the same kernel, from the process cache
  assert got['hits'].tobytes() != before['hits'].tobytes()
  same_bytes(got, run(tracers('off'), other, o, d))


@pytest.mark.parametrize('change', ['dist_tol', 'max_ray_length'])
def test_set_limits(tracers, small, change):
  rs = np.random.RandomState(28)
  o, d = cases.rays_grazing(rs, N, 4e-4)          # within +-6e-4 of edges and rims: 1e-6 and 1e-3 judge them differently
  tr = tracers('structure')
  before = run(tr, small, o, d)
  lim = dataclasses.replace(small.limits, dist_tol=1e-3) if change == 'dist_tol' else dataclasses.replace(small.limits, max_ray_length=60.0)
  tr.setLimits(lim)
  got = run(tr, small, o, d, upload=False)
  assert got['info']['mode'] == 1
  assert got['hits'].tobytes() != before['hits'].tobytes()
  ref = tracers('off')
  run(ref, small, o, d)
  ref.setLimits(lim)
  same_bytes(got, run(ref, small, o, d, upload=False))


def test_batch_of_three_scenes(native_lib):
  from freecad.optics_design_workbench_amd.simulation.tracer import Tracer
  batch = [cases.small_scene(radius=r, torus=t) for r, t in ((30.0, (6.0, 1.5)), (24.0, (7.0, 2.0)), (40.0, (5.5, 1.0)))]
  rows = {}
  for mode in ('off', 'structure'):
    with Tracer(0) as tr:
      tr.compileScene(mode)
      tr.setLimits(batch[0].limits)
      tr.setSource(batch[0].source)
      tr.setSceneBatch([b.scene for b in batch])
      tr.reset()
      tr.traceBatch(0, N, SEED, 8 * N)
      tr.sync()
      assert tr.counters()['traced_rays'] == 3 * N
      assert tr.compiledInfo()['mode'] == (1 if mode == 'structure' else 0)
      out = []
      for k in range(3):
        tr.batchSelect(k)
        out.append(tr.hits().tobytes())
      tr.batchSelect(None)
      rows[mode] = out
  assert len(set(rows['off'])) == 3 and min(len(r) for r in rows['off']) >= 64 * N
  assert rows['structure'] == rows['off']
