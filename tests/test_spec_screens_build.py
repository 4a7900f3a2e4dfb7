"""The compiled kernels' box screens on |1/d| and -(o/d) as values and the flat entry faces of a box, the part that
needs no GPU (odw_kernels.hip: spec_reciprocals / ray_box_centred(SpecBox, SpecRecip, .) / intersect_prim<.., FLAT>;
tests/spec_screens_cases.py):

  * every case's header compiles for gfx950, and the CPU oracle records rows for the rays the GPU test sends;
  * the lens trains hold 7, 13 and 16 primitives with a box of their own, and the value image of the longest does not
    fit the kernel arguments (that of 13 still does);
  * the census of the headline kernel (lensesAndMirrors), against the BATCH variant compiled for the same scene in the
    same run -- the BATCH variant keeps the screens on oi / inv and the entry faces as three regions, which is what every
    compiled kernel had before --: no `v_and_b32 .. 0x7fffffff` + `v_mov_b32` pair is left and three fewer
    `v_xor_b32 .. 0x80000000` + `v_mov_b32` pairs (the reference has three of each behind the reciprocals), fewer canonicalising
    `v_max_f64 x, y, y` than the reference (7 against 34 when this was written), no VGPR spill, occupancy 4."""
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import spec_image_cases as cases
import spec_isolated_cases as ic
import spec_screens_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_ROWS = 1000


def compiles(native, pr, **kw):
  header, code_bytes = native.compile_check(pr.scene, pr.limits, 'structure', **kw)
  assert code_bytes > 10000
  return header


def oracle_rows(oracle, pr, o, d):
  res = oracle.trace_rays(pr.scene, pr.limits, o, d, flags=oracle.TRACE_RECORD_HITS, nthreads=0)
  assert res['counters']['traced_rays'] == len(o)
  return res['counters']['recorded_hits']


@pytest.mark.parametrize('mixed', [False, True])
def test_headline_rays_record(native_lib, oracle, mixed):
  from freecad.optics_design_workbench_amd import _native
  pr = sc.golden('lensesAndMirrors')
  compiles(_native, pr)
  assert oracle_rows(oracle, pr, *sc.rays_headline(pr, mixed=mixed)) >= MIN_ROWS


@pytest.mark.parametrize('n_own', [7, 13, 16])
def test_lens_trains(native_lib, oracle, n_own):
  from freecad.optics_design_workbench_amd import _native
  pr = sc.train(n_own)
  compiles(_native, pr)
  count, in_arguments = sc.own_boxes(_native, pr)
  assert count == n_own
  assert in_arguments == (n_own < 16)
  assert oracle_rows(oracle, pr, *sc.rays_train()) >= MIN_ROWS


@pytest.mark.parametrize('kind', sc.SPECIAL)
def test_special_rays_record(native_lib, oracle, kind):
  from freecad.optics_design_workbench_amd import _native
  pr = cases.small_scene()
  if kind == sc.SPECIAL[0]:
    compiles(_native, pr)
  o, d = sc.special_rays(_native, pr, kind)
  if kind == 'zero1':
    assert np.count_nonzero((d == 0).sum(axis=1) == 1) > len(d) // 2
  if kind == 'zero2':
    assert np.all((d == 0).sum(axis=1) == 2)
  assert oracle_rows(oracle, pr, o, d) >= MIN_ROWS


def test_other_cases_compile_and_record(native_lib, oracle):
  from freecad.optics_design_workbench_amd import _native
  pr = ic.coherent()
  compiles(_native, pr)
  assert oracle_rows(oracle, pr, *sc.rays_leaving()) >= MIN_ROWS
  seq = sc.golden('lensesAndMirrorsSequential')
  assert seq.scene.seq_enabled == 1
  assert 'seq() { return true; }' in compiles(_native, seq)
  res = oracle.trace(seq.scene, seq.source, seq.limits, 0, sc.N, sc.SEED, flags=oracle.TRACE_RECORD_HITS, nthreads=0)
  assert res['counters']['recorded_hits'] >= MIN_ROWS
  batch = sc.batch()
  assert len({compiles(_native, pr) for pr in batch}) == 1
  boxes = [_native.spec_image(pr.scene, pr.limits)['boxes'] for pr in batch]
  assert not np.array_equal(boxes[0], boxes[1]) and not np.array_equal(boxes[1], boxes[2])
  assert _native.compile_check_fresnel(ic.fresnel().scene, ic.fresnel().limits)[1] > 10000
  assert _native.compile_check_chroma(ic.chroma().scene, ic.chroma().limits)[1] > 10000


# ---- the census of the headline kernel ---------------------------------------------------------------------------------
def kernel_asm(native, header, opts=()):
  """the assembly of odw_spec_kernel for `header`, compiled as odw_spec.hip has hiprtc compile it"""
  csrc = native.CSRC
  d = tempfile.mkdtemp()
  try:
    open(os.path.join(d, 'odw_spec.h'), 'w').write(header)
    shutil.copy(os.path.join(csrc, 'odw_kernels.hip'), d)
    shutil.copy(os.path.join(ROOT, 'include', 'odw_trace.h'), d)
    text = open(os.path.join(csrc, 'odw_device.h')).read().replace('"../../../include/odw_trace.h"', '"odw_trace.h"')
    open(os.path.join(d, 'odw_device.h'), 'w').write(text)
    cmd = [native.hipcc(), '--offload-arch=gfx950', '-std=c++17', '-O3', '-ffp-contract=on', '-DODW_SPEC_HEADER="odw_spec.h"',
           *opts, '-I' + d, '-S', '--cuda-device-only', '-o', os.path.join(d, 'k.s'), os.path.join(d, 'odw_kernels.hip')]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-4000:]
    return open(os.path.join(d, 'k.s')).read()
  finally:
    shutil.rmtree(d, ignore_errors=True)


def figures(asm):
  lines = asm.splitlines()
  start = next(i for i, l in enumerate(lines) if l.startswith('odw_spec_kernel:'))
  end = next(i for i in range(start, len(lines)) if re.match(r'\s+s_endpgm', lines[i]))
  body = [l.strip() for l in lines[start:end] if re.match(r'\s+[a-z]', l)]
  pair = lambda first: sum(1 for a, b in zip(body, body[1:]) if re.match(first, a) and b.startswith('v_mov_b32'))
  # (the resource comments follow the kernel's body; its metadata entry names it and ends with the spill counts)
  after = '\n'.join(lines[end:])
  meta = re.search(r'\.name:\s+odw_spec_kernel\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)', asm)
  return dict(abs_pairs=pair(r'v_and_b32\S* v\d+, 0x7fffffff, v\d+'), neg_pairs=pair(r'v_xor_b32\S* v\d+, 0x80000000, v\d+'),
              self_max=sum(1 for l in body if re.match(r'v_max_f64 v\[[0-9:]+\], (v\[[0-9:]+\]), \1$', l)),
              occupancy=int(re.search(r'; Occupancy: (\d+)', after).group(1)), vgpr_spills=int(meta.group(1)))


def test_census_of_the_headline_kernel(native_lib):
  from freecad.optics_design_workbench_amd import _native
  pr = sc.golden('lensesAndMirrors')
  header = compiles(_native, pr)
  ref = figures(kernel_asm(_native, header, ['-DODW_SPEC_BATCH=true']))
  got = figures(kernel_asm(_native, header))
  print('reference (BATCH variant):', ref, ' kernel:', got)
  assert ref['abs_pairs'] >= 3 and ref['neg_pairs'] >= 3, \
      'the BATCH variant no longer has the screens on oi / inv: it is no reference for this census any more'
  # (one negation with a copy belongs to other code, in both kernels)
  assert got['abs_pairs'] == 0 and got['neg_pairs'] == ref['neg_pairs'] - 3
  assert got['self_max'] < ref['self_max']
  assert got['vgpr_spills'] == 0
  assert got['occupancy'] == 4
