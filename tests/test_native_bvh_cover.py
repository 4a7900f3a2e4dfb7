"""The tables build_accel (csrc/odw_build.h) hands the binary-tree walk (odw_kernels.hip, nearest<BVH = true>) and the mesh
kernel, checked by brute force in a program of their own (tests/native/bvh_cover_main.hip) under AddressSanitizer +
UndefinedBehaviorSanitizer: every live primitive in exactly one leaf, child boxes in float32 around everything below them,
max_depth the true height and within the walk's stack (the coincident layouts reach 20 levels and more), leaf words that
decode back with the kernel's expressions, the eight-wide tree's slots around what they collapse -- on the layouts of
tests/grid_cases.py, the moved lattice, coincident boxes, a geometric chain, 5000 random boxes, boxes on a line, the
wrapper roots, cubes of 12 triangles and boxes whose area overflows.  The program links the sanitizer runtime itself:
no GPU, no Python in the process, nothing preloaded."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tree_tables_cover_their_primitives_under_asan_ubsan(tmp_path):
  from freecad.optics_design_workbench_amd import _native
  try:
    hipcc = _native.hipcc()
  except _native.NativeError:
    pytest.skip('hipcc not found')
  exe = str(tmp_path / 'bvh_cover_main')
  # (host code only: -fno-gpu-sanitize keeps the device side, which this program never runs, a plain gfx950 build)
  flags = '--offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=on -fsanitize=address,undefined -fno-gpu-sanitize -fno-omit-frame-pointer'
  cmd = [hipcc] + flags.split() + ['-I', _native.CSRC, '-o', exe, os.path.join(ROOT, 'tests', 'native', 'bvh_cover_main.hip')]
  res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
  assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-6000:]
  env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
  res = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
  print(res.stdout)
  assert res.returncode == 0, (res.stdout[-3000:], res.stderr[-6000:])
  assert 'runtime error' not in res.stderr and 'AddressSanitizer' not in res.stderr, res.stderr[-6000:]
  assert '17 layouts checked, 0 mismatches' in res.stdout, res.stdout[-3000:]
  # the depths reached: the coincident layouts exercise the bound of the walk's stack
  for name in ('80 coincident', '1000 coincident'):
    line = next(ln for ln in res.stdout.splitlines() if ln.startswith(name))
    depth = int(line.split('depth')[1].split('of')[0])
    assert 20 <= depth <= 30, line
