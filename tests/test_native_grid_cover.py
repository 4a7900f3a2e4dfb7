"""The tables build_grid (csrc/odw_build.h) hands the grid kernel, checked by brute force in a program of their own
(tests/native/grid_cover_main.hip) under AddressSanitizer + UndefinedBehaviorSanitizer: planes that increase and enclose
every box, every (cell, primitive) pair whose boxes touch listed exactly once, cell words that agree with the lists,
sphere records that repeat their primitives, and the LDS figures of the kernel's own offset arithmetic -- on the layouts of
tests/grid_cases.py, a line of 300 spheres (the even division, planes through boxes) and a cloud build_grid refuses.  The
program links the sanitizer runtime itself: no GPU, no Python in the process, nothing preloaded."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_grid_tables_cover_their_cells_under_asan_ubsan(tmp_path):
  from freecad.optics_design_workbench_amd import _native
  try:
    hipcc = _native.hipcc()
  except _native.NativeError:
    pytest.skip('hipcc not found')
  exe = str(tmp_path / 'grid_cover_main')
  # (host code only: -fno-gpu-sanitize keeps the device side, which this program never runs, a plain gfx950 build)
  flags = '--offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=on -fsanitize=address,undefined -fno-gpu-sanitize -fno-omit-frame-pointer'
  cmd = [hipcc] + flags.split() + ['-I', _native.CSRC, '-o', exe, os.path.join(ROOT, 'tests', 'native', 'grid_cover_main.hip')]
  res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
  assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-6000:]
  env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
  res = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
  print(res.stdout)
  assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-6000:])
  assert 'runtime error' not in res.stderr and 'AddressSanitizer' not in res.stderr, res.stderr[-6000:]
  assert '8 layouts checked, 0 mismatches' in res.stdout, res.stdout[-2000:]
