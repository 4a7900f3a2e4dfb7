"""The host twin of the coated reflectance and odw_set_coating's validation (csrc/odw_build.h) -- the reflectance against
complex characteristic matrices in extended precision and its closed forms, the validation against tables made to be
refused -- in a program of its own (tests/native/coating_main.hip) under AddressSanitizer + UndefinedBehaviorSanitizer.
The program links the sanitizer runtime itself: no GPU, no Python in the process, nothing preloaded."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_coating_host_code_under_asan_ubsan(tmp_path):
  from freecad.optics_design_workbench_amd import _native
  try:
    hipcc = _native.hipcc()
  except _native.NativeError:
    pytest.skip('hipcc not found')
  exe = str(tmp_path / 'coating_main')
  # (host code only: -fno-gpu-sanitize keeps the device side, which this program never runs, a plain gfx950 build)
  flags = '--offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=on -fsanitize=address,undefined -fno-gpu-sanitize -fno-omit-frame-pointer'
  cmd = [hipcc] + flags.split() + ['-I', _native.CSRC, '-o', exe, os.path.join(ROOT, 'tests', 'native', 'coating_main.hip')]
  res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
  assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-6000:]
  env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
  res = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
  assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-6000:])
  assert 'runtime error' not in res.stderr and 'AddressSanitizer' not in res.stderr, res.stderr[-6000:]
  m = re.search(r'coating: (\d+) checks, 0 mismatches', res.stdout)
  assert m and int(m.group(1)) > 10000, res.stdout[-2000:]
