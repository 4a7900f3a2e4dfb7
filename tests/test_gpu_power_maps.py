"""Power-weighted detector maps on the device: the power plane of the in-kernel detector (ODW_TRACE_POWER_HISTOGRAM,
every kernel family) and of the post-hoc binning (odw_hits_bin_power).  A hit weighs rint(power * 2^32) quanta, planes
are uint64 sums: expected planes are computed here with numpy from hit rows (the oracle has no power plane), and
integer planes are compared exactly."""
import copy
import os

import numpy as np
import pytest

import power_scene
from conftest import SCENES, project

pytestmark = pytest.mark.gpu
SEED = 0x0D15EA5E


@pytest.fixture(scope='module')
def tracer(native_lib):
  from freecad.optics_design_workbench_amd.simulation.tracer import Tracer
  tr = Tracer(0)
  yield tr
  tr.close()


@pytest.fixture(scope='module')
def varied():
  sc, lim = power_scene.scene()
  o, d = power_scene.rays(40000)
  return sc, lim, o, d


def _launch(tr, sc, lim, o, d, power, first=0, det=power_scene.DETECTOR, histogram=True):
  tr.setScene(sc)
  tr.setLimits(lim)
  tr.setDetector(det, power=power)
  tr.reserveHits(len(o) * (lim.max_intersections + 1))
  tr.reset()
  tr.traceRays(o, d, first=first, histogram=histogram)
  tr.sync()


@pytest.mark.parametrize('mode', ['off', 'structure'])
def test_plane_equals_the_devices_own_rows(native_lib, varied, mode):
  """one launch with RECORD_HITS | HISTOGRAM | POWER_HISTOGRAM: the power plane is numpy's sum of rint(power * 2^32) over
  the launch's own rows, bin by bin; the count plane, the rows and the counters (HIST_OVERFLOW among them) are those of
  the same launch without the flag -- generic flat kernel and the kernel compiled against the scene"""
  from freecad.optics_design_workbench_amd.simulation.tracer import Tracer
  sc, lim, o, d = varied
  out = {}
  for power in (False, True):
    with Tracer(0) as tr:
      info = tr.compileScene(mode)
      _launch(tr, sc, lim, o, d, power)
      assert tr.compiledInfo()['mode'] == (1 if mode == 'structure' else 0), info
      # (weighted launches run a variant of the compiled kernel of their own: it was built and bound, not replaced by a
      #  generic kernel; launches without the plane never ask for it)
      assert tr.compiledInfo()['power'] == (1 if mode == 'structure' and power else 0), tr.compiledInfo()
      out[power] = (tr.counters(), tr.hits(), tr.histogram(), tr.powerHistogramRaw() if power else None)
  cnt, rows, hist, raw = out[True]
  assert cnt['hits_dropped'] == 0 and len(np.unique(rows['power'])) > 100
  want_counts, want_power, outside = power_scene.planes(rows)
  assert outside > 0 and cnt['hist_overflow'] == outside
  assert np.array_equal(hist, want_counts)
  assert raw.dtype == np.uint64 and np.array_equal(raw, want_power)
  assert not np.array_equal(raw, hist << np.uint64(32))              # (a count map is not a power map here)
  assert cnt == out[False][0]
  assert np.array_equal(hist, out[False][2])
  for col in ('point', 'direction', 'power', 'tag'):
    assert np.array_equal(rows[col], out[False][1][col]), col


def test_power_histogram_is_the_raw_plane_in_source_power(tracer, varied):
  sc, lim, o, d = varied
  _launch(tracer, sc, lim, o[:5000], d[:5000], True)
  raw, real = tracer.powerHistogramRaw(), tracer.powerHistogram()
  assert real.dtype == np.float64 and real.shape == raw.shape == (power_scene.DETECTOR['nx'], power_scene.DETECTOR['ny'])
  assert np.array_equal(real, raw.astype(np.float64) * 2.0 ** -32) and 0 < real.sum() < tracer.histogram().sum()
  tracer.reset()
  assert not tracer.powerHistogramRaw().any() and not tracer.histogram().any()      # (odw_reset_results zeroes the plane)


def _unit_power_case(tr, pr, det, n, compile_mode='off'):
  tr.compileScene(compile_mode)
  tr.setScene(pr.scene)
  tr.setSource(pr.source)
  tr.setLimits(pr.limits)
  tr.setDetector(det, power=True)
  tr.reserveHits(0)
  tr.reset()
  tr.trace(0, n, SEED, record_hits=False)
  tr.sync()
  hist, raw = tr.histogram(), tr.powerHistogramRaw()
  assert hist.sum() > n // 20
  assert np.array_equal(raw, hist << np.uint64(32))
  return hist


def _huge_detector(sc):
  return dict(group=-1, origin=(0.0, 0.0, 0.0), ex=(1.0, 0.0, 0.0), ey=(0.0, 1.0, 0.0), x_lo=-60.0, x_hi=60.0, y_lo=-60.0,
              y_hi=60.0, nx=96, ny=96)


def test_unit_powers_flat_compiled_and_grid(native_lib):
  """every power is 1 on the golden scenes: the power plane is the count plane shifted by 32 bits, exactly -- flat
  generic kernel and compiled kernel (lensesAndMirrors: most hits inside the LDS count window), grid kernel (hugeArray)"""
  from freecad.optics_design_workbench_amd import _native, scenes
  from freecad.optics_design_workbench_amd.simulation.tracer import Tracer
  pr = project('lensesAndMirrors')
  det = scenes.planeDetector(pr.scene, 'OpticalAbsorberGroup', nx=256, ny=256, toward=pr.source.xform[[3, 7, 11]])
  hists = []
  for mode in ('off', 'structure'):
    with Tracer(0) as tr:
      hists.append(_unit_power_case(tr, pr, det, 2_000_000, mode))
      assert tr.compiledInfo()['mode'] == tr.compiledInfo()['power'] == (1 if mode == 'structure' else 0)
  assert np.array_equal(hists[0], hists[1])
  huge = project('hugeArray')
  assert _native.build_check(huge.scene, huge.limits)['structure'] == 'grid'
  sc = copy.copy(huge.scene)
  sc.group_record = np.ones_like(sc.group_record)
  pr2 = copy.copy(huge)
  pr2.scene = sc
  with Tracer(0) as tr:
    _unit_power_case(tr, pr2, _huge_detector(sc), 200_000)


def _ball_lens():
  from freecad.optics_design_workbench_amd.freecad_elements import make, point_source
  from freecad.optics_design_workbench_amd.scene import Document, bake
  doc = Document()
  ball = make.makeTessellated(doc, make.makeSphere(doc, 'S', 5, base=(0, 0, 30)), 64)      # (make.makeMesh of the facets)
  make.makeLens(doc, [ball], RefractiveIndex=1.5)
  make.makeAbsorber(doc, [make.makeBox(doc, 'A', 100, 100, 1, base=(-50, -50, 60))])
  make.makeSimulationSettings(doc)
  src = make.makePointSource(doc, PowerDensity='exp(-theta**2/0.05**2)')

  class Pr:
    scene, limits, source = bake.bakeScene(doc, src), bake.bakeLimits(doc, src), point_source.bakeSource(doc, src)
  return Pr


@pytest.mark.parametrize('mesh_kernel', ['1', '0'])
def test_unit_powers_mesh_and_bvh_kernels(native_lib, monkeypatch, mesh_kernel):
  """a tessellated ball lens: the mesh kernel, and (ODW_MESH_KERNEL=0, as tests/test_mesh.py switches it) the binary-tree
  kernel odw_trace_kernel<true, ...>"""
  from freecad.optics_design_workbench_amd import scenes
  from freecad.optics_design_workbench_amd.simulation.tracer import Tracer
  monkeypatch.setenv('ODW_MESH_KERNEL', mesh_kernel)
  pr = _ball_lens()
  det = scenes.planeDetector(pr.scene, 'OpticalAbsorberGroup', nx=128, ny=128, toward=(0.0, 0.0, 0.0))
  with Tracer(0) as tr:
    _unit_power_case(tr, pr, det, 300_000)


def test_against_the_oracle(tracer, oracle, varied):
  """the same explicit rays through the CPU oracle, its rows binned with numpy: identical count planes; per bin the
  power planes differ by at most n_bin * (1e-9 * 2^32 + 1) quanta -- the project's 1e-9 tolerance on a row's power
  (tests/test_gpu_parity_geometry.py: assert_same) plus one rounding step per hit"""
  sc, lim, o, d = varied
  o, d = o[:12000], d[:12000]
  _launch(tracer, sc, lim, o, d, True)
  counts, raw = tracer.histogram(), tracer.powerHistogramRaw()
  ref = oracle.trace_rays(sc, lim, o, d)['hits']
  want_counts, want_power, _ = power_scene.planes(ref)
  assert np.array_equal(counts, want_counts) and counts.sum() > 12000
  bound = np.ceil(counts.astype(np.float64) * (1e-9 * 2.0 ** 32 + 1)).astype(np.int64)
  diff = np.abs(raw.astype(np.int64) - want_power.astype(np.int64))
  print('largest |dq|', int(diff.max()), 'of allowed', int(bound[np.unravel_index(diff.argmax(), diff.shape)]))
  assert (diff <= bound).all()


def test_shards_add_up_and_the_results_block_grows(native_lib, varied):
  """the raw planes of two disjoint ray ranges, added with numpy, are the plane of one launch over both, exactly
  (integer sums: what `parallel.reduceResults` relies on); `resultsView()` is [counters | bins | power plane] with the
  plane enabled and [counters | bins] without"""
  from freecad.optics_design_workbench_amd.simulation.tracer import Tracer
  sc, lim, o, d = varied
  n, cut = 20000, 7777
  o, d = o[:n], d[:n]
  nb = power_scene.DETECTOR['nx'] * power_scene.DETECTOR['ny']
  with Tracer(0) as tr:
    _launch(tr, sc, lim, o, d, True)
    whole, whole_counts = tr.powerHistogramRaw(), tr.histogram()
    view, off = tr.resultsView()
    assert view.__cuda_array_interface__['shape'] == (off + 2 * nb,)
    assert tr.powerHistogramView().__cuda_array_interface__['shape'] == (nb,)
    assert tr.powerHistogramView().__cuda_array_interface__['data'][0] == view.__cuda_array_interface__['data'][0] + 8 * (off + nb)
    parts, part_counts = np.zeros_like(whole), np.zeros_like(whole_counts)
    for a, b in ((0, cut), (cut, n)):
      _launch(tr, sc, lim, o[a:b], d[a:b], True, first=a)
      parts += tr.powerHistogramRaw()
      part_counts += tr.histogram()
    assert np.array_equal(parts, whole) and np.array_equal(part_counts, whole_counts) and whole.any()
    tr.setDetector(power_scene.DETECTOR)
    view, off = tr.resultsView()
    assert view.__cuda_array_interface__['shape'] == (off + nb,)


def test_auto_mode_compiles_the_power_variant_in_the_background(native_lib, monkeypatch, tmp_path):
  """ODW_COMPILE_AUTO: once the scene's compiled kernel is bound, the first weighted launch starts the compilation of the
  POWER variant on a thread (the structure is hot already), weighted launches run the generic POWER kernel meanwhile and
  a later one takes the compiled variant -- the same planes throughout"""
  import time
  from freecad.optics_design_workbench_amd import scenes
  from freecad.optics_design_workbench_amd.simulation.tracer import Tracer
  monkeypatch.setenv('ODW_KERNEL_CACHE', str(tmp_path / 'kernels'))      # an empty disk cache: real compilations
  monkeypatch.setenv('ODW_SPEC_HOT_RAYS', '150000')
  monkeypatch.setenv('ODW_SPEC_OPTS', '-DODW_TEST_AUTO_POWER=1')         # (a key no other test has loaded)
  pr = project('lensesAndMirrors')
  det = scenes.planeDetector(pr.scene, 'OpticalAbsorberGroup', nx=128, ny=128, toward=pr.source.xform[[3, 7, 11]])
  n = 100000
  with Tracer(0) as tr:
    tr.setScene(pr.scene); tr.setSource(pr.source); tr.setLimits(pr.limits)
    assert tr.compileScene('auto')['mode'] == 0
    tr.reserveHits(0)

    def launch(power):
      tr.setDetector(det, power=power)
      tr.reset()
      tr.trace(0, n, SEED, record_hits=False)
      tr.sync()
      return tr.histogram()
    t0 = time.time()
    ref = launch(False)
    while tr.compiledInfo()['mode'] != 2 and time.time() - t0 < 60:
      time.sleep(0.05)
      assert np.array_equal(launch(False), ref)
    assert tr.compiledInfo()['mode'] == 2 and tr.compiledInfo()['power'] == 0
    seen = []
    t0 = time.time()
    while time.time() - t0 < 60:
      hist = launch(True)
      assert np.array_equal(hist, ref) and np.array_equal(tr.powerHistogramRaw(), ref << np.uint64(32))
      seen.append(tr.compiledInfo()['power'])
      if seen[-1] == 2:
        break
      time.sleep(0.05)
    assert seen[0] == 0 and seen[-1] == 2, seen      # generic POWER kernel while the thread compiles, then the variant
    assert np.array_equal(launch(True), ref) and np.array_equal(tr.powerHistogramRaw(), ref << np.uint64(32))


def _hip():
  import ctypes as C
  hip = C.CDLL('libamdhip64.so')
  hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
  return hip


def test_capacity_a_bin_of_2_to_the_32_hits_is_refused(native_lib, varied):
  """a bin of >= 2^32 hits may hold more than 2^64 quanta: `odw_fetch_power_histogram` returns ODW_ERR_CAPACITY with the
  bin in `odw_last_error` and hands out no plane.  The count plane is seeded through its device view (nobody traces
  4e9 rays here); after `reset()` the fetch succeeds again."""
  import ctypes as C
  from freecad.optics_design_workbench_amd._native import NativeError
  from freecad.optics_design_workbench_amd.simulation.tracer import Tracer
  sc, lim, o, d = varied
  nx, ny = power_scene.DETECTOR['nx'], power_scene.DETECTOR['ny']
  with Tracer(0) as tr:
    _launch(tr, sc, lim, o[:3000], d[:3000], True)
    assert tr.powerHistogramRaw().any()
    k = 5 * ny + 7
    for seed, refused in (((1 << 32) - 1, False), (1 << 32, True)):
      word = np.array([seed], dtype=np.uint64)
      view = tr.histogramView()
      assert view.__cuda_array_interface__['shape'] == (nx * ny,)
      assert _hip().hipMemcpy(view.__cuda_array_interface__['data'][0] + 8 * k, word.ctypes.data, 8, 1) == 0   # (1: host to device)
      assert tr.histogram()[5, 7] == seed
      if not refused:
        assert tr.powerHistogramRaw().any()
        continue
      with pytest.raises(NativeError) as err:
        tr.powerHistogramRaw()
      assert 'capacity' in str(err.value) and f'bin {k} holds {1 << 32} hits' in str(err.value) and 'wrapped' in str(err.value)
      # the entry point itself: the code, and nothing in `out`
      out = np.full(nx * ny, 0xABCD, dtype=np.uint64)
      rc = tr._lib.odw_fetch_power_histogram(tr._ctx, out.ctypes.data_as(C.POINTER(C.c_uint64)), C.c_uint64(nx * ny))
      assert rc == 4 and not out.any()                                 # (ODW_ERR_CAPACITY)
      with pytest.raises(NativeError):
        tr.powerHistogram()
    tr.reset()
    assert not tr.powerHistogramRaw().any()
    tr.traceRays(o[:3000], d[:3000])
    tr.sync()
    assert tr.powerHistogramRaw().any()


def test_device_rounding_of_edge_powers(tracer):
  """the weight of a hit as the DEVICE computes it (power_quanta in csrc/odw_kernels.hip), against the header's
  definition written out as integers: zero, one, negative, NaN, infinities, the clamp at 2^20, half quanta (ties go to
  even), less than half a quantum.  Post hoc the rows are loaded as they are (`Tracer.loadHits` -> `odw_hits_bin_power`);
  in the trace kernels explicit rays carry the powers that survive the power tolerance (`traceRays(..., powers=...)`)"""
  cases = [(0.0, 0), (1.0, 1 << 32), (-1.0, 0), (float('nan'), 0), (float('inf'), 1 << 52), (float('-inf'), 0),
           (2.0 ** 20, 1 << 52), (2.0 ** 21, 1 << 52), (2.0 ** -33, 0), (3 * 2.0 ** -33, 2), (5 * 2.0 ** -33, 2),
           (2.0 ** -34, 0), (3 * 2.0 ** -34, 1), (1 + 2.0 ** -33, 1 << 32), (1 + 3 * 2.0 ** -33, (1 << 32) + 2),
           (0.7 ** 3, 1473173783)]                                      # (0.7^3 * 2^32 = 1473173782.53)
  powers = np.array([c[0] for c in cases])
  want = np.array([c[1] for c in cases], dtype=np.uint64)
  m = len(cases)
  P = np.stack([np.arange(m) + 0.5, np.full(m, 0.5), np.zeros(m)], axis=1)
  D = np.tile([0.0, 0.0, -1.0], (m, 1))
  dh = tracer.loadHits(dict(points=P, directions=D, powers=powers, isEntering=np.ones(m, dtype=int)))
  H = dh.histogram(weights='powers', planeNormal=np.array([0.0, 0.0, 1.0]), xInPlaneVec=np.array([1.0, 0.0, 0.0]),
                   origin=np.zeros(2), bins=[np.arange(m + 1.0), np.array([0.0, 1.0])])
  assert np.array_equal(H.powerQuanta[:, 0], want), (H.powerQuanta[:, 0], want)
  # in the kernels: an absorbing plate under rays that come straight down, one per bin
  sc, lim = power_scene.build([('Absorber', lambda d: [power_scene.make.makeBox(d, 'Plate', 40, 4, 1, base=(-2, -2, -1))], {})])
  keep = [i for i, p in enumerate(powers) if p >= 1e-3]                # (finite or not; NaN and tiny powers end a ray at once)
  o = np.stack([np.array(keep) + 0.5, np.full(len(keep), 0.5), np.full(len(keep), 20.0)], axis=1)
  det = dict(group=-1, origin=(0.0, 0.0, 0.0), ex=(1.0, 0.0, 0.0), ey=(0.0, 1.0, 0.0), x_lo=0.0, x_hi=float(m), y_lo=0.0, y_hi=1.0,
             nx=m, ny=1)
  tracer.setScene(sc); tracer.setLimits(lim); tracer.setDetector(det, power=True)
  tracer.reserveHits(4 * m)
  tracer.reset()
  tracer.traceRays(o, np.tile([0.0, 0.0, -1.0], (len(keep), 1)), powers=powers[keep])
  tracer.sync()
  rows = tracer.hits()
  assert len(rows) == len(keep) and np.array_equal(rows['power'], powers[keep])
  raw = tracer.powerHistogramRaw()[:, 0]
  assert np.array_equal(tracer.histogram()[keep, 0], np.ones(len(keep), dtype=np.uint64))
  assert np.array_equal(raw[keep], want[keep]), (raw[keep], want[keep])


def _device_words(view):
  """the int64 words behind a device view, copied by the HIP runtime the library itself runs on"""
  cai = view.__cuda_array_interface__
  out = np.zeros(cai['shape'][0], dtype=np.int64)
  assert _hip().hipMemcpy(out.ctypes.data, cai['data'][0], out.nbytes, 2) == 0          # (2: hipMemcpyDeviceToHost)
  return out


def test_off_means_off(native_lib, varied):
  """without power=True nothing changes: a context that enabled the plane and switched it off again hands out the
  results block, histogram, rows and counters of a context that never enabled it; the power accessors raise"""
  from freecad.optics_design_workbench_amd.simulation.tracer import Tracer
  sc, lim, o, d = varied
  o, d = o[:15000], d[:15000]
  out = []
  for toggled in (False, True):
    with Tracer(0) as tr:
      if toggled:
        _launch(tr, sc, lim, o[:100], d[:100], True)
        assert tr.powerHistogramRaw().any()
      _launch(tr, sc, lim, o, d, False)
      with pytest.raises(ValueError):
        tr.powerHistogram()
      with pytest.raises(ValueError):
        tr.powerHistogramRaw()
      view, off = tr.resultsView()
      block = _device_words(view)
      out.append((block, off, tr.histogram(), tr.hits(), tr.counters()))
  (b0, off0, h0, r0, c0), (b1, off1, h1, r1, c1) = out
  assert off0 == off1 and b0.shape == b1.shape == (off0 + h0.size,) and np.array_equal(b0, b1)
  assert np.array_equal(b0[off0:].astype(np.uint64).reshape(h0.shape), h0)
  assert np.array_equal(h0, h1) and c0 == c1 and h0.any()
  for col in ('point', 'direction', 'power', 'tag'):
    assert np.array_equal(r0[col], r1[col]), col


def test_enable_needs_a_detector_and_a_launch_flag(native_lib, varied):
  """odw_enable_power_histogram before odw_set_detector is an error; a launch without histogram=True leaves both planes
  alone"""
  import ctypes as C
  from freecad.optics_design_workbench_amd._native import NativeError
  from freecad.optics_design_workbench_amd.simulation.tracer import Tracer
  sc, lim, o, d = varied
  with Tracer(0) as tr:
    with pytest.raises(NativeError):
      tr._chk(tr._lib.odw_enable_power_histogram(tr._ctx, C.c_int(1)), 'odw_enable_power_histogram')
    _launch(tr, sc, lim, o[:2000], d[:2000], True, histogram=False)
    assert not tr.histogram().any() and not tr.powerHistogramRaw().any()


POSTHOC = {'cart24': dict(bins=24), 'cartedges': dict(bins=[np.linspace(-20, 20, 41), np.linspace(-12, 12, 25)]),
           'polar4x30': dict(bins=(4, 30), binCoords='polar'),
           'polaredges': dict(binCoords='polar', bins=[np.linspace(-np.pi, np.pi, 7), np.geomspace(1e-2, 40, 60)])}
PLANE = dict(planeNormal=np.array([0.0, 0.0, 1.0]), xInPlaneVec=np.array([1.0, 0.0, 0.0]))


def _numpy_bins(edges, v):
  """numpy.histogramdd's rule: searchsorted(edges, v, 'right') - 1, the last edge closed; -1: outside"""
  k = np.searchsorted(edges, v, 'right') - 1
  k[v == edges[-1]] = len(edges) - 2
  k[(k < 0) | (k > len(edges) - 2)] = -1
  return k


@pytest.mark.parametrize('kind', list(POSTHOC))
def test_posthoc_power_plane(tracer, varied, kind):
  """`DeviceHits.histogram(weights='powers')` on the rows in HBM: `powerQuanta` is numpy.add.at of rint(power * 2^32)
  over the bins numpy's rule gives for the same edges, exactly; `hist` = powerQuanta * 2^-32 agrees with the host
  `Hits.histogram(weights='powers')` per bin within n_bin * 2^-33 (quantisation) + n_bin * 2^-52 * sum_bin (numpy's
  sequential float sum); the unweighted call is what it was.  (The plane is given, along coordinate axes: the projected
  coordinates are then the points' own, whatever the order of the products.)"""
  sc, lim, o, d = varied
  _launch(tracer, sc, lim, o, d, False)
  kw = POSTHOC[kind]
  dh = tracer.deviceHits(None)
  host = dh.toHits()
  dh = tracer.deviceHits(None)
  H = dh.histogram(weights='powers', **PLANE, **kw)
  C0 = dh.histogram(**PLANE, **kw)
  G = host.histogram(weights='powers', **PLANE, origin=H._origin, bins=[H.binX, H.binY], **{k: v for k, v in kw.items() if k != 'bins'})
  G0 = host.histogram(**PLANE, origin=H._origin, bins=[H.binX, H.binY], **{k: v for k, v in kw.items() if k != 'bins'})
  assert C0.powerQuanta is None and np.array_equal(C0.binX, H.binX) and np.array_equal(C0.binY, H.binY)
  assert H.powerQuanta.dtype == np.uint64 and np.array_equal(H.hist, H.powerQuanta.astype(np.float64) * 2.0 ** -32)
  # numpy's rule on the same edges
  P = host.points()
  X, Y = P[:, 0] - H._origin[0], P[:, 1] - H._origin[1]
  a, b = (np.arctan2(X, Y), np.sqrt(X**2 + Y**2)) if kw.get('binCoords') == 'polar' else (X, Y)      # (histogram.py:47)
  ia, ib = _numpy_bins(H.binX, a), _numpy_bins(H.binY, b)
  ok = (ia >= 0) & (ib >= 0)
  want_q = np.zeros(H.hist.shape, dtype=np.uint64)
  want_n = np.zeros(H.hist.shape, dtype=np.uint64)
  np.add.at(want_q, (ia[ok], ib[ok]), power_scene.quanta(host.hits['powers'][ok]))
  np.add.at(want_n, (ia[ok], ib[ok]), np.uint64(1))
  assert ok.sum() > 20000 and np.array_equal(C0.hist, want_n.astype(np.float64))
  assert np.array_equal(H.powerQuanta, want_q)
  assert np.array_equal(G0.hist, C0.hist)
  bound = want_n.astype(np.float64) * 2.0 ** -33 + want_n.astype(np.float64) * 2.0 ** -52 * G.hist
  print(kind, 'largest |hist - host|', float(np.abs(H.hist - G.hist).max()), 'bound there',
        float(bound[np.unravel_index(np.abs(H.hist - G.hist).argmax(), bound.shape)]))
  assert (np.abs(H.hist - G.hist) <= bound).all()
  with pytest.raises(TypeError):
    dh.histogram(weights=host.hits['powers'], **PLANE, **kw)          # (arrays and other columns: the host route)
  with pytest.raises(TypeError):
    dh.histogram(weights='points', **PLANE, **kw)


def test_run_hits_bins_powers_in_hbm(native_lib, tmp_path):
  """after a runSimulation('true') that kept its rows, `loadHits('*').histogram(weights='powers')` bins them where they are
  (no file is read: `_loaded` stays None) and agrees with the host answer within the post-hoc bound"""
  import shutil
  from freecad.optics_design_workbench_amd.jupyter_utils import FreecadDocument
  from freecad.optics_design_workbench_amd.simulation import results_store
  path = str(tmp_path / 'GettingStarted.FCStd')
  shutil.copy(os.path.join(SCENES, 'GettingStarted.FCStd'), path)
  kw = dict(binCoords='polar', bins=[np.arange(0, 2 * np.pi, np.pi / 2), np.geomspace(1e-3, 5, 200)])
  with FreecadDocument(path) as f:
    f.OpticalSimulationSettings.EndAfterRays = '2e5'
    raw = f.runSimulation('true', raysPerLaunch=70000, keepOnDevice=True)
    lazy = raw.loadHits('*')
    assert isinstance(lazy, results_store.RunHits) and lazy._loaded is None
    H = lazy.histogram(weights='powers', **kw)
    N = lazy.histogram(**kw)
    assert lazy._loaded is None and H.powerQuanta is not None and N.powerQuanta is None
    host = raw.loadHits('*', device=False)
    G = host.histogram(weights='powers', **kw)
    assert np.array_equal(N.hist, host.histogram(**kw).hist) and N.hist.sum() > 0.25 * len(host)      # (the edges cover three quadrants)
    bound = N.hist * 2.0 ** -33 + N.hist * 2.0 ** -52 * G.hist
    assert (np.abs(H.hist - G.hist) <= bound).all() and H.hist.sum() > 0
    # an argument the device route does not take: the arrays, with the same call
    A = lazy.histogram(weights=host.hits['powers'], **kw)
    assert lazy._loaded is not None and np.array_equal(A.hist, G.hist)
  results_store.releaseDeviceRuns()
