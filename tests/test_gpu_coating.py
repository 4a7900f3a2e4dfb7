"""Thin-film coatings on lens groups on the device: the stack's reflectance in the place of the bare one under 'Loss' and
'Split'.

The CPU oracle knows nothing of it.  Geometry is held against the same launch with the modes cleared (bit for bit),
powers against numpy's product of 1 - R from the rows' own directions with R from complex characteristic matrices
(coating_cases.reflectance), and 'Split' against coating_cases' numpy walker, which takes the reflectance as a callable.

Launches with a coating set run the COAT variant of the compiled FRESNEL kernel under compile = 'structure' and the COAT
instantiations of the binary-tree kernel otherwise (`compiledInfo()['fresnel']` says which; segment rows and spectral
launches are the tree's in either mode).  Both give the same rows as bytes."""
import copy

import numpy as np
import pytest

import coating_cases as cc
import fresnel_cases as fc
import power_scene
from freecad.optics_design_workbench_amd import _native
from test_gpu_fresnel import RAY, SEG_RAY, _axis_normals, _both_routes, _expected_powers, _same_bytes, _tiny_power_tol, _tracer

pytestmark = pytest.mark.gpu
SEED = 0xC0A7ED
ENTERING = np.cos(np.radians(np.linspace(0.0, 85.0, 86)))
LEAVING = np.cos(np.radians(np.linspace(0.0, 41.0, 42)))


def _launch(tr, sc, lim, o, d, *, wavelength=550.0, modes='scene', coating='scene', segments=False, wavelengths=None, first=0,
            seed=None, det=None, power=False):
  """one traceRays launch of `sc` at the launch wavelength `wavelength` -> (counters, hit rows, segment rows or None,
  compiledInfo); modes / coating: set after the scene's own (setFresnel clears the coating, so the coating follows)"""
  tr.setScene(sc)
  if modes != 'scene':
    tr.setFresnel(modes)
  if coating != 'scene':
    tr.setCoating(coating)
  tr.setWavelength(wavelength)
  tr.setLimits(lim)
  tr.setDetector(det, power=power) if det is not None else tr.setDetector(None)
  tr.reserveHits(len(o) * 16)
  if segments:
    tr.reserveSegments(len(o) * 16)
  if seed is not None:
    tr.setSurfaceSeed(seed)
  tr.reset()
  tr.traceRays(o, d, first=first, record_segments=segments, wavelengths=wavelengths)
  tr.sync()
  return tr.counters(), tr.hits(), (tr.segments() if segments else None), tr.compiledInfo()


def _coated_factors(rows, group, n_glass, normals, layers, wavelength):
  """1 - R of every row of lens group `group` under the stack `layers` (1 for the rows of other groups, and where the ray
  is totally reflected), from the row's incoming direction, the surface normal `normals` [rows, 3] (any sign), the
  entering bit and the wavelength (one, or one per row)"""
  g = ((rows['tag'] >> np.uint64(48)) & np.uint64(0x7FFF)).astype(np.int64)
  entering = (rows['tag'] >> np.uint64(63)).astype(bool)
  cos_i = np.abs(np.einsum('ij,ij->i', rows['direction'], normals))
  R = np.where(entering, cc.reflectance(1.0, n_glass, cos_i, layers, wavelength, True),
               cc.reflectance(n_glass, 1.0, cos_i, layers, wavelength, False))
  tir = ~entering & (fc.root_of(n_glass, 1.0, cos_i) < 0)
  return np.where((g == group) & ~tir, 1.0 - R, 1.0)


# ---- 5. the reflectance on the device ------------------------------------------------------------------------------------
def test_reflectance_on_the_device(native_lib):
  """the kernel-side function (the kernels' own square roots, sincos of the device library) against the host twin and numpy's
  complex matrices, on the grids of the host test"""
  tr = _tracer()
  try:
    for name, layers in cc.STACKS.items():
      for wl in cc.LINES:
        for n1, n2, cos_i, entering in ((1.0, 1.5, ENTERING, True), (1.5, 1.0, LEAVING, False)):
          host = tr.coatedReflectance(n1, n2, cos_i, layers, wl, entering)
          dev = tr.coatedReflectance(n1, n2, cos_i, layers, wl, entering, device=True)
          ref = cc.reflectance(n1, n2, cos_i, layers, wl, entering)
          print(f'{name} {wl:.0f} nm {n1} -> {n2}: host / device {np.abs(host - dev).max():.3g}, device / numpy {np.abs(dev - ref).max():.3g}')
          assert np.array_equal(host, _native.coated_reflectance(n1, n2, cos_i, layers, wl, entering))
          assert np.abs(host - dev).max() < 1e-12 and np.abs(dev - ref).max() < 1e-12
    # a layer that would hold an evanescent wave: the device's bare reflectance, bit for bit
    cos_i = np.cos(np.radians(np.linspace(56.0, 69.0, 14)))
    assert np.array_equal(tr.coatedReflectance(1.7, 1.6, cos_i, [(1.38, 100.0)], 550.0, device=True),
                          tr.fresnelReflectance(1.7, 1.6, cos_i, device=True))
    # no layers: likewise; total reflection: 1
    assert np.array_equal(tr.coatedReflectance(1.0, 1.5, ENTERING, [], 550.0, device=True), tr.fresnelReflectance(1.0, 1.5, ENTERING, device=True))
    assert np.all(tr.coatedReflectance(1.5, 1.0, np.cos(np.radians([45.0, 60.0, 89.0])), cc.W, 550.0, False, device=True) == 1.0)
  finally:
    tr.close()


# ---- 6. Loss on the slab with Q ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('compile', ['off', 'structure'])
def test_loss_on_planes(native_lib, compile):
  sc, lim, _ = cc.slab('Loss', cc.Q)
  lim = _tiny_power_tol(lim)
  o, d = fc.slab_rays_by_incidence(256)

  def run(compile):
    tr = _tracer(compile)
    try:
      cnt, rows, _, info = _launch(tr, sc, lim, o, d)
      assert info['fresnel'] == (1 if compile == 'structure' else 0), info
      _, _, segs, _ = _launch(tr, sc, lim, o, d, segments=True)
      cnt0, rows0, _, info0 = _launch(tr, sc, lim, o, d, modes=None)
      assert info0['fresnel'] == 0
      _, _, segs0, _ = _launch(tr, sc, lim, o, d, modes=None, segments=True)
    finally:
      tr.close()
    return dict(cnt=cnt, rows=rows, segs=segs, cnt0=cnt0, rows0=rows0, segs0=segs0)

  res = _both_routes('coat-planes', compile, run, segment_rows=True)
  cnt, rows, segs, cnt0, rows0, segs0 = (res[k] for k in ('cnt', 'rows', 'segs', 'cnt0', 'rows0', 'segs0'))
  assert cnt == cnt0 and cnt['died'] == 0 and cnt['traced_rays'] == 256
  assert len(rows) == 4 * 256                            # every ray: top face, bottom face, the back box's two faces
  _same_bytes(rows, rows0, ('point', 'direction', 'tag'))
  _same_bytes(segs, segs0, ('p1', 'p2', 'tag'))
  want = _expected_powers(rows, _coated_factors(rows, fc.G_SLAB, fc.N_GLASS, _axis_normals(rows), cc.Q, 550.0))
  err = np.abs(rows['power'] - want).max()
  print(f'largest power difference {err:.3g}; transmitted {rows["power"].reshape(256, 4)[[0, -1], -1]}')
  assert err < 1e-12
  assert np.all(rows0['power'] == 1.0)
  assert abs(rows['power'][3] - (1.0 - 0.014110458641778) ** 2) < 1e-12        # normal incidence
  assert rows['power'][3] > 0.96 ** 2 + 0.04                                     # ... 97.2 % where the bare slab passes 92.2 %
  # the segment rows' powers: the hit rows' (a segment carries the power at its start, a hit row the power it arrives with)
  seg_ray = (segs['tag'] & SEG_RAY).astype(np.int64)
  assert np.array_equal(seg_ray, np.repeat(np.arange(256), 5))
  assert np.array_equal(segs['power'].reshape(256, 5)[:, :4], rows['power'].reshape(256, 4))
  assert np.array_equal(segs['power'].reshape(256, 5)[:, 4], rows['power'].reshape(256, 4)[:, 3])


# ---- 7. orientation ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('compile', ['off', 'structure'])
def test_orientation(native_lib, compile):
  """V at 450 nm: at the bottom face the ray comes from the glass and meets the layers in reverse.  The factor taken there
  is numpy's 1 - R of the reversed stack met in listed order; at normal incidence R is 0.0075, where the stack met as
  listed -- a forgotten reversal -- would give 0.1716"""
  sc, lim, _ = cc.slab('Loss', cc.V, 450.0)
  lim = _tiny_power_tol(lim)
  o, d = fc.slab_rays_by_incidence(64)

  def run(compile):
    tr = _tracer(compile)
    try:
      cnt, rows, _, info = _launch(tr, sc, lim, o, d, wavelength=450.0)
      assert info['fresnel'] == (1 if compile == 'structure' else 0), info
    finally:
      tr.close()
    return dict(rows=rows)

  rows = _both_routes('coat-orientation', compile, run)['rows']
  assert len(rows) == 4 * 64
  r = rows.reshape(64, 4)
  assert np.all(r['tag'][:, 1] >> np.uint64(63) == 0) and np.all(np.abs(r['point'][:, 1, 2] - 2.0) < 1e-9)     # the bottom face, leaving
  cos_i = np.abs(r['direction'][:, 1, 2])
  taken = 1.0 - r['power'][:, 2] / r['power'][:, 1]
  want = cc.reflectance(fc.N_GLASS, 1.0, cos_i, cc.V[::-1], 450.0, True)
  wrong = cc.reflectance(fc.N_GLASS, 1.0, cos_i, cc.V, 450.0, True)
  print(f'bottom face: largest difference {np.abs(taken - want).max():.3g}; normal incidence R {taken[0]:.6f}, unreversed {wrong[0]:.6f}')
  assert np.abs(taken - want).max() < 1e-12
  assert abs(taken[0] - 0.0075) < 1e-4 and abs(wrong[0] - 0.1716) < 1e-4 and abs(taken[0] - wrong[0]) > 0.1


# ---- 8. wavelength -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('compile', ['off', 'structure'])
def test_wavelength(native_lib, compile):
  """the same 64 rays through W at 450 / 550 / 650 nm: three monochromatic launches (the launch wavelength) and one spectral
  launch with the wavelength per ray (the tree's CHROMA + FRESNEL + COAT kernel in either mode).  The lines differ: at
  normal incidence the back row's power differs pairwise by 1.3e-4, 2.0e-3 and 1.9e-3 (away from it the curves of 450 and
  550 nm cross, so the pairwise bound is asserted on the normal-incidence ray)"""
  sc, lim, _ = cc.slab('Loss', cc.W)
  lim = _tiny_power_tol(lim)
  o, d = fc.slab_rays_by_incidence(64)
  o3, d3, wl3 = np.tile(o, (3, 1)), np.tile(d, (3, 1)), np.repeat(cc.LINES, 64)

  def run(compile):
    tr = _tracer(compile)
    out = {}
    try:
      for wl in cc.LINES:
        cnt, rows, _, info = _launch(tr, sc, lim, o, d, wavelength=wl)
        assert info['fresnel'] == (1 if compile == 'structure' else 0), info
        out[wl] = rows
      cnt, rows, _, info = _launch(tr, sc, lim, o3, d3, wavelength=500.0, wavelengths=wl3)
      assert info['fresnel'] == 0 and info['chroma'] == 0, info          # spectral + Fresnel: the tree
    finally:
      tr.close()
    # (one array: the rows the two routes are compared on)
    return dict(rows=np.concatenate([out[wl] for wl in cc.LINES] + [rows]))

  res = _both_routes('coat-wavelength', compile, run)
  assert len(res['rows']) == 6 * 4 * 64
  mono_rows = {wl: res['rows'][k * 256:(k + 1) * 256] for k, wl in enumerate(cc.LINES)}
  back = {}
  for wl in cc.LINES:
    rows = mono_rows[wl]
    assert len(rows) == 4 * 64
    want = _expected_powers(rows, _coated_factors(rows, fc.G_SLAB, fc.N_GLASS, _axis_normals(rows), cc.W, wl))
    err = np.abs(rows['power'] - want).max()
    print(f'{wl:.0f} nm: largest power difference {err:.3g}')
    assert err < 1e-12
    _same_bytes(rows, mono_rows[450.0], ('point', 'direction', 'tag'))
    back[wl] = rows['power'].reshape(64, 4)[:, 3]
  for a, b in ((450.0, 550.0), (450.0, 650.0), (550.0, 650.0)):
    assert abs(back[a][0] - back[b][0]) > 1e-4, (a, b)
  # the spectral launch: every ray under its own wavelength -- the three monochromatic launches' powers, to rounding
  rows = res['rows'][3 * 256:]
  wl_row = np.repeat(wl3, 4)
  want = _expected_powers(rows, _coated_factors(rows, fc.G_SLAB, fc.N_GLASS, _axis_normals(rows), cc.W, wl_row))
  err = np.abs(rows['power'] - want).max()
  print(f'spectral: largest power difference {err:.3g}')
  assert err < 1e-12
  mono = np.concatenate([mono_rows[wl]['power'] for wl in cc.LINES])
  assert np.abs(rows['power'] - mono).max() < 1e-12


# ---- 9. curved surface ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('compile', ['off', 'structure'])
def test_loss_on_curved_surfaces(native_lib, compile):
  """the normal from the row's point: points lie within 1e-9 mm of the 5 mm sphere, so the normal, and with it cos_i, is off
  by <= 2e-10.  Under Q at 550 nm |dR / dcos_i| <= 0.43 entering (incidences up to 64.2 degrees, rays 4.5 mm off the axis)
  and <= 1.74 leaving (up to 36.9 degrees inside the glass) -- numerical derivatives of the numpy reference; both below the
  bare surface's 0.47 and 1.92 on the same ranges.  Two surfaces: 2e-10 x (0.43 + 1.74) = 4.4e-10 < 1e-8"""
  sc, lim, _ = cc.ball('Loss', cc.Q)
  lim = _tiny_power_tol(lim)
  o, d = fc.ball_rays(512)

  def run(compile):
    tr = _tracer(compile)
    try:
      cnt, rows, _, info = _launch(tr, sc, lim, o, d)
      assert info['fresnel'] == (1 if compile == 'structure' else 0), info
      cnt0, rows0, _, _ = _launch(tr, sc, lim, o, d, modes=None)
    finally:
      tr.close()
    return dict(cnt=cnt, rows=rows, cnt0=cnt0, rows0=rows0)

  res = _both_routes('coat-ball', compile, run)
  cnt, rows, cnt0, rows0 = res['cnt'], res['rows'], res['cnt0'], res['rows0']
  assert cnt == cnt0 and len(rows) == 4 * 512
  _same_bytes(rows, rows0, ('point', 'direction', 'tag'))
  g = ((rows['tag'] >> np.uint64(48)) & np.uint64(0x7FFF)).astype(np.int64)
  on_ball = g == 0
  assert np.abs(np.linalg.norm(rows['point'][on_ball], axis=1) - fc.BALL_R).max() < 1e-9
  normals = np.where(on_ball[:, None], rows['point'] / fc.BALL_R, [0.0, 0.0, 1.0])
  want = _expected_powers(rows, _coated_factors(rows, 0, fc.N_GLASS, normals, cc.Q, 550.0))
  err = np.abs(rows['power'] - want).max()
  print(f'largest power difference {err:.3g}')
  assert err < 1e-8
  assert rows['power'].reshape(512, 4)[:, 3].max() > 0.97            # (the bare ball passes less than 0.93 everywhere)


# ---- 10. Split, ray by ray -----------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def walked(oracle):
  """the numpy walker's segments of the 4096 tilted rays (ray numbers 2^33 + k: both words of the counter are in use)"""
  sc, lim, _ = cc.slab('Split', cc.Q)
  o, d = fc.slab_rays_tilted(4096)
  first = (1 << 33) + 12345

  def R(n1, n2, cos_i, entering):
    return cc.reflectance(n1, n2, [cos_i], cc.Q, 550.0, entering)[0]

  out = [cc.walk_split(o[k], d[k], first + k, SEED, oracle.philox, lim.max_ray_length, R, lim.max_intersections) for k in range(len(o))]
  return sc, lim, o, d, first, out


@pytest.mark.parametrize('compile', ['off', 'structure'])
def test_split_ray_by_ray(native_lib, walked, compile):
  sc, lim, o, d, first, ref = walked

  def run(compile):
    tr = _tracer(compile)
    try:
      cnt, rows, segs, info = _launch(tr, sc, lim, o, d, segments=True, first=first, seed=SEED)
      assert info['mode'] == (1 if compile == 'structure' else 0)
      cnt1, rows1, _, info1 = _launch(tr, sc, lim, o, d, first=first, seed=SEED)
      assert info1['fresnel'] == (1 if compile == 'structure' else 0), info1
    finally:
      tr.close()
    return dict(rows=rows1, segs=segs, cnt_segments=cnt, rows_segments=rows, cnt1=cnt1)

  res = _both_routes('coat-split', compile, run, segment_rows=True)
  cnt, rows, segs, cnt1, rows1 = res['cnt_segments'], res['rows_segments'], res['segs'], res['cnt1'], res['rows']
  assert cnt['capped'] == 0 and cnt['traced_rays'] == 4096 and cnt == cnt1
  _same_bytes(rows, rows1)
  assert np.all(rows['power'] == 1.0) and np.all(segs['power'] == 1.0)           # 'Split' never touches the power
  seg_ray = (segs['tag'] & SEG_RAY).astype(np.int64) - (first & int(SEG_RAY))
  ordinal = ((segs['tag'] >> np.uint64(40)) & np.uint64(0xFFF)).astype(np.int64)
  medium = ((segs['tag'] >> np.uint64(52)) & np.uint64(0xFFF)).astype(np.int64) - 1
  start = np.searchsorted(seg_ray, np.arange(4097))
  left_out, ghosts, worst = 0, 0, 0.0
  for k, (want, margin) in enumerate(ref):
    if margin < 1e-9:
      left_out += 1
      continue
    mine = slice(start[k], start[k + 1])
    assert start[k + 1] - start[k] == len(want), (k, start[k + 1] - start[k], len(want))
    assert np.array_equal(ordinal[mine], np.arange(len(want)))
    p1 = np.array([s[0] for s in want])
    p2 = np.array([s[1] for s in want])
    worst = max(worst, np.abs(segs['p1'][mine] - p1).max(), np.abs(segs['p2'][mine] - p2).max())
    assert np.array_equal(medium[mine], [s[2] for s in want]), k
    ghosts += len(want) != 5
  print(f'{ghosts} rays with a ghost, {left_out} left out, largest endpoint difference {worst:.3g} mm')
  assert worst < 1e-9
  assert left_out <= 1
  assert 50 < ghosts < 300                       # (2 R / (1 + R) of 4096 at R = 1.4 .. 2 %: about 130; bare: about 350 and more)


# ---- 11. Split conserves rays --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('compile', ['off', 'structure'])
def test_split_conserves_rays(native_lib, compile):
  """the collimated beam at 550 nm under Q: the share that never reaches the back box is 2 R / (1 + R) = 0.027828 with
  R = 0.0141105; sigma = sqrt(p (1 - p) / n) = 5.2e-4.  The bare slab gives 0.0769"""
  n = 100000
  sc, lim, src = cc.slab('Split', cc.Q)

  def run(compile):
    tr = _tracer(compile)
    try:
      tr.setScene(sc)
      tr.setSource(src)
      tr.setLimits(lim)
      tr.setDetector(None)
      tr.reserveHits(8 * n)
      tr.reset()
      tr.trace(0, n, SEED)
      tr.sync()
      cnt, rows, info = tr.counters(), tr.hits(), tr.compiledInfo()
    finally:
      tr.close()
    assert info['fresnel'] == (1 if compile == 'structure' else 0), info
    return dict(cnt=cnt, rows=rows)

  res = _both_routes('coat-conserve', compile, run)
  cnt, rows = res['cnt'], res['rows']
  g = ((rows['tag'] >> np.uint64(48)) & np.uint64(0x7FFF)).astype(np.int64)
  entering = (rows['tag'] >> np.uint64(63)).astype(bool)
  front, back = int(((g == fc.G_FRONT) & entering).sum()), int(((g == fc.G_BACK) & entering).sum())
  assert cnt['capped'] == 0 and cnt['traced_rays'] == n
  assert front + back == n
  p, sigma = 0.027828, 5.2e-4
  assert abs(2 * cc.R_Q_550 / (1 + cc.R_Q_550) - p) < 1e-6 and abs(np.sqrt(p * (1 - p) / n) - sigma) < 1e-6
  print(f'front {front}, back {back}: share {front / n:.5f}, expected {p:.5f} +- {sigma:.5f}')
  assert abs(front / n - p) < 5 * sigma


# ---- 12. shards ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('compile', ['off', 'structure'])
def test_shards(native_lib, compile):
  """one launch of 8192 generated rays against two of 4096 over the same ray numbers, Q under 'Split'"""
  sc, lim, src = cc.slab('Split', cc.Q, source=dict(fc.BEAM, PowerDensity='1', FocalLength='0', ThetaDomain='0, 0.5'))
  base = (1 << 34) + 777                                   # (both words of the counter in use)

  def run(compile):
    out = []
    tr = _tracer(compile)
    try:
      tr.setScene(sc)
      tr.setSource(src)
      tr.setLimits(lim)
      tr.setDetector(None)
      tr.reserveHits(8 * 8192)
      for launches in (((0, 8192),), ((0, 4096), (4096, 4096))):
        tr.reset()
        for first, n in launches:
          tr.trace(base + first, n, SEED)
        tr.sync()
        out.append(tr.hits())
        info = tr.compiledInfo()
        assert info['fresnel'] == (1 if compile == 'structure' else 0), info
    finally:
      tr.close()
    return dict(rows=out[0], halves=out[1])

  res = _both_routes('coat-shards', compile, run)
  _same_bytes(res['rows'], res['halves'])
  rows = res['rows']
  assert len(rows) > 4 * 8192 * 0.9
  # there are ghosts among them: rays that meet the front box (behind the source) at all
  g = ((rows['tag'] >> np.uint64(48)) & np.uint64(0x7FFF)).astype(np.int64)
  assert 50 < int(((g == fc.G_FRONT) & (rows['tag'] >> np.uint64(63)).astype(bool)).sum()) < 1000


# ---- 13. the power plane -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('compile', ['off', 'structure'])
def test_power_plane(native_lib, compile):
  det = dict(group=-1, origin=(0.0, 0.0, 0.0), ex=(1.0, 0.0, 0.0), ey=(0.0, 1.0, 0.0), x_lo=-10.0, x_hi=10.0, y_lo=-4.0, y_hi=4.0,
             nx=40, ny=16)
  sc, lim, _ = cc.slab('Loss', cc.Q)
  lim = _tiny_power_tol(lim)
  o, d = fc.slab_rays_by_incidence(256)
  tr = _tracer(compile)
  try:
    cnt, rows, _, info = _launch(tr, sc, lim, o, d, det=det, power=True)
    hist, raw = tr.histogram(), tr.powerHistogramRaw()
    assert info['fresnel'] == (1 if compile == 'structure' else 0), info
  finally:
    tr.close()
  counts, power, outside = power_scene.planes(rows, det)
  assert outside > 0 and cnt['hist_overflow'] == outside
  assert np.array_equal(hist, counts) and np.array_equal(raw, power)
  assert len(np.unique(raw)) > 50                       # (a continuum of powers: the plane saw the losses)
  want = _expected_powers(rows, _coated_factors(rows, fc.G_SLAB, fc.N_GLASS, _axis_normals(rows), cc.Q, 550.0))
  assert np.abs(rows['power'] - want).max() < 1e-12     # ... the coated ones


# ---- 14. nothing moved ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('compile', ['off', 'structure'])
def test_nothing_moved(native_lib, compile):
  sc, lim, _ = fc.slab('Loss', second='Loss')                                   # modes, no coating
  lim = _tiny_power_tol(lim)
  before = copy.copy(sc)
  before.group_coating = None                             # a scene of before this property
  zero = copy.copy(sc)
  zero.group_coating = np.zeros_like(sc.group_coating)
  coated2 = cc.slab('Loss', [], second='Loss', second_coating=cc.Q)[0]          # a coating on the second slab only
  assert coated2.group_coating['n'].tolist() == [0, 0, 0, 1]
  o, d = fc.slab_rays_by_incidence(256)
  o2 = o + [30.0, 0.0, 0.0]                               # the same rays onto the second slab
  oo, dd = np.concatenate([o, o2]), np.concatenate([d, d])

  def run(compile):
    tr = _tracer(compile)
    try:
      _, rows_before, _, info = _launch(tr, before, lim, oo, dd)
      assert info['fresnel'] == (1 if compile == 'structure' else 0), info
      _, rows_zero, _, _ = _launch(tr, zero, lim, oo, dd)
      _, rows_coated2, _, info = _launch(tr, coated2, lim, oo, dd)
      assert info['fresnel'] == (1 if compile == 'structure' else 0), info
      tr.setCoating(None)
      tr.reset()
      tr.traceRays(oo, dd)
      tr.sync()
      rows_cleared = tr.hits()
      # a layer of no thickness on both slabs
      _, rows_thin, _, _ = _launch(tr, sc, lim, oo, dd, coating=[[], [(1.38, 0.0)], [], [(2.0, 0.0)]])
    finally:
      tr.close()
    # (rows: what the two routes are compared on)
    return dict(rows=np.concatenate([rows_coated2, rows_thin]), before=rows_before, zero=rows_zero, cleared=rows_cleared)

  res = _both_routes('coat-moved', compile, run)
  rows_before, rows_zero, rows_cleared = (res[k] for k in ('before', 'zero', 'cleared'))
  assert len(res['rows']) == 2 * len(rows_before)
  rows_coated2, rows_thin = res['rows'][:len(rows_before)], res['rows'][len(rows_before):]
  _same_bytes(rows_zero, rows_before)
  _same_bytes(rows_cleared, rows_before)
  _same_bytes(rows_thin, rows_before, ('point', 'direction', 'tag'))
  assert np.abs(rows_thin['power'] - rows_before['power']).max() < 1e-12
  _same_bytes(rows_coated2, rows_before, ('point', 'direction', 'tag'))
  ray = (rows_coated2['tag'] & RAY).astype(np.int64)
  first_slab = ray < 256
  assert rows_coated2['power'][first_slab].tobytes() == rows_before['power'][first_slab].tobytes()      # the slab without a coating
  assert rows_coated2['power'][~first_slab].reshape(256, 4)[0, 3] > 0.97 > rows_before['power'][~first_slab].reshape(256, 4)[0, 3]


# ---- 15. refusals --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('compile', ['off', 'structure'])
def test_refusals(native_lib, compile):
  sc, lim, src = cc.slab('Loss', cc.Q)
  o, d = fc.slab_rays_by_incidence(64)
  tr = _tracer(compile)
  try:
    tr.setLimits(lim)
    tr.setSource(src)
    # a batch
    with pytest.raises(_native.NativeError, match='setSceneBatch: unsupported: scenes with a (Fresnel mode|coating)'):
      tr.setSceneBatch([sc, sc])
    modeless = copy.copy(sc)
    modeless.group_fresnel = np.zeros_like(sc.group_fresnel)
    with pytest.raises(_native.NativeError, match='setSceneBatch: unsupported: scenes with a coating'):
      tr.setSceneBatch([modeless, modeless])
    tr.setScene(sc)

    def goes_on():
      cnt, rows, _, info = _launch(tr, sc, lim, o, d)
      assert cnt['traced_rays'] == 64 and info['fresnel'] == (1 if compile == 'structure' else 0) and len(rows) == 4 * 64
      assert abs(rows['power'][3] - (1.0 - cc.R_Q_550) ** 2) < 1e-12

    goes_on()
    # a coating on a group without a mode; 5 layers; index 0.9; a negative thickness; another number of groups
    with pytest.raises(_native.NativeError, match='invalid.*group 0: a coating on a group without a Fresnel mode'):
      tr.setCoating([cc.Q, cc.Q, []])
    goes_on()
    with pytest.raises(_native.NativeError, match=r'invalid.*group 1: 5 layers \(a coating has at most 4\)'):
      tr.setCoating([[], [(1.38, 50.0)] * 5, []])
    goes_on()
    with pytest.raises(_native.NativeError, match='invalid.*group 1: layer 0: index 0.9'):
      tr.setCoating([[], [(0.9, 50.0)], []])
    goes_on()
    with pytest.raises(_native.NativeError, match='invalid.*group 1: layer 1: thickness -1 nm'):
      tr.setCoating([[], [(1.38, 50.0), (2.0, -1.0)], []])
    goes_on()
    with pytest.raises(_native.NativeError, match="n_groups is not the scene's"):
      tr.setCoating([[], cc.Q])
    goes_on()
    # (a refused call leaves what the context had: after each, the scene's own coating is in force)
    # a mode cleared takes the coating with it: a coating set then is one without a mode
    tr.setFresnel(None)
    with pytest.raises(_native.NativeError, match='invalid.*group 1: a coating on a group without a Fresnel mode'):
      tr.setCoating([[], cc.Q, []])
    tr.reset()
    tr.traceRays(o, d)
    tr.sync()
    assert np.all(tr.hits()['power'] == 1.0)
  finally:
    tr.close()
