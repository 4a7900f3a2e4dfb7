"""Fresnel reflection at lens surfaces on the device: 'Loss' (power *= 1 - R per crossing) and 'Split' (reflected with
probability R on Philox stream 7).

The CPU oracle knows nothing of it.  Geometry is held against the same launch with the modes cleared (bit for bit: 'Loss'
moves no ray), powers against numpy's product of 1 - R from the rows' own directions (fresnel_cases.reflectance_ab), and
'Split' against a numpy walker over the slab's planes that decides every interaction with `oracle.philox`.

Launches with a mode set run the FRESNEL variant of the compiled kernel under compile = 'structure' and the FRESNEL
instantiations of the binary-tree kernel otherwise (`compiledInfo()['fresnel']` says which; segment rows and spectral
launches are the tree's in either mode).  Both give the same rows as bytes."""
import copy

import numpy as np
import pytest

import fresnel_cases as fc
import power_scene
import spectral_cases as sp
from freecad.optics_design_workbench_amd import _native

pytestmark = pytest.mark.gpu
SEED = 0xF4E57E1
RAY = np.uint64(0xFFFFFFFFFFFF)
SEG_RAY = np.uint64(0xFFFFFFFFFF)
COLS = ('point', 'direction', 'power', 'tag')
_RUNS = {}            # (test, compile mode) -> what that mode's launches gave


def _tracer(compile='off'):
  from freecad.optics_design_workbench_amd.simulation.tracer import Tracer
  tr = Tracer(0)
  tr.compileScene(compile)
  return tr


def _same_bytes(a, b, cols=COLS):
  assert len(a) == len(b)
  for col in cols:
    assert a[col].tobytes() == b[col].tobytes(), col


def _both_routes(key, compile, run, segment_rows=False):
  """run(compile) -> dict with 'rows' (and 'segs'): this compile mode's launches, held as bytes against the other mode's.
  The other mode's launches are made here when its own test has not made them in this process, so the comparison does
  not depend on which tests run, or in which order; each mode's launches are made once."""
  for mode in (compile, 'off' if compile == 'structure' else 'structure'):
    if (key, mode) not in _RUNS:
      _RUNS[(key, mode)] = run(mode)
  mine, other = _RUNS[(key, compile)], _RUNS[(key, 'off' if compile == 'structure' else 'structure')]
  _same_bytes(mine['rows'], other['rows'])
  if segment_rows:
    _same_bytes(mine['segs'], other['segs'], ('p1', 'p2', 'power', 'tag'))
  return mine


def _launch(tr, sc, lim, o, d, *, modes='scene', segments=False, wavelengths=None, first=0, seed=None, det=None, power=False):
  """one traceRays launch of `sc` -> (counters, hit rows, segment rows or None, compiledInfo)"""
  tr.setScene(sc)
  if modes != 'scene':
    tr.setFresnel(modes)
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


def _tiny_power_tol(lim):
  lim = copy.copy(lim)
  lim.power_tol = 1e-12
  return lim


def _lens_factors(rows, group, n_glass, normals):
  """1 - R of every row of lens group `group` (1 for the rows of other groups, and where the ray is totally reflected:
  nothing changes there), from the row's incoming direction, the surface normal `normals` [rows, 3] (any sign) and the
  entering bit"""
  g = ((rows['tag'] >> np.uint64(48)) & np.uint64(0x7FFF)).astype(np.int64)
  entering = (rows['tag'] >> np.uint64(63)).astype(bool)
  cos_i = np.abs(np.einsum('ij,ij->i', rows['direction'], normals))
  n_glass = np.broadcast_to(np.asarray(n_glass, dtype=np.float64), cos_i.shape)
  R = np.where(entering, fc.reflectance_ab(1.0, n_glass, cos_i), fc.reflectance_ab(n_glass, 1.0, cos_i))
  tir = ~entering & (fc.root_of(n_glass, 1.0, cos_i) < 0)
  return np.where((g == group) & ~tir, 1.0 - R, 1.0)


def _expected_powers(rows, factors):
  """power of every row = the product of the factors of the ray's rows before it (rows sorted by ray, bounce)"""
  ray = (rows['tag'] & RAY).astype(np.int64)
  want = np.ones(len(rows))
  for k in range(1, len(rows)):
    if ray[k] == ray[k - 1]:
      want[k] = want[k - 1] * factors[k - 1]
  return want


def _axis_normals(rows):
  """the slab's exact face normal at every row: the axis whose face the point lies on"""
  p = rows['point']
  lo, hi = np.array(fc.SLAB[0]), np.array(fc.SLAB[1])
  dist = np.minimum(np.abs(p - lo), np.abs(p - hi))
  n = np.zeros_like(p)
  n[np.arange(len(p)), np.argmin(dist, axis=1)] = 1.0
  return n


# ---- the reflectance on the device -------------------------------------------------------------------------------------
def test_reflectance_on_the_device(native_lib):
  """the kernel-side function (cos_t from the kernels' own square root) against the host twin and numpy"""
  i = np.radians(np.linspace(0.0, 89.9, 1000))
  tr = _tracer()
  try:
    for n1, n2 in ((1.0, 1.5), (1.5, 1.0), (1.0, 1.9)):
      cos_i = np.cos(i)
      keep = np.abs(fc.root_of(n1, n2, cos_i)) >= 1e-3
      host = tr.fresnelReflectance(n1, n2, cos_i[keep])
      dev = tr.fresnelReflectance(n1, n2, cos_i[keep], device=True)
      print(f'{n1} -> {n2}: host / device {np.abs(host - dev).max():.3g}, device / numpy {np.abs(dev - fc.reflectance(n1, n2, cos_i[keep])).max():.3g}')
      assert np.array_equal(host, _native.fresnel_reflectance(n1, n2, cos_i[keep]))
      assert np.abs(host - dev).max() < 1e-12 and np.abs(dev - fc.reflectance(n1, n2, cos_i[keep])).max() < 1e-12
    assert np.all(tr.fresnelReflectance(1.5, 1.0, np.cos(np.radians([45.0, 60.0, 89.0])), device=True) == 1.0)
  finally:
    tr.close()


# ---- 1. Loss on planes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('compile', ['off', 'structure'])
def test_loss_on_planes(native_lib, compile):
  sc, lim, _ = fc.slab('Loss')
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

  res = _both_routes('planes', compile, run, segment_rows=True)
  cnt, rows, segs, cnt0, rows0, segs0 = (res[k] for k in ('cnt', 'rows', 'segs', 'cnt0', 'rows0', 'segs0'))
  assert cnt == cnt0 and cnt['died'] == 0 and cnt['traced_rays'] == 256
  # every ray: top face, bottom face, the back box's two faces
  assert len(rows) == 4 * 256
  _same_bytes(rows, rows0, ('point', 'direction', 'tag'))
  _same_bytes(segs, segs0, ('p1', 'p2', 'tag'))
  want = _expected_powers(rows, _lens_factors(rows, fc.G_SLAB, fc.N_GLASS, _axis_normals(rows)))
  err = np.abs(rows['power'] - want).max()
  print(f'largest power difference {err:.3g}; transmitted {rows["power"].reshape(256, 4)[[0, -1], -1]}')
  assert err < 1e-12
  assert np.all(rows0['power'] == 1.0) and rows['power'].min() < 0.3            # (85 degrees: most of it reflected, twice)
  assert abs(rows['power'][3] - 0.96 ** 2) < 1e-12                              # normal incidence
  # the segment rows' powers: the hit rows' (a segment carries the power at its start, a hit row the power it arrives with)
  seg_ray = (segs['tag'] & SEG_RAY).astype(np.int64)
  assert np.array_equal(seg_ray, np.repeat(np.arange(256), 5))
  assert np.array_equal(segs['power'].reshape(256, 5)[:, :4], rows['power'].reshape(256, 4))
  assert np.array_equal(segs['power'].reshape(256, 5)[:, 4], rows['power'].reshape(256, 4)[:, 3])


# ---- 2. total reflection keeps its power ---------------------------------------------------------------------------------
@pytest.mark.parametrize('compile', ['off', 'structure'])
def test_total_reflection_keeps_its_power(native_lib, compile):
  sc, lim, _ = fc.slab('Loss')
  lim = _tiny_power_tol(lim)
  o, d = fc.slab_rays_tir(64)

  def run(compile):
    tr = _tracer(compile)
    try:
      cnt, rows, _, info = _launch(tr, sc, lim, o, d)
      assert info['fresnel'] == (1 if compile == 'structure' else 0), info
    finally:
      tr.close()
    return dict(rows=rows)

  rows = _both_routes('tir', compile, run)['rows']
  # top face, side face (total reflection), bottom face, the back box's two faces
  assert len(rows) == 5 * 64
  r = rows.reshape(64, 5)
  assert np.all(np.abs(r['point'][:, 1, 0] - 10.0) < 1e-9) and np.all(np.abs(r['point'][:, 2, 2] - 2.0) < 1e-9)
  cos_side = np.abs(r['direction'][:, 1, 0])
  assert np.all(np.abs(np.degrees(np.arccos(cos_side)) - 54.7356) < 1e-3)
  assert np.all(fc.root_of(fc.N_GLASS, 1.0, cos_side) < -0.49)
  assert np.all(r['power'][:, 2] == r['power'][:, 1])                          # the side face took nothing
  assert np.all(r['direction'][:, 2, 0] < 0)                                     # ... and turned the ray round
  want = _expected_powers(rows, _lens_factors(rows, fc.G_SLAB, fc.N_GLASS, _axis_normals(rows)))
  assert np.abs(rows['power'] - want).max() < 1e-12
  assert np.all(r['power'][:, 1] < 0.92) and np.all(r['power'][:, 3] < r['power'][:, 2])


# ---- 3. Loss on curved surfaces ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('compile', ['off', 'structure'])
def test_loss_on_curved_surfaces(native_lib, compile):
  """the normal from the row's point: points lie within 1e-9 mm of the 5 mm sphere, so the normal is off by <= 2e-10;
  |dR / dcos_i| <= 4 n^2 / sqrt(n^2 - 1) = 8.05 at n = 1.5; two surfaces: 2 x 2e-10 x 8.05 = 3.2e-9 < 1e-8"""
  sc, lim, _ = fc.ball('Loss')
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

  res = _both_routes('ball', compile, run)
  cnt, rows, cnt0, rows0 = res['cnt'], res['rows'], res['cnt0'], res['rows0']
  assert cnt == cnt0 and len(rows) == 4 * 512
  _same_bytes(rows, rows0, ('point', 'direction', 'tag'))
  g = ((rows['tag'] >> np.uint64(48)) & np.uint64(0x7FFF)).astype(np.int64)
  on_ball = g == 0
  assert np.abs(np.linalg.norm(rows['point'][on_ball], axis=1) - fc.BALL_R).max() < 1e-9
  normals = np.where(on_ball[:, None], rows['point'] / fc.BALL_R, [0.0, 0.0, 1.0])
  want = _expected_powers(rows, _lens_factors(rows, 0, fc.N_GLASS, normals))
  err = np.abs(rows['power'] - want).max()
  print(f'largest power difference {err:.3g}')
  assert err < 1e-8
  assert rows['power'].reshape(512, 4)[:, 3].max() < 0.93 and rows['power'].reshape(512, 4)[:, 3].min() < 0.85


# ---- 4. Split, ray by ray ------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def walked(oracle):
  """the numpy walker's segments of the 4096 tilted rays (ray numbers 2^33 + k: both words of the counter are in use)"""
  sc, lim, _ = fc.slab('Split')
  o, d = fc.slab_rays_tilted(4096)
  first = (1 << 33) + 12345
  out = [fc.walk_split(o[k], d[k], first + k, SEED, oracle.philox, lim.max_ray_length, lim.max_intersections) for k in range(len(o))]
  return sc, lim, o, d, first, out


@pytest.mark.parametrize('compile', ['off', 'structure'])
def test_split_ray_by_ray(native_lib, walked, compile):
  sc, lim, o, d, first, ref = walked

  def run(compile):
    tr = _tracer(compile)
    try:
      cnt, rows, segs, info = _launch(tr, sc, lim, o, d, segments=True, first=first, seed=SEED)
      assert info['mode'] == (1 if compile == 'structure' else 0)
      # (segment rows are the tree's in either mode: the compiled variant runs the launch without them)
      cnt1, rows1, _, info1 = _launch(tr, sc, lim, o, d, first=first, seed=SEED)
      assert info1['fresnel'] == (1 if compile == 'structure' else 0), info1
    finally:
      tr.close()
    return dict(cnt=cnt, rows=rows1, segs=segs, cnt_segments=cnt, rows_segments=rows, cnt1=cnt1)

  res = _both_routes('split', compile, run, segment_rows=True)
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
  assert 300 < ghosts < 1200                     # (2 R / (1 + R) of 4096 at R = 4 .. 5 %: about 350, more at 40 degrees)


# ---- 5. Split conserves rays ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('compile', ['off', 'structure'])
def test_split_conserves_rays(native_lib, compile):
  """a ray leaves the slab to the back with probability T / (1 - R^2) ... = (1 - R) / (1 + R): the share that never
  reaches the back box is 2 R / (1 + R), R = 0.04"""
  n = 100000
  sc, lim, src = fc.slab('Split')

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

  res = _both_routes('conserve', compile, run)
  cnt, rows = res['cnt'], res['rows']
  g = ((rows['tag'] >> np.uint64(48)) & np.uint64(0x7FFF)).astype(np.int64)
  entering = (rows['tag'] >> np.uint64(63)).astype(bool)
  front, back = int(((g == fc.G_FRONT) & entering).sum()), int(((g == fc.G_BACK) & entering).sum())
  assert cnt['capped'] == 0 and cnt['traced_rays'] == n
  assert front + back == n
  R = 0.04
  p = 2 * R / (1 + R)
  sigma = np.sqrt(p * (1 - p) / n)
  print(f'front {front}, back {back}: share {front / n:.5f}, expected {p:.5f} +- {sigma:.5f}')
  assert abs(front / n - p) < 5 * sigma


# ---- 6. shards -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('compile', ['off', 'structure'])
def test_shards(native_lib, compile):
  """one launch of 8192 generated rays against two of 4096 over the same ray numbers: a ghost is keyed by the ray's number
  in the stream, not by its place in a launch -- on the tree and on the compiled variant, which generates its rays from
  the source compiled into it"""
  sc, lim, src = fc.slab('Split', source=dict(fc.BEAM, PowerDensity='1', FocalLength='0', ThetaDomain='0, 0.5'))
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

  res = _both_routes('shards', compile, run)
  _same_bytes(res['rows'], res['halves'])
  rows = res['rows']
  assert len(rows) > 4 * 8192 * 0.9
  # there are ghosts among them: rays that meet the front box (behind the source) at all
  g = ((rows['tag'] >> np.uint64(48)) & np.uint64(0x7FFF)).astype(np.int64)
  assert 100 < int(((g == fc.G_FRONT) & (rows['tag'] >> np.uint64(63)).astype(bool)).sum()) < 2000


# ---- 7. spectral plus Fresnel --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('compile', ['off', 'structure'])
def test_spectral_plus_loss(native_lib, compile):
  """'Loss' with a wavelength per ray (the tree's CHROMA + FRESNEL kernel in either mode), n(lambda) from
  Tracer.refractiveIndex.
  The prism (a Cauchy glass that does not absorb): both crossings count -- entering, n2 = n(lambda) of the group met;
  leaving, n1 = n(lambda) of the medium.  Its faces are planes with exact normals: the project's 1e-12.
  The singlet absorbs (AbsorptionLength 200 mm): the power at its second surface is ASSIGNED exp(-t / L) there, which
  overwrites the first surface's factor -- the rule this feature keeps -- so the row behind the lens holds the plain
  launch's power times 1 - R of the second surface alone.  Tolerance as on the ball (1e-8): the normal comes from the
  row's point on a 50 mm sphere."""
  sc, lim, _ = fc.singlet('Loss', prism='Loss')
  lim = _tiny_power_tol(lim)
  so, sd = sp.singlet_rays(33)
  po, pd = sp.prism_rays(16)
  o, d = np.concatenate([np.tile(so, (3, 1)), np.tile(po, (3, 1))]), np.concatenate([np.tile(sd, (3, 1)), np.tile(pd, (3, 1))])
  wl = np.concatenate([np.repeat(sp.LINES, 33), np.repeat(sp.LINES, 16)])
  tr = _tracer(compile)
  try:
    cnt, rows, _, info = _launch(tr, sc, lim, o, d, wavelengths=wl)
    # a launch that is both spectral and Fresnel binds neither variant of the compiled kernel: it walks the tree
    assert info['fresnel'] == 0 and info['chroma'] == 0 and info['mode'] == (1 if compile == 'structure' else 0), info
    n_singlet, n_prism = tr.refractiveIndex(0, wl[:99]), tr.refractiveIndex(1, wl[99:])
    cnt0, rows0, _, _ = _launch(tr, sc, lim, o, d, modes=None, wavelengths=wl)
  finally:
    tr.close()
  assert cnt == cnt0 and len(rows) == 3 * (99 + 48)      # two surfaces and the absorbing detector, for every ray
  _same_bytes(rows, rows0, ('point', 'direction', 'tag'))
  assert len(np.unique(n_singlet)) == 3 and len(np.unique(n_prism)) == 3
  # ---- the prism: the face z = 0, and the face through the apex edge turned by -120 degrees about y
  r = rows[3 * 99:].reshape(48, 3)
  assert np.all(r['tag'][:, 0] >> np.uint64(63) == 1) and np.all(r['tag'][:, 1] >> np.uint64(63) == 0)
  a = np.radians(-120.0)
  n_out = np.array([np.sin(a), 0.0, np.cos(a)])
  assert np.abs(r['point'][:, 0, 2]).max() < 1e-9
  assert np.abs((r['point'][:, 1] - [sp.PRISM_X, 0.0, 0.0]) @ n_out).max() < 1e-9      # the second row lies on that face
  R_in = fc.reflectance_ab(1.0, n_prism, np.abs(r['direction'][:, 0, 2]))
  R_out = fc.reflectance_ab(n_prism, 1.0, np.abs(r['direction'][:, 1] @ n_out))
  assert np.all(r['power'][:, 0] == 1.0)
  err_in = np.abs(r['power'][:, 1] - (1.0 - R_in)).max()
  err_out = np.abs(r['power'][:, 2] - (1.0 - R_in) * (1.0 - R_out)).max()
  print(f'prism: largest power difference behind the first face {err_in:.3g}, behind the second {err_out:.3g}')
  assert err_in < 1e-12 and err_out < 1e-12
  assert np.abs(R_in[:16] - R_in[32:]).min() > 1e-5 and np.abs(R_out[:16] - R_out[32:]).min() > 1e-5     # F against C
  # ---- the singlet
  r, r0 = rows[:3 * 99].reshape(99, 3), rows0[:3 * 99].reshape(99, 3)
  centre = np.where(r['point'][:, :, 2:3] < 3.0, [0.0, 0.0, 50.0], [0.0, 0.0, -44.0])[:, :2]
  normal = (r['point'][:, :2] - centre) / 50.0
  assert np.abs(np.linalg.norm(normal, axis=2) - 1.0).max() < 1e-9
  cos_i = np.abs(np.einsum('ijk,ijk->ij', r['direction'][:, :2], normal))
  R2 = fc.reflectance_ab(n_singlet, 1.0, cos_i[:, 1])
  assert np.all(r['power'][:, 0] == 1.0) and np.array_equal(r['power'][:, 1], r0['power'][:, 1])
  err = np.abs(r['power'][:, 2] - r0['power'][:, 2] * (1.0 - R2)).max()
  print(f'singlet: largest power difference {err:.3g}')
  assert err < 1e-8
  # the lines differ: the same ray loses a different share at F and at C
  assert np.abs(R2[:33] - R2[66:]).min() > 1e-5


# ---- 8. the power plane --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('compile', ['off', 'structure'])
def test_power_plane(native_lib, compile):
  det = dict(group=-1, origin=(0.0, 0.0, 0.0), ex=(1.0, 0.0, 0.0), ey=(0.0, 1.0, 0.0), x_lo=-10.0, x_hi=10.0, y_lo=-4.0, y_hi=4.0,
             nx=40, ny=16)
  sc, lim, _ = fc.slab('Loss')
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


# ---- 9. nothing moved ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('compile', ['off', 'structure'])
def test_nothing_moved(native_lib, compile):
  sc, lim, _ = fc.slab('', second='Loss')
  lim = _tiny_power_tol(lim)
  plain = copy.copy(sc)
  plain.group_fresnel = None                              # a scene of before this property
  none = copy.copy(sc)
  none.group_fresnel = np.zeros_like(sc.group_fresnel)
  o, d = fc.slab_rays_by_incidence(256)
  o2 = o + [30.0, 0.0, 0.0]                               # the same rays onto the second slab
  oo, dd = np.concatenate([o, o2]), np.concatenate([d, d])

  def run(compile):
    tr = _tracer(compile)
    try:
      _, rows_plain, _, info = _launch(tr, plain, lim, oo, dd)
      assert info['fresnel'] == 0
      _, rows_none, _, info = _launch(tr, none, lim, oo, dd)
      assert info['fresnel'] == 0
      _, rows_mixed, _, info = _launch(tr, sc, lim, oo, dd)
      assert info['fresnel'] == (1 if compile == 'structure' else 0), info
      tr.setFresnel(None)
      tr.reset()
      tr.traceRays(oo, dd)
      tr.sync()
      rows_cleared, info = tr.hits(), tr.compiledInfo()
      assert info['fresnel'] == 0
    finally:
      tr.close()
    return dict(rows=rows_mixed, plain=rows_plain, none=rows_none, cleared=rows_cleared)

  res = _both_routes('mixed', compile, run)
  rows_mixed, rows_plain, rows_none, rows_cleared = res['rows'], res['plain'], res['none'], res['cleared']
  _same_bytes(rows_none, rows_plain)
  _same_bytes(rows_cleared, rows_plain)
  _same_bytes(rows_mixed, rows_plain, ('point', 'direction', 'tag'))
  ray = (rows_mixed['tag'] & RAY).astype(np.int64)
  first_slab = ray < 256
  assert np.all(rows_mixed['power'][first_slab] == 1.0)                          # the group without a mode keeps its powers
  assert rows_mixed['power'][~first_slab].min() < 0.3


# ---- 10. refusals --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('compile', ['off', 'structure'])
def test_refusals(native_lib, compile):
  from freecad.optics_design_workbench_amd.freecad_elements import make
  from freecad.optics_design_workbench_amd.scene import bake
  sc, lim, src = fc.slab('Split')
  o, d = fc.slab_rays_by_incidence(64)
  tr = _tracer(compile)
  try:
    tr.setLimits(lim)
    tr.setSource(src)
    # batches: scenes that carry a mode; an upload while a mode is set; a mode set on an uploaded batch
    with pytest.raises(_native.NativeError, match='setSceneBatch: unsupported: scenes with a Fresnel mode'):
      tr.setSceneBatch([sc, sc])
    plain = copy.copy(sc)
    plain.group_fresnel = np.zeros_like(sc.group_fresnel)
    tr.setScene(sc)
    with pytest.raises(_native.NativeError, match='unsupported.*odw_upload_scene_batch: a batch with a Fresnel mode set'):
      tr.setSceneBatch([plain, plain])
    tr.setFresnel(None)
    tr.setSceneBatch([plain, plain])
    tr.setFresnel(sc.group_fresnel)
    tr.reset()
    with pytest.raises(_native.NativeError, match='unsupported.*odw_trace_batch: a batch with a Fresnel mode set'):
      tr.traceBatch(0, 64, SEED, 1024)
    tr.setFresnel(None)
    tr.traceBatch(0, 64, SEED, 1024)                        # (cleared: the batch runs)
    tr.sync()
    # a non-lens group; an unknown mode
    tr.setScene(plain)
    with pytest.raises(_native.NativeError, match='invalid.*group 0: a Fresnel mode on a group that is not a lens'):
      tr.setFresnel([1, 1, 0])
    with pytest.raises(_native.NativeError, match='invalid.*group 1: unknown Fresnel mode 3'):
      tr.setFresnel([0, 3, 0])
    with pytest.raises(_native.NativeError, match="n_groups is not the scene's"):
      tr.setFresnel([0, 1])
    # a sequence with 'Split' ('Loss' is allowed)
    seq = copy.copy(sc)
    seq.seq_enabled = 1
    seq.seq_mask = np.full(8, (1 << sc.n_groups) - 1, dtype=np.uint64)
    tr.setScene(seq)
    tr.reserveHits(4096)
    with pytest.raises(_native.NativeError, match="unsupported.*'Split' in a scene with a tracing sequence"):
      tr.traceRays(o, d)
    tr.setFresnel(['', 'Loss', ''])
    tr.reset()
    tr.traceRays(o, d)
    tr.sync()
    assert tr.counters()['traced_rays'] == 64
    # stochastic surfaces
    doc = fc.slab_document('Loss', RefractedProbabilityDensity='exp(-(theta-theta_refl)^2/1e-4)')
    make.makeSimulationSettings(doc)
    rough = bake.bakeScene(doc, make.makePointSource(doc))
    assert len(rough.surface_samplers) > 0
    tr.setScene(rough)
    with pytest.raises(_native.NativeError, match='unsupported.*Fresnel launch: scenes with stochastic surfaces'):
      tr.traceRays(o, d)
    # ... and the context goes on: the next launch of a scene that is in order
    cnt, rows, _, info = _launch(tr, sc, lim, o, d, seed=SEED)
    assert cnt['traced_rays'] == 64 and info['fresnel'] == (1 if compile == 'structure' else 0) and len(rows) >= 2 * 64
  finally:
    tr.close()
