"""Device tracer: the accelerated region of runSimulationIteration.

In the reference `GenericSourceProxy.runSimulationIteration`
(freecad_elements/generic_source.py:51-146) generates RaysPerIteration rays and
walks `ray.traceRay(store=store)` for each; here one `Tracer.trace(first, n,
seed)` call does that for n rays on the GPU through the C-ABI and leaves hit
rows, counters and the detector histogram in HBM until they are fetched.
"""
import atexit
import ctypes as C
import weakref

import numpy as np

from .. import _native
from .._native import (CNT_NAMES, HIT_DTYPE, POWER_QUANTUM_BITS, SEGMENT_DTYPE, TRACE_BAND_HISTOGRAM, TRACE_HISTOGRAM, TRACE_POWER_HISTOGRAM,
                       TRACE_RECORD_HITS, TRACE_RECORD_SEGMENTS)


# Contexts that are still open when the interpreter ends are closed in ITS order, at the start of its shutdown (atexit),
# while the HIP runtime and every module are whole -- not whenever the garbage collector reaches their Tracer during
# module teardown
_LIVE = weakref.WeakSet()


@atexit.register
def _close_live_tracers():
  for t in list(_LIVE):
    try:
      t.close()
    except Exception:
      pass


class _CudaArrayView:
  """zero-copy view of a device buffer for torch.as_tensor (RCCL reductions)"""

  def __init__(self, ptr, n, typestr, owner):
    self.__cuda_array_interface__ = dict(shape=(int(n),), typestr=typestr, data=(int(ptr), False),
                                         version=2, strides=None)
    self._owner = owner


class _PinnedPool:
  """page-locked host memory for the arrays a launch hands over (Tracer.hitColumns): the copy engine writes
  into them directly (48 - 56 GB/s; 17 GB/s through the staging copies of pageable memory).  One pool per
  process: the arrays may outlive the tracer that filled them (a run's results kept in memory).  A slab goes
  back to the pool when the last array carved from it is garbage-collected (the run loop's arrays: once the
  writer threads have pickled them), so a continuous run cycles through as many slabs as it has launches in flight
  between the device and the files (writer threads + their queue + the fetch under way: `reserve` tells the pool; with
  fewer slabs kept than that, every launch page-locks a new 300 MB slab and gives one back -- 50 - 100 ms each, which is
  why MORE writer threads made round 4's run loop SLOWER: 4 / 6 / 8 / 12 writers = 2.9 / 2.1 / 1.7 / 1.2e8 rays/s);
  arrays that are kept keep their slab and the pool allocates another; free slabs beyond KEEP are given back to the
  system.  Page-locking costs 0.22 ms per MB on the pool's boxes (67 ms for a launch's 300 MB slab, 55 ms to give it
  back: scripts/bench_pinned_alloc.py) -- fifteen times what the launch itself may take at 5e8 rays/s --, so the slabs stay
  with the process between runs (a second run starts warm); `releasePinnedMemory()` gives them back."""
  KEEP = 4

  def __init__(self):
    import threading
    self._free = []           # (bytes, address)
    self._lock = threading.Lock()

  def _release(self, nbytes, addr):
    drop = None
    with self._lock:
      self._free.append((nbytes, addr))
      if len(self._free) > self.KEEP:
        drop = self._free.pop(0)
    if drop is not None:
      try:
        _native.lib().odw_host_free(None, C.c_void_p(drop[1]))
      except Exception:
        pass

  def reserve(self, slabs):
    """free slabs the pool holds on to from now on (a run's pipeline depth)"""
    self.KEEP = max(4, int(slabs))

  def trim(self, keep=2):
    """after a run: give free slabs beyond `keep` back to the system"""
    self.KEEP = max(int(keep), 0)
    while True:
      with self._lock:
        if len(self._free) <= self.KEEP:
          break
        drop = self._free.pop(0)
      try:
        _native.lib().odw_host_free(None, C.c_void_p(drop[1]))
      except Exception:
        pass
    self.KEEP = 4

  def take(self, tracer, nbytes):
    """a ctypes buffer of >= nbytes page-locked bytes; numpy arrays made from it (np.frombuffer) keep it alive"""
    import weakref
    nbytes = max(int(nbytes), 4096)
    size = addr = None
    with self._lock:
      fit = [k for k, (b, _) in enumerate(self._free) if nbytes <= b <= 2 * nbytes + (1 << 20)]
      if fit:
        size, addr = self._free.pop(min(fit, key=lambda k: self._free[k][0]))
    if addr is None:
      size = (nbytes + (1 << 20) - 1) & ~((1 << 20) - 1)
      p = C.c_void_p()
      tracer._chk(tracer._lib.odw_host_alloc(tracer._ctx, C.c_uint64(size), C.byref(p)), 'odw_host_alloc')
      addr = p.value
    buf = (C.c_char * size).from_address(addr)
    weakref.finalize(buf, self._release, size, addr)
    return buf


_POOL = _PinnedPool()


def releasePinnedMemory(keep=0):
  """give the page-locked slabs the run loops of this process keep for their next run back to the system"""
  _POOL.trim(keep)


_MONO = ('mono', 'the rows come from monochromatic launches (no spectrum bound, no wavelengths given)')


class Tracer:

  def __init__(self, device=0, referenceStrict=None):
    """referenceStrict: upload scenes without ODW_FLAG_CONVEX, i.e. without the convex-solid skip
    (include/odw_trace.h): every solid of every relevant group is a candidate of every segment, as in
    findNearestIntersection (ray.py:328-364).  Default (None): the environment variable ODW_STRICT, else
    off.  The skip changes results only for rays that leave a convex solid within ~distTol of one of its
    edges (0 of 1e6 rays at DistanceTolerance 1e-6, 2.5e-4 - 5.7e-4 of the rays of the
    two reference scenes with DistanceTolerance 1e-2) and buys 6 % on lensesAndMirrors."""
    import os
    if referenceStrict is None:
      referenceStrict = os.environ.get('ODW_STRICT', '') not in ('', '0')
    self.referenceStrict = bool(referenceStrict)
    self._lib = _native.lib()
    self._ctx = C.c_void_p()
    self.device = int(device)
    _native.check(None, self._lib.odw_create(self.device, C.byref(self._ctx)), 'odw_create')
    _LIVE.add(self)
    self._det = None
    self._power = False
    self._bands = None
    self._keep = {}
    self._spectral = False        # a spectrum is bound (setSpectrum): trace() is a spectral launch
    self._prov = self._archiveProv = None
    self._archiveOn = self._batchOn = False
    # ODW_COMPILE=structure: every tracer of the process compiles its scenes (test campaigns)
    if os.environ.get('ODW_COMPILE'):
      self.compileScene(os.environ['ODW_COMPILE'])

  # -- lifecycle ------------------------------------------------------------
  def close(self):
    for extra in getattr(self, '_sweepLanes', None) or []:      # (contexts a parameter sweep keeps beside this one)
      extra.close()
    self._sweepLanes = []
    if self._ctx:
      for p in getattr(self, '_pinned', []):
        self._lib.odw_host_free(self._ctx, p)
      self._pinned = []
      self._lib.odw_destroy(self._ctx)
      self._ctx = C.c_void_p()

  def __del__(self):
    try:
      self.close()
    except Exception:
      pass

  def __enter__(self):
    return self

  def __exit__(self, *a):
    self.close()

  def _chk(self, rc, what):
    _native.check(self._ctx, rc, what)

  # -- uploads --------------------------------------------------------------
  def setScene(self, scene):
    if self.referenceStrict:
      import copy
      stripped = copy.copy(scene)
      stripped.prim_flags = np.asarray(scene.prim_flags, dtype=np.int32) & ~np.int32(_native.FLAG_CONVEX)
      d, keep = _native.scene_desc(stripped)
    else:
      d, keep = _native.scene_desc(scene)
    self._chk(self._lib.odw_upload_scene(self._ctx, C.byref(d)), 'odw_upload_scene')
    arr, n, keep = _native.surface_sampler_descs(getattr(scene, 'surface_samplers', None))
    self._chk(self._lib.odw_upload_surface_samplers(self._ctx, arr, C.c_int32(n)), 'odw_upload_surface_samplers')
    self.scene = scene
    # (odw_upload_scene has cleared the previous scene's dispersion: what this one carries, if anything)
    kind = getattr(scene, 'group_disp_kind', None)
    if kind is not None and np.any(np.asarray(kind) != 0):
      self.setDispersion(kind, scene.group_disp)
    # (... and its Fresnel modes)
    mode = getattr(scene, 'group_fresnel', None)
    if mode is not None and np.any(np.asarray(mode) != 0):
      self.setFresnel(mode)
    # (... and its coatings, which belong to the modes)
    coating = getattr(scene, 'group_coating', None)
    if coating is not None and np.any(_native.coating_tables(coating)[0] != 0):
      self.setCoating(coating)

  def setCoating(self, coating):
    """Thin-film coatings of the uploaded scene's groups (`odw_set_coating`), after setFresnel: one list of (index,
    thickness_nm) per group, from the outside inwards, at most four layers (or the bake's group_coating).  Groups with a
    Fresnel mode only.  The stack's reflectance takes the bare one's place at every face of the group.  None or an empty
    list clears it, and so do setFresnel and setScene."""
    pi, pd = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    f = self._lib.odw_set_coating
    f.argtypes = [C.c_void_p, C.c_int32, pi, pd]
    if coating is None or len(coating) == 0:
      self._chk(f(self._ctx, 0, None, None), 'odw_set_coating')
      return
    cnt, lay = _native.coating_tables(coating)
    self._chk(f(self._ctx, len(cnt), cnt.ctypes.data_as(pi), lay.ctypes.data_as(pd)), 'odw_set_coating')

  def coatedReflectance(self, n1, n2, cos_i, layers, wavelength_nm, entering=True, device=False):
    """unpolarised reflectance of a surface from index n1 to n2 under the stack `layers` ((index, thickness_nm) from the
    outside inwards; entering: the ray meets them in that order) at the cosines of incidence cos_i and wavelength_nm
    (`odw_coated_reflectance`); device=True: evaluated by the kernel-side function"""
    c = np.ascontiguousarray(cos_i, dtype=np.float64).reshape(-1)
    lay = np.ascontiguousarray(layers, dtype=np.float64).reshape(-1, 2) if len(layers) else np.zeros((0, 2))
    out = np.empty(len(c), np.float64)
    pd = C.POINTER(C.c_double)
    f = self._lib.odw_coated_reflectance
    f.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_int32, C.c_int32, pd, C.c_double, C.c_uint64, pd, pd, C.c_int32]
    self._chk(f(self._ctx, float(n1), float(n2), 1 if entering else 0, len(lay), lay.ctypes.data_as(pd) if len(lay) else None,
                float(wavelength_nm), len(c), c.ctypes.data_as(pd), out.ctypes.data_as(pd), 1 if device else 0),
              'odw_coated_reflectance')
    return out

  def setFresnel(self, mode):
    """Fresnel modes of the uploaded scene's groups (`odw_set_fresnel`): mode [G] of 0 / '' (none), 1 / 'Loss'
    (power *= 1 - R at every crossing of the group's surfaces), 2 / 'Split' (reflected with probability R, decided on a
    Philox stream of its own).  Lens groups only.  None or an empty mode clears it.  Launches with a mode set run the
    compiled kernel's FRESNEL variant under compileScene('structure') (compiledInfo()['fresnel']), else the binary tree."""
    pi = C.POINTER(C.c_int32)
    if mode is None or len(mode) == 0:
      self._chk(self._lib.odw_set_fresnel(self._ctx, C.c_int32(0), None), 'odw_set_fresnel')
      return
    m = np.ascontiguousarray([_native.FRESNEL_MODES[v] if (v is None or isinstance(v, str)) else int(v) for v in mode], dtype=np.int32)
    self._chk(self._lib.odw_set_fresnel(self._ctx, C.c_int32(len(m)), m.ctypes.data_as(pi)), 'odw_set_fresnel')

  def fresnelReflectance(self, n1, n2, cos_i, device=False):
    """unpolarised reflectance of a surface from index n1 to n2 at the cosines of incidence cos_i
    (`odw_fresnel_reflectance`); device=True: evaluated by the kernel-side function"""
    c = np.ascontiguousarray(cos_i, dtype=np.float64).reshape(-1)
    out = np.empty(len(c), np.float64)
    pd = C.POINTER(C.c_double)
    f = self._lib.odw_fresnel_reflectance
    f.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_uint64, pd, pd, C.c_int32]
    self._chk(f(self._ctx, float(n1), float(n2), len(c), c.ctypes.data_as(pd), out.ctypes.data_as(pd), 1 if device else 0),
              'odw_fresnel_reflectance')
    return out

  def setDispersion(self, kind, coef=None):
    """Dispersion of the uploaded scene's groups (`odw_set_dispersion`): kind [G] (0 constant, 1 Sellmeier, 2 Cauchy),
    coef [G, 6] (Sellmeier B1 B2 B3 C1 C2 C3 with C in um^2; Cauchy A B C).  None or an empty kind clears it.
    Monochromatic launches trace the glasses at the launch wavelength (folded into the tables on the host: every
    kernel, today's speed); spectral launches (setSpectrum, traceRays(wavelengths=)) evaluate them per interaction."""
    pi = C.POINTER(C.c_int32)
    pd = C.POINTER(C.c_double)
    if kind is None or len(kind) == 0:
      self._chk(self._lib.odw_set_dispersion(self._ctx, C.c_int32(0), None, None), 'odw_set_dispersion')
      return
    k = np.ascontiguousarray(kind, dtype=np.int32)
    c = np.ascontiguousarray(coef, dtype=np.float64).reshape(len(k), _native.DISP_COEFS)
    self._chk(self._lib.odw_set_dispersion(self._ctx, C.c_int32(len(k)), k.ctypes.data_as(pi), c.ctypes.data_as(pd)),
              'odw_set_dispersion')

  def setSpectrum(self, spectrum):
    """Spectrum of the uploaded point source (`odw_set_spectrum`): a `freecad_elements.point_source.BakedSpectrum`
    (mode 'lines' / 'density', wavelengths, cdf) or None (clears it).  With one bound, trace() is a spectral launch."""
    pd = C.POINTER(C.c_double)
    if spectrum is None:
      self._chk(self._lib.odw_set_spectrum(self._ctx, C.c_int32(0), C.c_int32(0), None, None), 'odw_set_spectrum')
      self._spectral = False
      return
    w = np.ascontiguousarray(spectrum.wavelengths, dtype=np.float64)
    c = np.ascontiguousarray(spectrum.cdf, dtype=np.float64)
    if w.shape != c.shape or w.ndim != 1:
      raise ValueError('Spectrum: wavelengths and cdf differ in shape')
    self._chk(self._lib.odw_set_spectrum(self._ctx, C.c_int32(_native.SPECTRUM_MODES[spectrum.mode]), C.c_int32(len(w)),
                                         w.ctypes.data_as(pd), c.ctypes.data_as(pd)), 'odw_set_spectrum')
    self._spectral = True

  def rayWavelengths(self, rays, seed):
    """the wavelengths (nm) the bound spectrum gives the ray indices `rays` under `seed` (`odw_ray_wavelengths`)"""
    r = np.ascontiguousarray(rays, dtype=np.uint64).reshape(-1)
    out = np.empty(len(r), np.float64)
    self._chk(self._lib.odw_ray_wavelengths(self._ctx, C.c_uint64(len(r)), r.ctypes.data_as(C.POINTER(C.c_uint64)),
                                            C.c_uint64(int(seed)), out.ctypes.data_as(C.POINTER(C.c_double))), 'odw_ray_wavelengths')
    return out

  def refractiveIndex(self, group, wavelengths, device=False):
    """index of group `group` of the uploaded scene at `wavelengths` (nm) under the dispersion set
    (`odw_dispersion_index`); device=True: evaluated by the kernel-side function"""
    w = np.ascontiguousarray(wavelengths, dtype=np.float64).reshape(-1)
    out = np.empty(len(w), np.float64)
    pd = C.POINTER(C.c_double)
    self._chk(self._lib.odw_dispersion_index(self._ctx, C.c_int32(int(group)), C.c_int32(0), None, C.c_uint64(len(w)),
                                             w.ctypes.data_as(pd), out.ctypes.data_as(pd), C.c_int32(1 if device else 0)),
              'odw_dispersion_index')
    return out

  def compileScene(self, mode='structure'):
    """Scene-compiled kernels (odw_compile_scene): 'structure' -- the ray loop compiled against the
    scene's structure when the scene is bound (0.5 - 2 s up to 16 primitives, 17 s for 61; one kernel per
    structure: parameter sweeps reuse it; cached per process and on disk); 'auto' -- never waits: a cached
    kernel is taken at once, otherwise the generic kernels trace, a thread compiles once the scene has
    traced 5e7 rays, and the launch after it has finished switches over; 'off' / None -- the generic
    kernels.  Sticky: applies to the uploaded scene and to every scene set later.  The results are those of
    the generic kernels bit for bit (which is what makes 'auto' invisible); scenes outside the domain keep
    them silently.  Returns compiledInfo()."""
    f = self._lib.odw_compile_scene
    f.argtypes = [C.c_void_p, C.c_int32]
    self._chk(f(self._ctx, _native.COMPILE_MODES[mode]), 'odw_compile_scene')
    self._compileMode = _native.COMPILE_MODES[mode]
    return self.compiledInfo()

  def compileMode(self):
    """the sticky mode compileScene last set: 0 off, 1 structure, 2 auto"""
    return getattr(self, '_compileMode', 0)

  def compiledInfo(self):
    """dict(mode: 0 generic (in 'auto' mode: not compiled yet) / 1 structure / 2 auto -- of the kernel the next eligible launch runs,
    seconds: compile time of it (0 from a cache), cache: 0 compiled now / 1 process / 2 disk,
    power: the same as `mode` for launches that fill the power plane -- they run a variant of the compiled kernel of
    their own, bound by the first such launch (`odw_compiled_power_info`),
    source: non-zero if the bound kernel generates its rays compiled against the source's structure, 0 if it is the
    source-free kernel (explicit rays, batches, compileScene before setSource) or none (`odw_compiled_source_info`))"""
    f = self._lib.odw_compiled_info
    f.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int32)]
    b, sec, hit = C.c_int32(0), C.c_double(0), C.c_int32(0)
    self._chk(f(self._ctx, C.byref(b), C.byref(sec), C.byref(hit)), 'odw_compiled_info')
    pw = C.c_int32(0)
    self._chk(self._lib.odw_compiled_power_info(self._ctx, C.byref(pw)), 'odw_compiled_power_info')
    key = C.c_uint64(0)
    f = self._lib.odw_compiled_source_info
    f.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    self._chk(f(self._ctx, C.byref(key)), 'odw_compiled_source_info')
    # chroma: the same as `mode` for spectral launches -- they run a variant of the compiled kernel of their own, bound by
    # the first such launch under 'structure' (`odw_compiled_chroma_info`); 0: they walk the binary tree
    ch = C.c_int32(0)
    self._chk(self._lib.odw_compiled_chroma_info(self._ctx, C.byref(ch)), 'odw_compiled_chroma_info')
    # fresnel: likewise for launches with a Fresnel mode set (`odw_compiled_fresnel_info`); 0 also when no mode is set
    fr = C.c_int32(0)
    self._chk(self._lib.odw_compiled_fresnel_info(self._ctx, C.byref(fr)), 'odw_compiled_fresnel_info')
    # bands: likewise for spectral launches that fill the detector's band planes (`odw_compiled_bands_info`)
    bd = C.c_int32(0)
    self._chk(self._lib.odw_compiled_bands_info(self._ctx, C.byref(bd)), 'odw_compiled_bands_info')
    return dict(mode=int(b.value), seconds=float(sec.value), cache=int(hit.value), power=int(pw.value), source=int(key.value),
                chroma=int(ch.value), fresnel=int(fr.value), bands=int(bd.value))

  def setSurfaceSeed(self, seed):
    """Philox key of the stochastic-surface draws in traceRays launches"""
    self._chk(self._lib.odw_set_surface_seed(self._ctx, C.c_uint64(int(seed))), 'odw_set_surface_seed')

  def setWavelength(self, wavelength_nm):
    """wavelength of the following launches (explicit rays); setSource resets it"""
    self._chk(self._lib.odw_set_wavelength(self._ctx, C.c_double(float(wavelength_nm))), 'odw_set_wavelength')

  def setSource(self, source):
    """point source (BakedSource) or surface source (BakedSurfaceSource)"""
    if hasattr(source, 'face_prim'):
      d, keep = _native.surface_source_desc(source)
      self._chk(self._lib.odw_upload_surface_source(self._ctx, C.byref(d)), 'odw_upload_surface_source')
    else:
      d, keep = _native.source_desc(source)
      self._chk(self._lib.odw_upload_source(self._ctx, C.byref(d)), 'odw_upload_source')
    self.source = source
    self._spectral = False
    # (the upload has cleared the previous source's spectrum: what this one carries, if anything)
    if getattr(source, 'spectrum', None) is not None:
      if hasattr(source, 'face_prim'):
        raise ValueError('Spectrum / SpectralDensity: surface sources carry no spectrum')
      self.setSpectrum(source.spectrum)

  def generateRays(self, first, n, seed):
    """initial conditions only (returnInitialConditions, generic_source.py:57): origins, directions"""
    o = np.empty((int(n), 3))
    d = np.empty((int(n), 3))
    pd = C.POINTER(C.c_double)
    self._chk(self._lib.odw_generate_rays(self._ctx, C.c_uint64(int(first)), C.c_uint64(int(n)),
                                          C.c_uint64(int(seed)), o.ctypes.data_as(pd), d.ctypes.data_as(pd)),
              'odw_generate_rays')
    return o, d

  def setLimits(self, lim):
    d = _native.LimitsDesc(float(lim.max_ray_length), int(lim.max_intersections),
                           float(lim.dist_tol), float(lim.power_tol))
    self._chk(self._lib.odw_set_limits(self._ctx, C.byref(d)), 'odw_set_limits')
    self.limits = lim

  def setDetector(self, det, power=False, bands=None):
    """det: dict(group, origin, ex, ey, x_lo, x_hi, y_lo, y_hi, nx, ny) or None
    power: keep a power plane beside the counts (`odw_enable_power_histogram`): every binned hit also adds its power,
    in fixed point (rint(power * 2^32) as uint64 -- integer sums, independent of launch order and GPU count), to
    `powerHistogram()`; launches with `histogram=True` then fill both planes
    bands: K + 1 band edges in nm (strictly increasing, finite, > 0, K <= 64; `odw_set_detector_bands`): spectral launches
    with `histogram=True` -- `trace` under a spectrum, `traceRays(..., wavelengths=)` -- also count every binned hit in the
    plane of its wavelength's band (numpy.histogram's rule on the edges) -> `bandHistogram()`, and with `power` weigh it
    there -> `bandPowerHistogram()`.  Launches that cannot fill the planes (monochromatic, `record_segments`, batches)
    raise NativeError.  None: no bands, exactly as before."""
    self._power = False
    self._bands = None
    if det is None:
      self._chk(self._lib.odw_set_detector(self._ctx, None), 'odw_set_detector')
      self._det = None
      if bands is not None:
        self._setBands(bands)              # (refused by name: bands need a detector)
      return
    d = _native.DetectorDesc()
    d.group = int(det.get('group', -1))
    d.origin = (C.c_double * 3)(*det['origin'])
    d.ex = (C.c_double * 3)(*det['ex'])
    d.ey = (C.c_double * 3)(*det['ey'])
    d.x_lo, d.x_hi, d.y_lo, d.y_hi = (float(det[k]) for k in ('x_lo', 'x_hi', 'y_lo', 'y_hi'))
    d.nx, d.ny = int(det['nx']), int(det['ny'])
    self._chk(self._lib.odw_set_detector(self._ctx, C.byref(d)), 'odw_set_detector')
    self._det = dict(det)
    if power:
      self._chk(self._lib.odw_enable_power_histogram(self._ctx, C.c_int(1)), 'odw_enable_power_histogram')
      self._power = True
    if bands is not None:
      self._setBands(bands)

  def _setBands(self, bands):
    e = np.ascontiguousarray(bands, dtype=np.float64).ravel()
    f = self._lib.odw_set_detector_bands
    f.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_double)]
    if len(e) == 0:
      raise ValueError('bands: at least two edges (None: no bands)')
    self._chk(f(self._ctx, C.c_int32(len(e)), e.ctypes.data_as(C.POINTER(C.c_double))), 'odw_set_detector_bands')
    self._bands = e

  def reserveHits(self, capacity):
    self._chk(self._lib.odw_reserve_hits(self._ctx, C.c_uint64(int(capacity))), 'odw_reserve_hits')

  def reserveSegments(self, capacity):
    """room for the rows of sources with RecordRays (one per ray segment)"""
    self._chk(self._lib.odw_reserve_segments(self._ctx, C.c_uint64(int(capacity))), 'odw_reserve_segments')

  # -- tracing --------------------------------------------------------------
  def _flags(self, record_hits, histogram, record_segments=False):
    return ((TRACE_RECORD_HITS if record_hits else 0) | (TRACE_HISTOGRAM if histogram else 0)
            | (TRACE_RECORD_SEGMENTS if record_segments else 0)
            | (TRACE_POWER_HISTOGRAM if histogram and self._power else 0)
            | (TRACE_BAND_HISTOGRAM if histogram and self._bands is not None else 0))

  def trace(self, first, n, seed, record_hits=True, histogram=True, record_segments=False):
    """asynchronous: rays first..first+n-1 of Philox stream `seed`"""
    self._chk(self._lib.odw_trace(self._ctx, C.c_uint64(int(first)), C.c_uint64(int(n)), C.c_uint64(int(seed)),
                                  C.c_uint32(self._flags(record_hits, histogram, record_segments))),
              'odw_trace')
    if record_hits:
      self._noteLaunch(('seed', int(seed)) if self._spectral else _MONO)

  # -- where the wavelengths of the hit list's rows come from (DeviceHits.histogram(bands=)) -------------------------
  @staticmethod
  def _mergeProvenance(have, new):
    """the provenance of a hit list after rows of provenance `new` joined rows of provenance `have` (None: no rows)"""
    if have is None or new is None:
      return new if have is None else ('mixed', 'rows of unknown wavelengths joined the hit list')
    if have[0] == 'mixed':
      return have
    if new[0] == 'mixed':
      return new
    if 'mono' in (have[0], new[0]):
      return have if have[0] == new[0] else ('mixed', 'monochromatic and spectral launches share the hit list')
    if have[0] != new[0]:
      return ('mixed', 'launches under a spectrum and launches with explicit wavelengths share the hit list')
    if new[0] == 'seed':
      return have if have[1] == new[1] else ('mixed', f'launches under two seeds ({have[1]} and {new[1]}) share the hit list')
    if new[1] != have[1] + len(have[2]):
      return ('mixed', f'the wavelength tables of the launches are not contiguous (rays {have[1]} .. {have[1] + len(have[2]) - 1}, '
                       f'then from {new[1]})')
    return ('table', have[1], np.concatenate([have[2], new[2]]))

  def _noteLaunch(self, new):
    self._archiveOn = self._batchOn = False       # (a launch writes the tracer's own list)
    self._prov = self._mergeProvenance(self._prov, new)

  def hitProvenance(self):
    """what is known about the wavelengths of the rows `deviceHits()` sees: None (nothing: no recording launch, or rows put
    back with loadHits), ('seed', s) -- every launch was a trace() with seed s under a bound spectrum --, ('table', first,
    wavelengths) -- traceRays(wavelengths=) launches whose ray ranges follow each other --, ('mono', reason), or
    ('mixed', reason) when the launches do not share one such description"""
    if self._batchOn:
      return ('mono', 'the rows come from a batch launch (batches carry one wavelength)')
    return self._archiveProv if self._archiveOn else self._prov

  def traceRays(self, origins, directions, powers=None, first=0, record_hits=True, histogram=True,
                record_segments=False, wavelengths=None):
    """wavelengths: one per ray (nm) -- a spectral launch (`odw_trace_rays_spectral`); None: the launch wavelength"""
    o = np.ascontiguousarray(origins, dtype=np.float64).reshape(-1, 3)
    d = np.ascontiguousarray(directions, dtype=np.float64).reshape(-1, 3)
    if o.shape != d.shape:
      raise ValueError('origins and directions differ in shape')
    p = np.ascontiguousarray(powers, dtype=np.float64) if powers is not None else None
    pd = C.POINTER(C.c_double)
    if wavelengths is not None:
      w = np.ascontiguousarray(wavelengths, dtype=np.float64).reshape(-1)
      if len(w) != len(o):
        raise ValueError('wavelengths: one per ray')
      self._chk(self._lib.odw_trace_rays_spectral(
          self._ctx, C.c_uint64(int(first)), C.c_uint64(len(o)), o.ctypes.data_as(pd), d.ctypes.data_as(pd),
          p.ctypes.data_as(pd) if p is not None else None, w.ctypes.data_as(pd),
          C.c_uint32(self._flags(record_hits, histogram, record_segments))), 'odw_trace_rays_spectral')
      if record_hits:
        self._noteLaunch(('table', int(first), w.copy()))
      return
    self._chk(self._lib.odw_trace_rays(
        self._ctx, C.c_uint64(int(first)), C.c_uint64(len(o)), o.ctypes.data_as(pd), d.ctypes.data_as(pd),
        p.ctypes.data_as(pd) if p is not None else None,
        C.c_uint32(self._flags(record_hits, histogram, record_segments))), 'odw_trace_rays')
    if record_hits:
      self._noteLaunch(_MONO)

  # -- batches: scenes of one structure in one launch -------------------------------
  def setSceneBatch(self, scenes):
    """scenes that differ in their numbers only (a parameter sweep: the same primitives, trimming lists, groups and
    optical types) side by side in HBM (`odw_upload_scene_batch`; limits first).  Scene 0 becomes the tracer's scene.
    Raises NativeError (unsupported) when the scenes differ in structure or lie outside the flat kernels' domain --
    the caller then traces them one by one.  Scenes with a paraboloid, an ellipsoid, a conicoid or an asphere (whose coefficients travel in
    the scene's prim_coef, the last field of the descriptor) are in that domain only through
    the kernel compiled against them: after compileScene('structure')."""
    if not len(scenes):
      raise ValueError('empty batch')
    descs, keeps = [], []
    for sc in scenes:
      if self.referenceStrict:
        import copy
        stripped = copy.copy(sc)
        stripped.prim_flags = np.asarray(sc.prim_flags, dtype=np.int32) & ~np.int32(_native.FLAG_CONVEX)
        sc = stripped
      if getattr(sc, 'surface_samplers', None):
        raise _native.NativeError('setSceneBatch: unsupported: scenes with stochastic surfaces are traced one by one')
      if getattr(sc, 'group_fresnel', None) is not None and np.any(np.asarray(sc.group_fresnel) != 0):
        raise _native.NativeError('setSceneBatch: unsupported: scenes with a Fresnel mode are traced one by one')
      if getattr(sc, 'group_coating', None) is not None and np.any(_native.coating_tables(sc.group_coating)[0] != 0):
        raise _native.NativeError('setSceneBatch: unsupported: scenes with a coating are traced one by one')
      d, keep = _native.scene_desc(sc)
      descs.append(d)
      keeps.append(keep)
    arr = (_native.SceneDescCoef * len(descs))(*descs)
    self._chk(self._lib.odw_upload_scene_batch(self._ctx, arr, C.c_int32(len(descs))), 'odw_upload_scene_batch')
    arr0, n0, keep0 = _native.surface_sampler_descs(None)
    self._chk(self._lib.odw_upload_surface_samplers(self._ctx, arr0, C.c_int32(n0)), 'odw_upload_surface_samplers')
    self.scene = scenes[0]
    self.batchScenes = list(scenes)

  def reserveBatch(self, nScenes, rays, rowsPerScene):
    """room for batches of up to nScenes scenes (and for measuring them in HBM) now, not when the first large batch arrives"""
    self._chk(self._lib.odw_batch_reserve(self._ctx, C.c_int32(int(nScenes)), C.c_uint64(int(rays)), C.c_uint64(int(rowsPerScene))),
              'odw_batch_reserve')

  def traceBatch(self, first, n, seed, rowsPerScene, record_hits=True):
    """asynchronous: rays first..first+n-1 of Philox stream `seed` in EVERY scene of the batch, one launch; a scene's
    rows (those of trace() on that scene alone) go to its own segment of the batch's hit list"""
    self._chk(self._lib.odw_trace_batch(self._ctx, C.c_uint64(int(first)), C.c_uint64(int(n)), C.c_uint64(int(seed)),
                                        C.c_uint32(self._flags(record_hits, False)), C.c_uint64(int(rowsPerScene))),
              'odw_trace_batch')

  def batchSelect(self, k):
    """the rows of scene k of the last traceBatch become the tracer's hit list (hits(), hitCount(), deviceHits(),
    hitColumns() ...); None: back to the tracer's own list"""
    self._chk(self._lib.odw_batch_select(self._ctx, C.c_int32(-1 if k is None else int(k))), 'odw_batch_select')
    self._batchOn, self._archiveOn = k is not None, False
    if k is not None:
      self.scene = self.batchScenes[int(k)]

  # -- a run's rows kept in HBM ----------------------------------------------------
  def archiveHits(self, source=None):
    """append the rows of `source`'s hit list (default: this tracer's own) to this tracer's archive in HBM
    (device to device; the source's launch is waited for) -> rows archived so far"""
    src = self if source is None else source
    n = C.c_uint64(0)
    f = self._lib.odw_archive_append
    f.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
    self._chk(f(self._ctx, src._ctx, C.byref(n)), 'odw_archive_append')
    # (the rows' provenance travels with them; so does the source's spectrum, inside odw_archive_append)
    self._archiveProv = self._mergeProvenance(self._archiveProv, src._prov)
    return int(n.value)

  def archiveSelect(self, on=True):
    """the archive becomes the tracer's hit list (hits(), hitCount(), deviceHits() ...); False: back to its own list"""
    self._chk(self._lib.odw_archive_select(self._ctx, C.c_int32(1 if on else 0)), 'odw_archive_select')
    self._archiveOn, self._batchOn = bool(on), False

  def archiveReset(self):
    self._chk(self._lib.odw_archive_reset(self._ctx), 'odw_archive_reset')
    self._archiveProv, self._archiveOn = None, False

  def batchRows(self):
    """(rows recorded per scene, slots asked for per scene) of the last traceBatch"""
    n = len(self.batchScenes)
    rows, wanted = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    pu = C.POINTER(C.c_uint64)
    self._chk(self._lib.odw_batch_rows(self._ctx, rows.ctypes.data_as(pu), wanted.ctypes.data_as(pu), C.c_int32(n)), 'odw_batch_rows')
    return rows, wanted

  def memInfo(self):
    """(free, total) bytes of the tracer's device"""
    free, total = C.c_uint64(0), C.c_uint64(0)
    self._chk(self._lib.odw_mem_info(self._ctx, C.byref(free), C.byref(total)), 'odw_mem_info')
    return int(free.value), int(total.value)

  def sync(self):
    self._chk(self._lib.odw_sync(self._ctx), 'odw_sync')

  def reset(self):
    self._chk(self._lib.odw_reset_results(self._ctx), 'odw_reset_results')
    self._prov = None

  def resetHits(self):
    """recycle the hit list (the reference's periodic flush,
    results_store.py:455-457); counters and histogram keep accumulating"""
    self._chk(self._lib.odw_reset_hits(self._ctx), 'odw_reset_hits')
    self._prov = None

  # -- results --------------------------------------------------------------
  def counters(self):
    out = np.zeros(len(CNT_NAMES), dtype=np.uint64)
    self._chk(self._lib.odw_fetch_counters(self._ctx, out.ctypes.data_as(C.POINTER(C.c_uint64)),
                                           C.c_int32(len(out))), 'odw_fetch_counters')
    return {k: int(v) for k, v in zip(CNT_NAMES, out)}

  @staticmethod
  def raiseForRayErrors(cnt):
    """exceptions the reference raises from inside Ray.traceRay, turned into counters by the kernels:
    a ray that enters a transmission grating while inside a medium (ray.py:234-237)"""
    if cnt.get('grating_in_medium'):
      raise ValueError('ray entered grating while already being inside a medium, get rid of any overlapping '
                       'lenses/transmission gratings in your project '
                       f'({cnt["grating_in_medium"]} ray(s) of this launch)')

  def hitCount(self):
    n = C.c_uint64(0)
    self._chk(self._lib.odw_hit_count(self._ctx, C.byref(n)), 'odw_hit_count')
    return int(n.value)

  def hits(self):
    """recorded hit rows sorted by (ray index, bounce order)"""
    n = self.hitCount()
    out = np.zeros(n, dtype=HIT_DTYPE)
    got = C.c_uint64(0)
    self._chk(self._lib.odw_fetch_hits(self._ctx, out.ctypes.data_as(C.c_void_p), C.c_uint64(n),
                                       C.byref(got)), 'odw_fetch_hits')
    return out[:int(got.value)]

  def hostRows(self, n):
    """page-locked array of n hit rows (destination of row fetches: copied into directly by the
    copy engine); freed with the tracer"""
    p = C.c_void_p()
    nbytes = int(n) * HIT_DTYPE.itemsize
    self._chk(self._lib.odw_host_alloc(self._ctx, C.c_uint64(nbytes), C.byref(p)), 'odw_host_alloc')
    self._pinned = getattr(self, '_pinned', [])
    self._pinned.append(p)
    buf = (C.c_char * nbytes).from_address(p.value)
    return np.frombuffer(buf, dtype=HIT_DTYPE)

  def traceStreaming(self, jobs, seed, capacity, histogram=True, buffers=None):
    """generator: trace every (first, n) of `jobs` and yield each job's hit rows on the host, the
    copy of job k overlapping the trace of job k+1 (two device hit lists, a copy stream of its
    own: odw_swap_hit_lists / odw_fetch_swapped_hits).  Rows come in append order (unordered
    across rays).  The arrays yielded are views of two alternating host buffers: use one before
    asking for the one after the next."""
    self.reserveHits(capacity)
    host = buffers or [self.hostRows(capacity) for _ in range(2)]
    got = C.c_uint64(0)

    def fetch(k):
      buf = host[k % 2]
      self._chk(self._lib.odw_fetch_swapped_hits(self._ctx, buf.ctypes.data_as(C.c_void_p), C.c_uint64(len(buf)),
                                                 C.byref(got)), 'odw_fetch_swapped_hits')
      return buf[:int(got.value)]
    # from the first swap on appends are dense (the rows of a list are copied as they lie)
    self._chk(self._lib.odw_swap_hit_lists(self._ctx), 'odw_swap_hit_lists')
    try:
      k = -1
      for k, (first, n) in enumerate(jobs):
        self.resetHits()
        self.trace(first, n, seed, histogram=histogram)       # asynchronous, into the current list
        if k > 0:
          yield fetch(k - 1)                                  # the list put aside: job k-1
        self._chk(self._lib.odw_swap_hit_lists(self._ctx), 'odw_swap_hit_lists')
      if k >= 0:
        yield fetch(k)
    finally:
      # back to one list: later launches reserve hit-list blocks per wave again
      self._chk(self._lib.odw_release_swapped_hits(self._ctx), 'odw_release_swapped_hits')

  def hitColumns(self, group, pinned=True, rayIndex=True):
    """the recorded rows of one group as the arrays the reference pickles per (source, object)
    (results_store.py:405-457): dict(points (n, 3), directions (n, 3), powers (n), isEntering (n) int64,
    rayIndex (n) int64), in (ray index, bounce) order -- selected and split into columns on the device
    (odw_hits_select + odw_hits_columns), so the host only receives them; None if the group has no row.
    pinned: the arrays live in page-locked memory of the process' pool (_PinnedPool) until they are dropped
    (they may outlive the tracer); then their memory returns to the pool.  rayIndex=False: without that column (it
    serves the per-ray metadata only: an eighth less to copy)"""
    n, leaving = C.c_uint64(0), C.c_uint64(0)
    self._chk(self._lib.odw_hits_select(self._ctx, C.c_int32(int(group)), C.byref(n), C.byref(leaving)), 'odw_hits_select')
    m = int(n.value)
    if m == 0:
      return None
    per_row = 9 if rayIndex else 8                          # doubles per row: 3 + 3 + 1 + 1 (+ 1: the ray's number)
    if pinned:
      buf = _POOL.take(self, m * 8 * per_row)
      f8 = np.frombuffer(buf, dtype=np.float64, count=per_row * m)
      out = dict(points=f8[:3 * m].reshape(m, 3), directions=f8[3 * m:6 * m].reshape(m, 3), powers=f8[6 * m:7 * m],
                 isEntering=f8[7 * m:8 * m].view(np.int64))
      if rayIndex:
        out['rayIndex'] = f8[8 * m:9 * m].view(np.int64)
    else:
      out = dict(points=np.empty((m, 3)), directions=np.empty((m, 3)), powers=np.empty(m), isEntering=np.empty(m, dtype=np.int64))
      if rayIndex:
        out['rayIndex'] = np.empty(m, dtype=np.int64)
    f = self._lib.odw_hits_columns
    f.argtypes = [C.c_void_p] + [C.c_void_p] * 5 + [C.c_uint64, C.POINTER(C.c_uint64)]
    got = C.c_uint64(0)
    self._chk(f(self._ctx, *(out[k].ctypes.data_as(C.c_void_p) if k in out else None
                             for k in ('points', 'directions', 'powers', 'isEntering', 'rayIndex')), C.c_uint64(m), C.byref(got)),
              'odw_hits_columns')
    assert int(got.value) == m
    return out

  def deviceHits(self, group=None):
    """the recorded rows as a `Hits`-like object that bins them where they are, in HBM
    (`simulation.device_hits.DeviceHits`); valid until the next launch, reset or fetch"""
    from .device_hits import DeviceHits
    self.sync()
    return DeviceHits(self, group)

  def loadHits(self, hits, group=0):
    """put recorded hits back into the device hit list (replacing its content) and return them as
    `DeviceHits`: `hits` = HIT_DTYPE rows, or a hit dictionary / `Hits` as `RawFolder.loadHits`
    returns it (points, directions, powers, isEntering; rows are numbered in their order)"""
    if isinstance(hits, np.ndarray) and hits.dtype == HIT_DTYPE:
      rows = np.ascontiguousarray(hits)
    else:
      d = getattr(hits, 'hits', hits)
      n = len(d['points'])
      rows = np.zeros(n, dtype=HIT_DTYPE)
      rows['point'], rows['direction'] = d['points'], d['directions']
      rows['power'] = d['powers'] if 'powers' in d else 1.0
      ent = np.asarray(d['isEntering'] if 'isEntering' in d else np.ones(n), dtype=np.uint64)
      rows['tag'] = (np.arange(n, dtype=np.uint64) | (np.uint64(int(group)) << np.uint64(48))
                     | ((ent != 0).astype(np.uint64) << np.uint64(63)))
    self._chk(self._lib.odw_load_hits(self._ctx, rows.ctypes.data_as(C.c_void_p), C.c_uint64(len(rows))), 'odw_load_hits')
    self._prov, self._archiveOn, self._batchOn = None, False, False      # (rows of unknown wavelengths: histogram(bands=, wavelengths=))
    return self.deviceHits()

  def resetSegments(self):
    self._chk(self._lib.odw_reset_segments(self._ctx), 'odw_reset_segments')

  def segmentCount(self):
    """(rows in the segment list, rows that did not fit)"""
    n, dropped = C.c_uint64(0), C.c_uint64(0)
    self._chk(self._lib.odw_segment_count(self._ctx, C.byref(n), C.byref(dropped)), 'odw_segment_count')
    return int(n.value), int(dropped.value)

  def segments(self):
    """recorded ray segments sorted by (ray index, ordinal)"""
    n, _ = self.segmentCount()
    out = np.zeros(n, dtype=SEGMENT_DTYPE)
    got = C.c_uint64(0)
    self._chk(self._lib.odw_fetch_segments(self._ctx, out.ctypes.data_as(C.c_void_p), C.c_uint64(n),
                                           C.byref(got)), 'odw_fetch_segments')
    return out[:int(got.value)]

  def histogram(self):
    if self._det is None:
      raise ValueError('no detector set')
    nb = self._det['nx'] * self._det['ny']
    out = np.zeros(nb, dtype=np.uint64)
    self._chk(self._lib.odw_fetch_histogram(self._ctx, out.ctypes.data_as(C.POINTER(C.c_uint64)),
                                            C.c_uint64(nb)), 'odw_fetch_histogram')
    return out.reshape(self._det['nx'], self._det['ny'])

  def powerHistogramRaw(self):
    """the power plane as the library keeps it: uint64 (nx, ny), bin = sum over its hits of rint(power * 2^32).  Raises
    without `setDetector(..., power=True)`, and NativeError (capacity) when a bin holds 2^32 hits or more -- its sum may
    have wrapped.  Explicit rays with powers above 1 (`traceRays`): the bound is hits of a bin x largest power < 2^32."""
    if self._det is None or not self._power:
      raise ValueError('no power plane: setDetector(det, power=True)')
    nb = self._det['nx'] * self._det['ny']
    out = np.zeros(nb, dtype=np.uint64)
    self._chk(self._lib.odw_fetch_power_histogram(self._ctx, out.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                  C.c_uint64(nb)), 'odw_fetch_power_histogram')
    return out.reshape(self._det['nx'], self._det['ny'])

  def powerHistogram(self):
    """power per detector bin, float64 (nx, ny), in units of the source's power: `powerHistogramRaw() * 2^-32`"""
    return self.powerHistogramRaw().astype(np.float64) * 2.0 ** -POWER_QUANTUM_BITS

  def _bandPlanes(self, name):
    if self._det is None or self._bands is None:
      raise ValueError('no bands: setDetector(det, bands=edges)')
    k, nx, ny = len(self._bands) - 1, self._det['nx'], self._det['ny']
    out = np.zeros(k * nx * ny, dtype=np.uint64)
    self._chk(getattr(self._lib, name)(self._ctx, out.ctypes.data_as(C.POINTER(C.c_uint64)), C.c_uint64(len(out))), name)
    return out.reshape(k, nx, ny)

  def bandHistogram(self):
    """the band count planes: uint64 (K, nx, ny); plane b counts the binned hits of spectral launches whose wavelength
    lies in band b of `setDetector(..., bands=)` -- `bandHistogram().sum(0) <= histogram()`, equal where the edges
    cover every wavelength"""
    return self._bandPlanes('odw_fetch_band_histogram')

  def bandPowerHistogramRaw(self):
    """the band power planes as raw quanta: uint64 (K, nx, ny), `powerHistogramRaw()`'s rules per band plane"""
    if not self._power:
      raise ValueError('no power plane: setDetector(det, power=True, bands=edges)')
    return self._bandPlanes('odw_fetch_band_power_histogram')

  def bandPowerHistogram(self):
    """power per band and detector bin, float64 (K, nx, ny), in units of the source's power"""
    return self.bandPowerHistogramRaw().astype(np.float64) * 2.0 ** -POWER_QUANTUM_BITS

  @staticmethod
  def bandIndex(edges, wavelengths, device=False):
    """the band (int32, -1: none) of every wavelength among `edges`: the kernels' rule (`odw_band_index`), on the host
    or, with device=True, by the kernels' own search on the GPU"""
    return _native.band_index(edges, wavelengths, device=device)

  def sample(self, first, n, seed):
    t = np.empty(int(n))
    phi = np.empty(int(n))
    pd = C.POINTER(C.c_double)
    self._chk(self._lib.odw_sample(self._ctx, C.c_uint64(int(first)), C.c_uint64(int(n)),
                                   C.c_uint64(int(seed)), t.ctypes.data_as(pd), phi.ctypes.data_as(pd)),
              'odw_sample')
    return t, phi

  # -- device views for collectives ------------------------------------------
  def histogramView(self):
    p, n = C.c_void_p(), C.c_uint64(0)
    self._chk(self._lib.odw_device_histogram(self._ctx, C.byref(p), C.byref(n)), 'odw_device_histogram')
    return _CudaArrayView(p.value, n.value, '<i8', self)

  def powerHistogramView(self):
    """the power plane in HBM (raw quanta)"""
    if not self._power:
      raise ValueError('no power plane: setDetector(det, power=True)')
    p, n = C.c_void_p(), C.c_uint64(0)
    self._chk(self._lib.odw_device_power_histogram(self._ctx, C.byref(p), C.byref(n)), 'odw_device_power_histogram')
    return _CudaArrayView(p.value, n.value, '<i8', self)

  def bandHistogramView(self):
    """the band planes in HBM: K count planes, then with the power plane K planes of raw quanta, as one int64 vector"""
    if self._bands is None:
      raise ValueError('no bands: setDetector(det, bands=edges)')
    p, n = C.c_void_p(), C.c_uint64(0)
    self._chk(self._lib.odw_device_band_histogram(self._ctx, C.byref(p), C.byref(n)), 'odw_device_band_histogram')
    return _CudaArrayView(p.value, n.value, '<i8', self)

  def countersView(self):
    p, n = C.c_void_p(), C.c_uint64(0)
    self._chk(self._lib.odw_device_counters(self._ctx, C.byref(p), C.byref(n)), 'odw_device_counters')
    return _CudaArrayView(p.value, n.value, '<i8', self)

  def resultsView(self):
    """counters and histogram -- and, with `setDetector(..., power=True)`, the power plane directly behind the
    histogram's nx * ny bins, and with `bands=` the K band count planes and (with power) K band power planes behind
    those -- as ONE int64 vector in HBM (`odw_device_results`): what a multi-GPU job sums with a
    single reduce (the plane's uint64 quanta add as int64 words do).  -> (view, offset of the first histogram bin in words)"""
    p, n, off = C.c_void_p(), C.c_uint64(0), C.c_uint64(0)
    self._chk(self._lib.odw_device_results(self._ctx, C.byref(p), C.byref(n), C.byref(off)), 'odw_device_results')
    return _CudaArrayView(p.value, n.value, '<i8', self), int(off.value)

  def stream(self):
    p = C.c_void_p()
    self._chk(self._lib.odw_stream(self._ctx, C.byref(p)), 'odw_stream')
    return p.value

  # -- timing -----------------------------------------------------------------
  def timingEnable(self, on=True):
    self._chk(self._lib.odw_timing_enable(self._ctx, C.c_int(1 if on else 0)), 'odw_timing_enable')
    self._timingOn = bool(on)          # (contexts a sweep creates beside this one follow it: simulation/sweep.py)

  def timingRead(self):
    ms, n = C.c_double(0), C.c_uint64(0)
    self._chk(self._lib.odw_timing_read(self._ctx, C.byref(ms), C.byref(n)), 'odw_timing_read')
    return float(ms.value), int(n.value)


def segmentsToRays(segs, scene):
  """rows sorted by (ray, ordinal) -> one dictionary per ray, the layout
  SimulationResultsSingleRay.dump pickles (results_store.py:241-257):
  points (k+1, 3) = every segment's start + the end of the last one,
  powers (k,), media (k names, None = vacuum); plus globalRayIndex"""
  if len(segs) == 0:
    return []
  tags = segs['tag']
  ray = (tags & np.uint64(0xFFFFFFFFFF)).astype(np.int64)
  medium = ((tags >> np.uint64(52)) & np.uint64(0xFFF)).astype(np.int64) - 1
  starts = np.flatnonzero(np.r_[True, ray[1:] != ray[:-1]])
  ends = np.r_[starts[1:], len(segs)]
  names = list(scene.group_names)
  out = []
  for a, b in zip(starts, ends):
    out.append(dict(points=np.vstack([segs['p1'][a:b], segs['p2'][b - 1:b]]),
                    powers=np.array(segs['power'][a:b]),
                    media=[names[m] if m >= 0 else None for m in medium[a:b]],
                    globalRayIndex=int(ray[a])))
  return out


def hitsToDict(hits, scene, sourceName='', group=None):
  """rows -> the reference's pickled hit dictionary
  (results_store.py:405-457): one dict per (source, object)."""
  tags = hits['tag']
  grp = ((tags >> np.uint64(48)) & np.uint64(0x7FFF)).astype(np.int64)
  out = {}
  for g in np.unique(grp) if group is None else [group]:
    sel = grp == g
    out[scene.group_names[g]] = dict(
        source=sourceName, obj=scene.group_names[g],
        points=np.ascontiguousarray(hits['point'][sel]),
        directions=np.ascontiguousarray(hits['direction'][sel]),
        powers=np.ascontiguousarray(hits['power'][sel]),
        isEntering=(tags[sel] >> np.uint64(63)).astype(np.int64),
        globalRayIndex=(tags[sel] & np.uint64(0xFFFFFFFFFFFF)).astype(np.int64))
  return out
