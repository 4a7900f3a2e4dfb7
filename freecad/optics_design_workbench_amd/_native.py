"""ctypes binding of the HIP library (csrc/libodw_trace.so, include/odw_trace.h).

There is no CPU fallback: if the library is missing or no GPU is present the
calls raise.  `build()` compiles the library in-tree with hipcc for gfx950
(cross-compiles without a GPU).
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

# HIP spreads a process' streams over this many hardware queues (default 4); kernels of streams that share one wait for each
# other.  A parameter sweep keeps five contexts' chains in flight beside each other: small kernels of one must not queue
# behind the 7 ms launch of another.  Read by the HIP runtime when it initialises, so: set before the first HIP call.
os.environ.setdefault('GPU_MAX_HW_QUEUES', '16')

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, 'csrc')
LIB_PATH = os.path.join(CSRC, 'libodw_trace.so')
_SOURCES = ['odw_capi.hip', 'odw_kernels.hip', 'odw_grid.hip', 'odw_mesh.hip', 'odw_posthoc.hip', 'odw_posthoc_batch.hip', 'odw_spec.hip', 'odw_device.h', 'odw_build.h']
_HEADER = os.path.normpath(os.path.join(_HERE, '..', '..', 'include', 'odw_trace.h'))

ABI_VERSION = 12
CNT_NAMES = ['traced_rays', 'recorded_hits', 'segments', 'escaped', 'died', 'capped',
             'hist_overflow', 'hits_dropped', 'grating_in_medium']
TRACE_RECORD_HITS, TRACE_HISTOGRAM, TRACE_RECORD_SEGMENTS, TRACE_POWER_HISTOGRAM = 1, 2, 4, 8
TRACE_BAND_HISTOGRAM = 16                 # ODW_TRACE_BAND_HISTOGRAM: the detector's band planes (odw_set_detector_bands)
BAND_MAX = 64                             # ODW_BAND_MAX: bands of a detector at most
POWER_QUANTUM_BITS = 32                   # ODW_POWER_QUANTUM_BITS: a hit's weight is rint(clamp(power, 0, 2^20) * 2^32)
FLAG_FLIP_NORMAL, FLAG_CONVEX = 1, 2      # ODW_FLAG_* of prim_flags (include/odw_trace.h)
PRIM_PARABOLOID, PRIM_ELLIPSOID, PRIM_CONICOID, PRIM_ASPHERE = 6, 7, 8, 9    # ODW_PRIM_*: the rare kinds (scene.geometry holds the whole list of kinds)
ASPH_COEFS = 8                            # ODW_ASPH_COEFS: a_1 .. a_8 of an asphere's row of prim_coef
COMPILE_OFF, COMPILE_STRUCTURE, COMPILE_AUTO = 0, 1, 2
COMPILE_MODES = {None: 0, False: 0, 'off': 0, 0: 0, 'structure': 1, 1: 1, True: 1, 'auto': 2, 2: 2}
ERRORS = {1: 'invalid argument', 2: 'device error', 3: 'no scene', 4: 'capacity', 5: 'unsupported'}
BUSY = 6             # ODW_BUSY: not an error (polling calls)

HIT_DTYPE = np.dtype([('point', '<f8', 3), ('direction', '<f8', 3), ('power', '<f8'), ('tag', '<u8')])
SEGMENT_DTYPE = np.dtype([('p1', '<f8', 3), ('p2', '<f8', 3), ('power', '<f8'), ('tag', '<u8')])

# every symbol include/odw_trace.h declares
SYMBOLS = ['odw_abi_version', 'odw_create', 'odw_destroy', 'odw_last_error', 'odw_upload_scene',
           'odw_upload_source', 'odw_upload_surface_source', 'odw_generate_rays', 'odw_upload_surface_samplers', 'odw_set_surface_seed', 'odw_set_wavelength', 'odw_set_limits', 'odw_set_detector', 'odw_reserve_hits', 'odw_reserve_segments', 'odw_trace',
           'odw_trace_rays', 'odw_sync', 'odw_reset_results', 'odw_reset_hits', 'odw_fetch_counters', 'odw_hit_count',
           'odw_fetch_hits', 'odw_fetch_histogram', 'odw_segment_count', 'odw_fetch_segments', 'odw_reset_segments', 'odw_sample', 'odw_device_histogram',
           'odw_device_counters', 'odw_device_results', 'odw_stream', 'odw_timing_enable', 'odw_timing_read',
           'odw_swap_hit_lists', 'odw_fetch_swapped_hits', 'odw_release_swapped_hits', 'odw_mem_info', 'odw_host_alloc', 'odw_host_free', 'odw_load_hits', 'odw_hits_select', 'odw_hits_gather', 'odw_hits_project', 'odw_hits_range', 'odw_hits_bin', 'odw_hits_moments', 'odw_plane_screen',
           'odw_compile_scene', 'odw_compiled_info', 'odw_compile_check', 'odw_compile_check_source', 'odw_compiled_source_info', 'odw_upload_source_unguided', 'odw_build_check', 'odw_table_slopes', 'odw_spec_image', 'odw_hits_columns',
           'odw_upload_scene_batch', 'odw_trace_batch', 'odw_batch_select', 'odw_batch_rows',
           'odw_plane_screen_batch', 'odw_archive_append', 'odw_archive_select', 'odw_archive_reset', 'odw_batch_hits_select', 'odw_batch_hits_sample', 'odw_batch_hits_project', 'odw_batch_hits_bin',
           'odw_batch_reserve', 'odw_batch_hits_begin', 'odw_batch_hits_sampled', 'odw_batch_hits_measure', 'odw_batch_hits_measured',
           'odw_enable_power_histogram', 'odw_fetch_power_histogram', 'odw_device_power_histogram', 'odw_hits_bin_power', 'odw_compiled_power_info',
           'odw_set_dispersion', 'odw_set_spectrum', 'odw_trace_rays_spectral', 'odw_ray_wavelengths', 'odw_dispersion_index',
           'odw_dispersion_check', 'odw_spectrum_check', 'odw_compiled_chroma_info', 'odw_compile_check_chroma',
           'odw_set_fresnel', 'odw_compiled_fresnel_info', 'odw_fresnel_reflectance', 'odw_compile_check_fresnel', 'odw_fresnel_check',
           'odw_set_coating', 'odw_coating_check', 'odw_coated_reflectance', 'odw_compile_check_coating',
           'odw_set_detector_bands', 'odw_fetch_band_histogram', 'odw_fetch_band_power_histogram', 'odw_device_band_histogram',
           'odw_band_index', 'odw_compiled_bands_info', 'odw_compile_check_bands',
           'odw_hits_bin_bands', 'odw_hits_bin_bands_info']

# dispersion of a group (ODW_DISP_*) and spectrum of a point source (ODW_SPECTRUM_*)
DISP_NONE, DISP_SELLMEIER, DISP_CAUCHY = 0, 1, 2
DISP_KINDS = {'': 0, None: 0, 'Sellmeier': 1, 'Cauchy': 2}
DISP_COEFS = 6                            # ODW_DISP_COEFS
SPECTRUM_MODES = {'lines': 1, 'density': 2}
ROW_WL_SPECTRUM, ROW_WL_TABLE = 1, 2      # ODW_ROW_WL_*: where odw_hits_bin_bands takes a row's wavelength from
STREAM_WAVELENGTH = 6                     # ODW_STREAM_WAVELENGTH: word 3 of the Philox counter of the wavelength draw
# Fresnel mode of a lens group (ODW_FRESNEL_*)
FRESNEL_NONE, FRESNEL_LOSS, FRESNEL_SPLIT = 0, 1, 2
FRESNEL_MODES = {'': 0, None: 0, 'Loss': 1, 'Split': 2}
COAT_LAYERS = 4                           # ODW_COAT_LAYERS: layers of a group's thin-film coating at most
STREAM_FRESNEL = 7                        # ODW_STREAM_FRESNEL: word 3 of the Philox counter of the reflect-or-transmit draw

_pd = C.POINTER(C.c_double)
_pi = C.POINTER(C.c_int32)
_pu = C.POINTER(C.c_uint64)


class SceneDesc(C.Structure):
  _fields_ = [('n_prims', C.c_int32), ('prim_type', _pi), ('prim_group', _pi), ('prim_solid', _pi),
              ('prim_flags', _pi), ('prim_xform', _pd), ('prim_params', _pd), ('prim_cond_off', _pi),
              ('n_conds', C.c_int32), ('cond_prim', _pi), ('cond_inside', _pi),
              ('n_groups', C.c_int32), ('group_type', _pi), ('group_ior', _pd), ('group_refl', _pd),
              ('group_abslen', _pd), ('group_record', _pi), ('group_grating_type', _pi),
              ('group_grating_lpm', _pd), ('group_grating_dir', _pd), ('group_grating_order', _pi),
              ('seq_enabled', C.c_int32), ('seq_len', C.c_int32), ('seq_mask', _pu),
              ('ignore_mask', C.c_uint64), ('tri_normals', _pd), ('tri_edges', _pi)]


class SceneDescCoef(SceneDesc):
  """odw_scene_desc as the library reads it: the fields above (the layout it shares with the oracle's descriptor) and,
  behind them, the aspheres' coefficient table.  What scene_desc() returns and what arrays of scenes are made of.

  Why two classes: SceneDesc stays, field for field, the oracle's descriptor (the frozen oracle does not know the new
  field), and callers that declare POINTER(SceneDesc) keep working, since ctypes takes an instance of a subclass there.
  Pass the library a SceneDescCoef, always.  A bare SceneDesc is 8 bytes short of what the library's struct is: the
  library reads the last field only once a scene holds an asphere row (and the validation of the tables comes first),
  so a bare one is read correctly as long as it describes no asphere -- but never put bare ones into an array for
  odw_upload_scene_batch, whose stride is the full size."""
  _fields_ = [('prim_coef', _pd)]


class SourceDesc(C.Structure):
  _fields_ = [('xform', C.c_double * 12), ('focal_length', C.c_double), ('wavelength', C.c_double),
              ('power', C.c_double), ('n_phi_knots', C.c_int32), ('phi_edges', _pd), ('phi_cdf', _pd),
              ('n_t_knots', C.c_int32), ('n_t_rows', C.c_int32), ('t_edges', _pd), ('t_cdf', _pd)]


class SurfaceSamplerDesc(C.Structure):
  _fields_ = [('group', C.c_int32), ('kind', C.c_int32), ('family_axis', C.c_int32), ('n_family', C.c_int32),
              ('family_lo', C.c_double), ('family_hi', C.c_double), ('n_phi_knots', C.c_int32),
              ('phi_edges', _pd), ('phi_cdf', _pd), ('n_t_knots', C.c_int32), ('n_t_rows', C.c_int32),
              ('t_edges', _pd), ('t_cdf', _pd), ('mu', C.c_double), ('n_atoms', C.c_int32),
              ('atom_mass', _pd), ('atom_theta', _pd), ('atom_phi', _pd)]


class SurfaceSourceDesc(C.Structure):
  _fields_ = [('wavelength', C.c_double), ('power', C.c_double), ('dist_tol', C.c_double),
              ('n_prims', C.c_int32), ('prim_type', _pi), ('prim_flags', _pi), ('prim_xform', _pd),
              ('prim_params', _pd), ('prim_cond_off', _pi), ('n_conds', C.c_int32), ('cond_prim', _pi),
              ('cond_inside', _pi), ('n_faces', C.c_int32), ('face_prim', _pi), ('face_id', _pi),
              ('face_area', _pd), ('n_t_knots', C.c_int32), ('t_edges', _pd), ('t_cdf', _pd), ('tri_normals', _pd)]


class LimitsDesc(C.Structure):
  _fields_ = [('max_ray_length', C.c_double), ('max_intersections', C.c_int32),
              ('dist_tol', C.c_double), ('power_tol', C.c_double)]


class DetectorDesc(C.Structure):
  _fields_ = [('group', C.c_int32), ('origin', C.c_double * 3), ('ex', C.c_double * 3),
              ('ey', C.c_double * 3), ('x_lo', C.c_double), ('x_hi', C.c_double),
              ('y_lo', C.c_double), ('y_hi', C.c_double), ('nx', C.c_int32), ('ny', C.c_int32)]


class NativeError(RuntimeError):
  pass


def hipcc():
  for cand in (os.environ.get('HIPCC'), '/opt/rocm/bin/hipcc', shutil.which('hipcc')):
    if cand and os.path.exists(cand):
      return cand
  raise NativeError('hipcc not found; the HIP library cannot be built')


def sources_hash(csrc=None, header=None):
  """sha256 over the sources a build of the library is made of (csrc/*.hip, csrc/*.h, include/odw_trace.h; names and
  contents, in name order): what ties a committed counter pass (profiles/pmc_current.json) to the code it was taken on"""
  import hashlib
  csrc = CSRC if csrc is None else csrc
  header = _HEADER if header is None else header
  h = hashlib.sha256()
  for name in sorted(_SOURCES):
    path = os.path.join(csrc, name)
    h.update(name.encode() + b'\0')
    with open(path, 'rb') as f:
      h.update(f.read())
    h.update(b'\0')
  h.update(b'odw_trace.h\0')
  with open(header, 'rb') as f:
    h.update(f.read())
  return h.hexdigest()


def needs_build():
  if not os.path.exists(LIB_PATH):
    return True
  t = os.path.getmtime(LIB_PATH)
  deps = [os.path.join(CSRC, s) for s in _SOURCES] + [_HEADER]
  return any(os.path.getmtime(d) > t for d in deps if os.path.exists(d))


def build(force=False, verbose=False):
  """compile csrc/ for gfx950 into csrc/libodw_trace.so"""
  if not force and not needs_build():
    return LIB_PATH
  # -ffp-contract=on: products and sums are fused where one expression says so, never across statements
  # -- the generic kernels and the scene-compiled ones (odw_spec.hip, same flag) then round alike
  cmd = [hipcc(), '--offload-arch=gfx950', '-O3', '-std=c++17', '-ffp-contract=on', '-fPIC', '-shared',
         '-o', LIB_PATH + '.tmp', os.path.join(CSRC, 'odw_capi.hip')]
  if verbose:
    cmd.insert(1, '-Rpass-analysis=kernel-resource-usage')
  res = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
  if res.returncode != 0:
    raise NativeError('hipcc failed:\n' + res.stdout + res.stderr)
  os.replace(LIB_PATH + '.tmp', LIB_PATH)
  if verbose:
    print(res.stderr)
  return LIB_PATH


ASAN_LIB_PATH = os.path.join(CSRC, 'libodw_trace_asan.so')


def build_sanitized(force=False):
  """The library with AddressSanitizer + UndefinedBehaviorSanitizer on its HOST code (the device code is compiled as
  usual: GPU sanitizers are not available on this pool), for the entry points that never touch a GPU -- scene validation,
  boxes, the grid / tree builders (odw_build_check), the plane screens, the header of a compiled scene -- in a child
  process with the sanitizer runtime preloaded (tests/test_native_sanitized.py).  -> (library path, runtime path)"""
  runtime = subprocess.run([hipcc(), '--print-file-name=libclang_rt.asan-x86_64.so'], capture_output=True, text=True).stdout.strip()
  if not os.path.isabs(runtime) or not os.path.exists(runtime):
    raise NativeError('the sanitizer runtime of hipcc\'s clang was not found')
  deps = [os.path.join(CSRC, s) for s in _SOURCES] + [_HEADER]
  if force or not os.path.exists(ASAN_LIB_PATH) or any(os.path.getmtime(d) > os.path.getmtime(ASAN_LIB_PATH) for d in deps):
    cmd = [hipcc(), '--offload-arch=gfx950', '-O1', '-g', '-std=c++17', '-ffp-contract=on', '-fPIC', '-shared',
           '-fsanitize=address,undefined', '-fno-gpu-sanitize', '-fno-omit-frame-pointer', '-shared-libasan',
           '-o', ASAN_LIB_PATH + '.tmp', os.path.join(CSRC, 'odw_capi.hip')]
    res = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
    if res.returncode != 0:
      raise NativeError('hipcc (sanitized build) failed:\n' + res.stdout + res.stderr)
    os.replace(ASAN_LIB_PATH + '.tmp', ASAN_LIB_PATH)
  return ASAN_LIB_PATH, runtime


_lib = None


def lib():
  """the loaded library; raises if it is absent (no fallback)"""
  global _lib
  if _lib is None:
    if not os.path.exists(LIB_PATH):
      raise NativeError(f'{LIB_PATH} is missing: run __graft_entry__.build() '
                        f'(or freecad.optics_design_workbench_amd._native.build()) first')
    # ODW_TRACE_LIB: another build of the same library (kernel experiments, scripts/build_variant.py)
    l = C.CDLL(os.environ.get('ODW_TRACE_LIB') or LIB_PATH)
    l.odw_last_error.restype = C.c_char_p
    l.odw_last_error.argtypes = [C.c_void_p]
    l.odw_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    l.odw_destroy.argtypes = [C.c_void_p]
    l.odw_destroy.restype = None
    for name in SYMBOLS:
      getattr(l, name)
    if l.odw_abi_version() != ABI_VERSION:
      raise NativeError('libodw_trace.so ABI version mismatch; rebuild')
    _lib = l
  return _lib


def check(ctx, rc, what):
  if rc != 0:
    msg = lib().odw_last_error(ctx)
    raise NativeError(f'{what}: {ERRORS.get(rc, rc)}: {msg.decode() if msg else ""}')


def _arr(a, dtype):
  return np.ascontiguousarray(a, dtype=dtype)


def scene_desc(sc):
  keep = dict(
      prim_type=_arr(sc.prim_type, np.int32), prim_group=_arr(sc.prim_group, np.int32),
      prim_solid=_arr(sc.prim_solid, np.int32), prim_flags=_arr(sc.prim_flags, np.int32),
      prim_xform=_arr(sc.prim_xform, np.float64), prim_params=_arr(sc.prim_params, np.float64),
      prim_cond_off=_arr(sc.prim_cond_off, np.int32), cond_prim=_arr(sc.cond_prim, np.int32),
      cond_inside=_arr(sc.cond_inside, np.int32), group_type=_arr(sc.group_type, np.int32),
      group_ior=_arr(sc.group_ior, np.float64), group_refl=_arr(sc.group_refl, np.float64),
      group_abslen=_arr(sc.group_abslen, np.float64), group_record=_arr(sc.group_record, np.int32),
      group_grating_type=_arr(sc.group_grating_type, np.int32),
      group_grating_lpm=_arr(sc.group_grating_lpm, np.float64),
      group_grating_dir=_arr(sc.group_grating_dir, np.float64),
      group_grating_order=_arr(sc.group_grating_order, np.int32),
      seq_mask=_arr(sc.seq_mask, np.uint64))
  if getattr(sc, 'tri_normals', None) is not None:
    keep_tri = _arr(sc.tri_normals, np.float64).reshape(-1, 9)
    if len(keep_tri) != len(sc.prim_type):
      raise ValueError('tri_normals needs one row of 9 values per primitive')
  d = SceneDescCoef()
  d.n_prims, d.n_conds, d.n_groups = len(keep['prim_type']), len(keep['cond_prim']), len(keep['group_type'])
  for name, typ in SceneDesc._fields_:
    if name in keep:
      setattr(d, name, keep[name].ctypes.data_as(typ))
  d.seq_enabled, d.seq_len, d.ignore_mask = int(sc.seq_enabled), len(keep['seq_mask']), int(sc.ignore_mask)
  if getattr(sc, 'tri_normals', None) is not None:
    keep['tri_normals'] = keep_tri
    d.tri_normals = keep_tri.ctypes.data_as(_pd)
  if getattr(sc, 'tri_edges', None) is not None:
    keep['tri_edges'] = _arr(sc.tri_edges, np.int32)
    if len(keep['tri_edges']) != len(sc.prim_type):
      raise ValueError('tri_edges needs one entry per primitive')
    d.tri_edges = keep['tri_edges'].ctypes.data_as(_pi)
  # the aspheres' polynomial coefficients; the field stays NULL for a scene without one
  if getattr(sc, 'prim_coef', None) is not None:
    keep['prim_coef'] = _arr(sc.prim_coef, np.float64).reshape(-1, ASPH_COEFS)
    if len(keep['prim_coef']) != len(sc.prim_type):
      raise ValueError('prim_coef needs one row of 8 values per primitive')
    d.prim_coef = keep['prim_coef'].ctypes.data_as(_pd)
  return d, keep


def compile_check_chroma(scene, limits, arch=None, source=None):
  """Host only (no GPU): header and code size of the compiled kernel's CHROMA variant (spectral launches) for `scene`
  under its group_disp_kind (`odw_compile_check_chroma`)"""
  d, keep = scene_desc(scene)
  lim = LimitsDesc(float(limits.max_ray_length), int(limits.max_intersections), float(limits.dist_tol),
                   float(limits.power_tol))
  kinds = _arr(scene.group_disp_kind, np.int32)
  buf = C.create_string_buffer(1 << 20)
  size = C.c_uint64(0)
  f = lib().odw_compile_check_chroma
  f.argtypes = [C.POINTER(SceneDescCoef), C.POINTER(LimitsDesc), C.c_char_p, C.POINTER(SourceDesc), _pi, C.c_char_p, C.c_uint64,
                C.POINTER(C.c_uint64)]
  sd, keep_source = source_desc(source) if source is not None else (None, None)
  rc = f(C.byref(d), C.byref(lim), arch.encode() if arch else None, C.byref(sd) if sd is not None else None,
         kinds.ctypes.data_as(_pi), buf, len(buf), C.byref(size))
  check(None, rc, 'odw_compile_check_chroma')
  return buf.value.decode(), int(size.value)


def compile_check_bands(scene, limits, arch=None, source=None, power=False):
  """Host only (no GPU): header and code size of the CHROMA variant that fills the detector's band planes
  (`odw_compile_check_bands`); power: with the power plane"""
  d, keep = scene_desc(scene)
  lim = LimitsDesc(float(limits.max_ray_length), int(limits.max_intersections), float(limits.dist_tol),
                   float(limits.power_tol))
  kinds = _arr(scene.group_disp_kind, np.int32)
  buf = C.create_string_buffer(1 << 20)
  size = C.c_uint64(0)
  f = lib().odw_compile_check_bands
  f.argtypes = [C.POINTER(SceneDescCoef), C.POINTER(LimitsDesc), C.c_char_p, C.POINTER(SourceDesc), _pi, C.c_int32, C.c_char_p,
                C.c_uint64, C.POINTER(C.c_uint64)]
  sd, keep_source = source_desc(source) if source is not None else (None, None)
  rc = f(C.byref(d), C.byref(lim), arch.encode() if arch else None, C.byref(sd) if sd is not None else None,
         kinds.ctypes.data_as(_pi), 1 if power else 0, buf, len(buf), C.byref(size))
  check(None, rc, 'odw_compile_check_bands')
  return buf.value.decode(), int(size.value)


def band_edges_check(edges):
  """Host only (no GPU): `odw_set_detector_bands`' check of the edges, without a context; raises NativeError naming the edge"""
  e = np.ascontiguousarray(edges, np.float64).ravel()
  f = lib().odw_set_detector_bands
  f.argtypes = [C.c_void_p, C.c_int32, _pd]
  check(None, f(None, len(e), e.ctypes.data_as(_pd)), 'odw_set_detector_bands')


def band_index(edges, wavelengths, device=False):
  """The band (int32; -1: none) of every wavelength among `edges` (nm), numpy.histogram's rule (`odw_band_index`); device:
  by the trace kernels' own search on the current GPU, else on the host (no GPU needed)"""
  e = np.ascontiguousarray(edges, np.float64).ravel()
  w = np.ascontiguousarray(wavelengths, np.float64)
  out = np.empty(w.shape, np.int32)
  f = lib().odw_band_index
  f.argtypes = [_pd, C.c_int32, _pd, C.c_uint64, _pi, C.c_int32]
  check(None, f(e.ctypes.data_as(_pd), len(e), w.ctypes.data_as(_pd), w.size, out.ctypes.data_as(_pi), 1 if device else 0), 'odw_band_index')
  return out


def compile_check_fresnel(scene, limits, arch=None, source=None, modes=None):
  """Host only (no GPU): header and code size of the compiled kernel's FRESNEL variant for `scene` under `modes`
  (default: its group_fresnel) (`odw_compile_check_fresnel`); all modes 0: the plain header"""
  d, keep = scene_desc(scene)
  lim = LimitsDesc(float(limits.max_ray_length), int(limits.max_intersections), float(limits.dist_tol),
                   float(limits.power_tol))
  m = _arr(scene.group_fresnel if modes is None else modes, np.int32).reshape(-1)
  if len(m) != scene.n_groups:          # (the entry point reads one mode per group of the scene)
    raise ValueError(f'compile_check_fresnel: {len(m)} modes for a scene of {scene.n_groups} groups')
  buf = C.create_string_buffer(1 << 20)
  size = C.c_uint64(0)
  f = lib().odw_compile_check_fresnel
  f.argtypes = [C.POINTER(SceneDescCoef), C.POINTER(LimitsDesc), C.c_char_p, C.POINTER(SourceDesc), _pi, C.c_char_p, C.c_uint64,
                C.POINTER(C.c_uint64)]
  sd, keep_source = source_desc(source) if source is not None else (None, None)
  rc = f(C.byref(d), C.byref(lim), arch.encode() if arch else None, C.byref(sd) if sd is not None else None,
         m.ctypes.data_as(_pi), buf, len(buf), C.byref(size))
  check(None, rc, 'odw_compile_check_fresnel')
  return buf.value.decode(), int(size.value)


def coating_tables(coating, n_groups=None):
  """(n_layers int32 [G], layers float64 [G, COAT_LAYERS, 2]) of `coating`: such a pair already, the bake's group_coating, or one list of
  (index, thickness_nm) pairs per group (None or empty: no coating).  Counts beyond COAT_LAYERS are kept as they are -- the
  library refuses them by name -- and the rows that fit are filled"""
  if isinstance(coating, np.ndarray) and coating.dtype.names == ('n', 'layers'):        # (the bake's group_coating)
    coating = (coating['n'], coating['layers'])
  if isinstance(coating, tuple) and len(coating) == 2 and np.ndim(coating[0]) == 1 and np.ndim(coating[1]) == 3:
    cnt = _arr(coating[0], np.int32).reshape(-1)
    lay = _arr(coating[1], np.float64).reshape(len(cnt), COAT_LAYERS, 2)
    return cnt, lay
  stacks = [[] if st is None else list(st) for st in coating]
  cnt = np.array([len(st) for st in stacks], dtype=np.int32)
  lay = np.zeros((len(stacks), COAT_LAYERS, 2), dtype=np.float64)
  for g, st in enumerate(stacks):
    for j, (n, d) in enumerate(st[:COAT_LAYERS]):
      lay[g, j] = float(n), float(d)
  return cnt, lay


def compile_check_coating(scene, limits, arch=None, source=None, modes=None, coating=None):
  """Host only (no GPU): header and code size of the compiled kernel's FRESNEL variant for `scene` under `modes` (default:
  its group_fresnel) and the stacks `coating` (default: its group_coating; see coating_tables)
  (`odw_compile_check_coating`); no layer anywhere: compile_check_fresnel's header"""
  d, keep = scene_desc(scene)
  lim = LimitsDesc(float(limits.max_ray_length), int(limits.max_intersections), float(limits.dist_tol),
                   float(limits.power_tol))
  m = _arr(scene.group_fresnel if modes is None else modes, np.int32).reshape(-1)
  if coating is None:
    coating = getattr(scene, 'group_coating', None)
  cnt, lay = coating_tables(coating if coating is not None else [[]] * scene.n_groups)
  if len(m) != scene.n_groups or len(cnt) != scene.n_groups:          # (the entry point reads one row per group of the scene)
    raise ValueError(f'compile_check_coating: {len(m)} modes and {len(cnt)} stacks for a scene of {scene.n_groups} groups')
  buf = C.create_string_buffer(1 << 20)
  size = C.c_uint64(0)
  f = lib().odw_compile_check_coating
  f.argtypes = [C.POINTER(SceneDescCoef), C.POINTER(LimitsDesc), C.c_char_p, C.POINTER(SourceDesc), _pi, _pi, _pd, C.c_char_p, C.c_uint64,
                C.POINTER(C.c_uint64)]
  sd, keep_source = source_desc(source) if source is not None else (None, None)
  rc = f(C.byref(d), C.byref(lim), arch.encode() if arch else None, C.byref(sd) if sd is not None else None,
         m.ctypes.data_as(_pi), cnt.ctypes.data_as(_pi), lay.ctypes.data_as(_pd), buf, len(buf), C.byref(size))
  check(None, rc, 'odw_compile_check_coating')
  return buf.value.decode(), int(size.value)


def coated_reflectance(n1, n2, cos_i, layers, wavelength_nm, entering=True):
  """Host only (no GPU): the unpolarised reflectance of a surface from index n1 to n2 that carries the stack `layers`
  ((index, thickness_nm) pairs from the outside inwards; entering: the ray meets them in that order) at the cosines of
  incidence `cos_i` -- the library's coated_reflectance (`odw_coated_reflectance` without a context)"""
  c = _arr(cos_i, np.float64).reshape(-1)
  lay = _arr(layers, np.float64).reshape(-1, 2) if len(layers) else np.zeros((0, 2))
  out = np.empty(len(c), np.float64)
  f = lib().odw_coated_reflectance
  f.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_int32, C.c_int32, _pd, C.c_double, C.c_uint64, _pd, _pd, C.c_int32]
  check(None, f(None, float(n1), float(n2), 1 if entering else 0, len(lay), lay.ctypes.data_as(_pd) if len(lay) else None,
                float(wavelength_nm), len(c), c.ctypes.data_as(_pd), out.ctypes.data_as(_pd), 0), 'odw_coated_reflectance')
  return out


def coating_check(coating, modes=None):
  """Host only (no GPU): `odw_set_coating`'s validation of the stacks `coating` (see coating_tables; with the groups'
  Fresnel modes where given); raises NativeError naming the group"""
  cnt, lay = coating_tables(coating)
  m = _arr(modes, np.int32).reshape(-1) if modes is not None else None
  f = lib().odw_coating_check
  f.argtypes = [C.c_int32, _pi, _pd, _pi]
  check(None, f(len(cnt), cnt.ctypes.data_as(_pi), lay.ctypes.data_as(_pd), m.ctypes.data_as(_pi) if m is not None else None),
        'odw_coating_check')


def fresnel_reflectance(n1, n2, cos_i):
  """Host only (no GPU): the unpolarised reflectance of a surface from index n1 to n2 at the cosines of incidence
  `cos_i` -- the library's fresnel_reflectance (`odw_fresnel_reflectance` without a context); 1 beyond the critical angle"""
  c = _arr(cos_i, np.float64).reshape(-1)
  out = np.empty(len(c), np.float64)
  f = lib().odw_fresnel_reflectance
  f.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_uint64, _pd, _pd, C.c_int32]
  check(None, f(None, float(n1), float(n2), len(c), c.ctypes.data_as(_pd), out.ctypes.data_as(_pd), 0), 'odw_fresnel_reflectance')
  return out


def fresnel_check(modes, group_types=None):
  """Host only (no GPU): `odw_set_fresnel`'s validation of `modes` (with the groups' ODW_OPT_* types where given);
  raises NativeError naming the group"""
  m = _arr(modes, np.int32).reshape(-1)
  t = _arr(group_types, np.int32).reshape(-1) if group_types is not None else None
  f = lib().odw_fresnel_check
  f.argtypes = [C.c_int32, _pi, _pi]
  check(None, f(len(m), m.ctypes.data_as(_pi), t.ctypes.data_as(_pi) if t is not None else None), 'odw_fresnel_check')


def compile_check(scene, limits, mode='structure', arch=None, source=None):
  """Host only (no GPU): the header of constants the library writes for `scene` and the size of the
  code object hiprtc builds from it for `arch` (default gfx950).  Raises NativeError when the scene
  is outside the flat kernel's domain or the compilation fails.  source: a baked point source -- the kernel
  a launch binds that generates its rays from it (ray generation compiled against the source's structure);
  None: the source-free kernel of explicit rays and batches."""
  d, keep = scene_desc(scene)
  lim = LimitsDesc(float(limits.max_ray_length), int(limits.max_intersections), float(limits.dist_tol),
                   float(limits.power_tol))
  buf = C.create_string_buffer(1 << 20)
  size = C.c_uint64(0)
  f = lib().odw_compile_check_source
  f.argtypes = [C.POINTER(SceneDescCoef), C.POINTER(LimitsDesc), C.c_int32, C.c_char_p, C.POINTER(SourceDesc), C.c_char_p,
                C.c_uint64, C.POINTER(C.c_uint64)]
  sd, keep_source = source_desc(source) if source is not None else (None, None)
  rc = f(C.byref(d), C.byref(lim), COMPILE_MODES[mode], arch.encode() if arch else None,
         C.byref(sd) if sd is not None else None, buf, len(buf), C.byref(size))
  check(None, rc, 'odw_compile_check')
  return buf.value.decode(), int(size.value)


STRUCTURES = {0: 'flat', 1: 'grid', 2: 'bvh', 3: 'wide-bvh'}


def build_check(scene, limits, library=None):
  """Host only (no GPU): what the library will trace `scene` with -- 'flat' loop, rectilinear 'grid', binary 'bvh' or the
  eight-wide tree of the mesh kernel --, after building it in host memory (`odw_build_check`), and the sizes it reports"""
  d, keep = scene_desc(scene)
  lim = LimitsDesc(float(limits.max_ray_length), int(limits.max_intersections), float(limits.dist_tol),
                   float(limits.power_tol))
  structure = C.c_int32(-1)
  sizes = (C.c_uint64 * 6)()
  f = (library or lib()).odw_build_check
  f.argtypes = [C.POINTER(SceneDescCoef), C.POINTER(LimitsDesc), C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]
  rc = f(C.byref(d), C.byref(lim), C.byref(structure), sizes)
  if rc != 0:
    msg = (library or lib()).odw_last_error(None)
    raise NativeError(f'odw_build_check: {ERRORS.get(rc, rc)}: {msg.decode() if msg else ""}')
  names = ('primitives', 'nodes', 'grid_cells', 'grid_items', 'grid_lds_bytes', 'dead_primitives')
  return dict(structure=STRUCTURES[int(structure.value)], **{k: int(v) for k, v in zip(names, sizes)})


def spec_image(scene, limits):
  """Host only (no GPU): the value image of the kernel compiled against `scene` (`odw_spec_image`: the block of doubles its
  unrolled loop reads) for `limits`, and its layout -> dict(image, boxes, gf, gd, gi, frame, par, box, der, box_of, in_arguments);
  frame ... box_of: one entry per primitive, offsets into image (-1: none)"""
  d, keep = scene_desc(scene)
  lim = LimitsDesc(float(limits.max_ray_length), int(limits.max_intersections), float(limits.dist_tol),
                   float(limits.power_tol))
  f = lib().odw_spec_image
  f.argtypes = [C.POINTER(SceneDescCoef), C.POINTER(LimitsDesc), _pd, C.c_uint64, C.POINTER(C.c_uint64), _pi, C.c_uint64,
                _pd, C.POINTER(C.c_int32)]
  size, inside = C.c_uint64(0), C.c_int32(0)
  check(None, f(C.byref(d), C.byref(lim), None, 0, C.byref(size), None, 0, None, C.byref(inside)), 'odw_spec_image')
  image = np.zeros(int(size.value), np.float64)
  n = int(d.n_prims)
  offsets = np.zeros(3 + 5 * n, np.int32)
  boxes = np.zeros((n, 6), np.float64)
  check(None, f(C.byref(d), C.byref(lim), image.ctypes.data_as(_pd), image.size, C.byref(size), offsets.ctypes.data_as(_pi),
                offsets.size, boxes.ctypes.data_as(_pd), C.byref(inside)), 'odw_spec_image')
  per = offsets[3:].reshape(n, 5)
  return dict(image=image, boxes=boxes, gf=int(offsets[0]), gd=int(offsets[1]), gi=int(offsets[2]), frame=per[:, 0].copy(),
              par=per[:, 1].copy(), box=per[:, 2].copy(), der=per[:, 3].copy(), box_of=per[:, 4].copy(),
              in_arguments=bool(inside.value))


def table_slopes(cdf, edges):
  """Host only (no GPU): the segment slopes the library stores behind the (cdf, edge) pairs of an inverse-CDF table
  (`odw_table_slopes`): one row per row of `cdf`, the last knot of a row 0"""
  edges = _arr(edges, np.float64)
  cdf = _arr(cdf, np.float64).reshape(-1, len(edges))
  out = np.empty_like(cdf)
  f = lib().odw_table_slopes
  f.argtypes = [_pd, _pd, C.c_int32, C.c_int32, _pd]
  rc = f(cdf.ctypes.data_as(_pd), edges.ctypes.data_as(_pd), cdf.shape[0], cdf.shape[1], out.ctypes.data_as(_pd))
  check(None, rc, 'odw_table_slopes')
  return out


def dispersion_index(kind, coef, wavelengths):
  """Host only (no GPU): the index of the glass (kind: 'Sellmeier' / 'Cauchy' or ODW_DISP_*, coef: up to 6 numbers) at
  `wavelengths` (nm) -- the library's disp_index (`odw_dispersion_index` without a context)"""
  k = DISP_KINDS[kind] if isinstance(kind, str) else int(kind)
  c = np.zeros(DISP_COEFS, np.float64)
  cc = np.asarray(coef, dtype=np.float64).reshape(-1)
  if len(cc) > DISP_COEFS:
    raise ValueError('DispersionCoefficients: at most 6 numbers')
  c[:len(cc)] = cc
  w = _arr(wavelengths, np.float64).reshape(-1)
  out = np.empty(len(w), np.float64)
  f = lib().odw_dispersion_index
  f.argtypes = [C.c_void_p, C.c_int32, C.c_int32, _pd, C.c_uint64, _pd, _pd, C.c_int32]
  check(None, f(None, 0, k, c.ctypes.data_as(_pd), len(w), w.ctypes.data_as(_pd), out.ctypes.data_as(_pd), 0), 'odw_dispersion_index')
  return out


def dispersion_check(kind, coef, lo_nm, hi_nm):
  """Host only (no GPU): the checks a launch runs on a dispersion (`odw_dispersion_check`): kinds and coefficients, then
  every index finite and >= 1 and no Sellmeier pole over [lo_nm, hi_nm].  Raises NativeError naming the group."""
  k = _arr(kind, np.int32).reshape(-1)
  c = _arr(coef, np.float64).reshape(len(k), DISP_COEFS)
  f = lib().odw_dispersion_check
  f.argtypes = [C.c_int32, _pi, _pd, C.c_double, C.c_double]
  check(None, f(len(k), k.ctypes.data_as(_pi), c.ctypes.data_as(_pd), float(lo_nm), float(hi_nm)), 'odw_dispersion_check')


def spectrum_check(mode, wavelengths, cdf):
  """Host only (no GPU): `odw_set_spectrum`'s validation of a table; raises NativeError"""
  w, c = _arr(wavelengths, np.float64).reshape(-1), _arr(cdf, np.float64).reshape(-1)
  if len(w) != len(c):
    raise ValueError('Spectrum: wavelengths and cdf differ in length')
  f = lib().odw_spectrum_check
  f.argtypes = [C.c_int32, C.c_int32, _pd, _pd]
  check(None, f(SPECTRUM_MODES.get(mode, mode), len(w), w.ctypes.data_as(_pd), c.ctypes.data_as(_pd)), 'odw_spectrum_check')


def source_desc(src):
  t = src.tables
  keep = dict(phi_edges=_arr(t.phi_edges, np.float64), phi_cdf=_arr(t.phi_cdf, np.float64),
              t_edges=_arr(t.t_edges, np.float64), t_cdf=_arr(t.t_cdf, np.float64).reshape(-1, len(t.t_edges)))
  d = SourceDesc()
  d.xform = (C.c_double * 12)(*np.asarray(src.xform, dtype=np.float64).reshape(12))
  d.focal_length, d.wavelength, d.power = float(src.focal_length), float(src.wavelength), float(src.power)
  d.n_phi_knots, d.n_t_knots, d.n_t_rows = len(keep['phi_edges']), len(keep['t_edges']), keep['t_cdf'].shape[0]
  for name in keep:
    setattr(d, name, keep[name].ctypes.data_as(_pd))
  return d, keep


def surface_sampler_descs(samplers):
  """array of odw_surface_sampler_desc for scene.surface_samplers"""
  samplers = list(samplers or [])
  arr = (SurfaceSamplerDesc * max(1, len(samplers)))()
  keep = [arr]
  for d, s in zip(arr, samplers):
    phi_edges, phi_cdf = _arr(s.phi_edges, np.float64), _arr(s.phi_cdf, np.float64)
    t_edges, t_cdf = _arr(s.t_edges, np.float64), _arr(s.t_cdf, np.float64)
    keep += [phi_edges, phi_cdf, t_edges, t_cdf]
    d.group, d.kind, d.family_axis, d.n_family = int(s.group), int(s.kind), int(s.axis), int(s.n_family)
    d.family_lo, d.family_hi = float(s.lo), float(s.hi)
    d.n_phi_knots, d.n_t_knots, d.n_t_rows = len(phi_edges), len(t_edges), int(t_cdf.shape[-2])
    for name, a in (('phi_edges', phi_edges), ('phi_cdf', phi_cdf), ('t_edges', t_edges), ('t_cdf', t_cdf)):
      setattr(d, name, a.ctypes.data_as(_pd))
    d.mu = float(getattr(s, 'mu', 0.0))
    d.n_atoms = int(getattr(s, 'n_atoms', 0) or 0)
    if d.n_atoms:
      for name in ('atom_mass', 'atom_theta', 'atom_phi'):
        a = _arr(getattr(s, name), np.float64)
        keep.append(a)
        setattr(d, name, a.ctypes.data_as(_pd))
  return arr, len(samplers), keep


def surface_source_desc(src):
  """odw_surface_source_desc for a freecad_elements.surface_source.BakedSurfaceSource"""
  keep = dict(prim_type=_arr(src.prim_type, np.int32), prim_flags=_arr(src.prim_flags, np.int32),
              prim_xform=_arr(src.prim_xform, np.float64), prim_params=_arr(src.prim_params, np.float64),
              prim_cond_off=_arr(src.prim_cond_off, np.int32),
              cond_prim=_arr(src.cond_prim if len(src.cond_prim) else [0], np.int32),
              cond_inside=_arr(src.cond_inside if len(src.cond_inside) else [0], np.int32),
              face_prim=_arr(src.face_prim, np.int32), face_id=_arr(src.face_id, np.int32),
              face_area=_arr(src.face_area, np.float64), t_edges=_arr(src.t_edges, np.float64),
              t_cdf=_arr(src.t_cdf, np.float64))
  if getattr(src, 'tri_normals', None) is not None:
    keep['tri_normals'] = _arr(src.tri_normals, np.float64).reshape(-1, 9)
    if len(keep['tri_normals']) != len(keep['prim_type']):
      raise ValueError('tri_normals needs one row of 9 values per primitive')
  d = SurfaceSourceDesc()
  d.wavelength, d.power, d.dist_tol = float(src.wavelength), float(src.power), float(src.dist_tol)
  d.n_prims, d.n_conds, d.n_faces = len(keep['prim_type']), len(src.cond_prim), len(keep['face_prim'])
  d.n_t_knots = len(keep['t_edges'])
  for name, typ in SurfaceSourceDesc._fields_:
    if name in keep:
      setattr(d, name, keep[name].ctypes.data_as(typ))
  return d, keep
