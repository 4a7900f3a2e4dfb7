"""Dispersion of a group and spectrum of a point source on the host (no GPU): the library's disp_index against the
numpy sequence bit for bit, the catalogue numbers of N-BK7, glassFromAbbe, the bake's tables, the spectrum tables,
and every refusal with its name in the message."""
import copy

import numpy as np
import pytest

import spectral_cases as sp
from freecad.optics_design_workbench_amd import _native
from freecad.optics_design_workbench_amd.distributions import ScalarRandomVariable
from freecad.optics_design_workbench_amd.freecad_elements import make, point_source
from freecad.optics_design_workbench_amd.scene import bake

WAVELENGTHS = np.linspace(350.0, 2000.0, 1000)


def test_bk7_against_the_catalogue():
  n = sp.sellmeier(sp.BK7, np.array(sp.LINES))
  assert np.abs(n - np.array(sp.BK7_CATALOGUE)).max() < 5e-6, n
  abbe = (n[1] - 1.0) / (n[0] - n[2])
  assert abs(abbe - sp.BK7_ABBE) < 5e-3, abbe          # (the catalogue prints two decimals)
  assert abs(abbe - 64.167) < 1e-3


@pytest.mark.parametrize('kind,coef', [('Sellmeier', sp.BK7), ('Cauchy', sp.FLINT['DispersionCoefficients']),
                                       ('Cauchy', [1.5046, 0.00420])])
def test_host_index_is_the_numpy_sequence_bit_for_bit(kind, coef):
  got = _native.dispersion_index(kind, coef, WAVELENGTHS)
  want = sp.index(kind, coef, WAVELENGTHS)
  assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), np.abs(got - want).max()


def test_glass_from_abbe():
  g = make.glassFromAbbe(1.5168, 64.17)
  assert g['Dispersion'] == 'Cauchy' and g['RefractiveIndex'] == 1.5168
  nF, nd, nC = _native.dispersion_index('Cauchy', g['DispersionCoefficients'], sp.LINES)
  assert abs(nd - 1.5168) < 1e-12
  assert abs((nd - 1.0) / (nF - nC) - 64.17) < 1e-9
  with pytest.raises(ValueError, match='glassFromAbbe'):
    make.glassFromAbbe(1.5, -3.0)


def test_bake_tables():
  sc, lim, src = sp.scene(dispersive=True)
  assert sc.group_disp_kind.dtype == np.int32 and sc.group_disp.dtype == np.float64
  assert sc.group_disp_kind.tolist() == [1, 2, 0, 0] and sc.group_disp.shape == (4, 6)
  assert sc.group_disp[0].tolist() == sp.BK7
  assert sc.group_disp[1].tolist() == sp.FLINT['DispersionCoefficients'] + [0.0, 0.0, 0.0]
  assert not sc.group_disp[2:].any()
  # a document without Dispersion bakes kind 0 everywhere, and every other table byte for byte what it was
  plain, _, _ = sp.scene(dispersive=False)
  assert not plain.group_disp_kind.any() and not plain.group_disp.any()
  for name in ('prim_type', 'prim_group', 'prim_solid', 'prim_flags', 'prim_xform', 'prim_params', 'prim_cond_off', 'cond_prim',
               'cond_inside', 'group_type', 'group_ior', 'group_refl', 'group_abslen', 'group_record', 'group_grating_type',
               'group_grating_lpm', 'group_grating_dir', 'group_grating_order', 'seq_mask'):
    a, b = np.asarray(getattr(sc, name)), np.asarray(getattr(plain, name))
    assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), name
  assert sc.group_ior.tolist() == [1.5168, 1.62, 2.0, 2.0]          # group_ior stays what it is
  # the descriptor the library (and the oracle) reads does not know the new tables
  d, keep = _native.scene_desc(sc)
  assert not any('disp' in name for name, _ in type(d)._fields_)


@pytest.mark.parametrize('props,word', [
    (dict(Dispersion='Schott'), 'Dispersion'),
    (dict(Dispersion='Sellmeier', DispersionCoefficients=[1.0, 2.0, 3.0]), 'DispersionCoefficients'),
    (dict(Dispersion='Sellmeier', DispersionCoefficients=[1.0] * 8), 'DispersionCoefficients'),        # more than three terms
    (dict(Dispersion='Cauchy', DispersionCoefficients=[1.5, np.inf, 0.0]), 'non-finite'),
])
def test_bake_refuses_by_name(props, word):
  groups = [('Lens', lambda d: [make.makeBox(d, 'B', 10, 10, 10)], props)]
  doc, src = sp.document(groups_=groups)
  with pytest.raises(ValueError, match=word):
    bake.bakeScene(doc, src)


def test_bake_refuses_dispersion_on_a_mirror():
  groups = [('Mirror', lambda d: [make.makeBox(d, 'B', 10, 10, 10)], dict(make.N_BK7))]
  doc, src = sp.document(groups_=groups)
  with pytest.raises(ValueError, match='neither a lens nor a transmission grating'):
    bake.bakeScene(doc, src)


# ---- spectrum tables ---------------------------------------------------------------------------------------------------
def source_with(**props):
  doc, src = sp.document(source=props)
  return src


def test_spectrum_lines():
  s = point_source.bakeSpectrum(source_with(Spectrum=[(486.1327, 1.0), (587.5618, 2.0), (656.2725, 1.0)]))
  assert s.mode == 'lines' and s.wavelengths.tolist() == list(sp.LINES)
  assert s.cdf.tolist() == [0.25, 0.75, 1.0]
  _native.spectrum_check('lines', s.wavelengths, s.cdf)
  u = np.array([0.0, 0.2499999, 0.25, 0.7499999, 0.75, 0.9999999])
  assert s.wavelengthOf(u).tolist() == [sp.LINES[0], sp.LINES[0], sp.LINES[1], sp.LINES[1], sp.LINES[2], sp.LINES[2]]
  assert point_source.bakeSpectrum(source_with()) is None
  with pytest.raises(ValueError, match='Spectrum: wavelengths must be strictly ascending'):
    point_source.bakeSpectrum(source_with(Spectrum=[(600.0, 1.0), (500.0, 1.0)]))
  with pytest.raises(ValueError, match='Spectrum: weights'):
    point_source.bakeSpectrum(source_with(Spectrum=[(500.0, 0.0), (600.0, 0.0)]))


def test_spectrum_density_is_the_scalar_variable_s_table():
  density, lo, hi = 'exp(-(wavelength-550)^2/(2*40^2))', 450.0, 700.0
  s = point_source.bakeSpectrum(source_with(SpectralDensity=density, SpectrumDomain='450, 700', SpectrumResolution='1e3'))
  edges, cdf = ScalarRandomVariable(density, (lo, hi), variable='wavelength', numericalResolution=1e3).tables()
  assert s.mode == 'density' and np.array_equal(s.wavelengths, edges) and np.array_equal(s.cdf, cdf)
  assert s.cdf[0] == 0.0 and s.cdf[-1] == 1.0 and len(s.cdf) == 1001
  _native.spectrum_check('density', s.wavelengths, s.cdf)
  default = point_source.bakeSpectrum(source_with(SpectralDensity='1', SpectrumDomain='400, 800'))
  assert len(default.cdf) == 10001                     # SpectrumResolution defaults to 1e4 (odd knot count)


def test_both_spectrum_properties_at_once():
  with pytest.raises(ValueError, match='Spectrum and SpectralDensity are both set'):
    point_source.bakeSpectrum(source_with(Spectrum=[(500.0, 1.0)], SpectralDensity='1', SpectrumDomain='400, 800'))
  with pytest.raises(ValueError, match='SpectrumDomain'):
    point_source.bakeSpectrum(source_with(SpectralDensity='1'))


@pytest.mark.parametrize('mode,wl,cdf,word', [
    ('lines', [600.0, 500.0], [0.5, 1.0], 'not ascending'),
    ('lines', [0.0, 500.0], [0.5, 1.0], '> 0'),
    ('lines', [500.0, 600.0], [0.5, 0.9], 'run from 0 to 1'),
    ('lines', [500.0, 600.0], [0.7, 0.5], 'not monotone'),
    ('density', [500.0, 600.0, 700.0], [0.1, 0.5, 1.0], 'run from 0 to 1'),
    ('density', [500.0, 600.0, 700.0], [0.0, 0.6, 0.5], 'not monotone'),
    ('density', [500.0], [1.0], 'bad argument'),
])
def test_library_refuses_spectrum_tables(mode, wl, cdf, word):
  with pytest.raises(_native.NativeError, match=word):
    _native.spectrum_check(mode, wl, cdf)


def test_library_refuses_dispersions():
  bk7 = np.array(sp.BK7)
  ok = np.zeros((2, 6))
  ok[1] = bk7
  _native.dispersion_check([0, 1], ok, 350.0, 2000.0)
  with pytest.raises(_native.NativeError, match='group 1: unknown dispersion kind 3'):
    _native.dispersion_check([0, 3], ok, 500.0, 600.0)
  bad = ok.copy()
  bad[1, 2] = np.nan
  with pytest.raises(_native.NativeError, match='group 1: non-finite dispersion coefficient'):
    _native.dispersion_check([0, 1], bad, 500.0, 600.0)
  # N-BK7's ultraviolet poles: sqrt(C1) = 77.46 nm, sqrt(C2) = 141.5 nm; the infrared one at 10.18 um
  with pytest.raises(_native.NativeError, match='group 1: Sellmeier pole at 141.4'):
    _native.dispersion_check([0, 1], ok, 120.0, 400.0)
  with pytest.raises(_native.NativeError, match='group 1: Sellmeier pole at 10176'):
    _native.dispersion_check([0, 1], ok, 9000.0, 11000.0)
  # no index at all: below the first pole the Sellmeier sum is negative (1 - 1.56 - 0.05 at 60 nm), its root NaN
  with pytest.raises(_native.NativeError, match=r'group 1: index .* \(must be finite and >= 1\)'):
    _native.dispersion_check([0, 1], ok, 60.0, 70.0)
  low = np.zeros((1, 6))
  low[0, :3] = [0.9, 0.001, 0.0]
  with pytest.raises(_native.NativeError, match='group 0: index'):
    _native.dispersion_check([2], low, 500.0, 600.0)
  with pytest.raises(_native.NativeError, match='wavelengths must be finite and > 0'):
    _native.dispersion_check([0, 1], ok, 0.0, 600.0)
  # without a context the index needs a formula
  with pytest.raises(_native.NativeError, match='needs a dispersion kind'):
    _native.dispersion_index(0, bk7, [500.0])


def test_compiled_chroma_header():
  """the compiled kernel's variant for spectral launches: Spec::chroma(), a constexpr Spec::disp(G) per group and the place
  of its coefficients in the value image are in the emitted header -- the cache key --, the variant compiles for gfx950,
  and the header of every other launch does not know about any of it"""
  sc, lim, src = sp.scene()
  h, n = _native.compile_check_chroma(sc, lim, source=src)
  assert 'static constexpr bool chroma() { return true; }' in h and '#define ODW_SPEC_CHROMA true' in h and n > 10000
  assert 'static constexpr int disp(int i) { constexpr int T[] = {1, 2, 0, 0}; return T[i]; }' in h
  img = int(h.split('static constexpr int IMG = ')[1].split(';')[0])
  plain, _ = _native.compile_check(sc, lim, 'structure', source=src)
  assert 'chroma' not in plain and 'CHROMA' not in plain
  img0 = int(plain.split('static constexpr int IMG = ')[1].split(';')[0])
  assert img == img0 + 12                                  # six words per dispersive group, behind everything else
  assert f'static constexpr int dc(int i) {{ constexpr int T[] = {{{img0}, {img0 + 6}, -1, -1}}; return T[i]; }}' in h
  other = copy.copy(sc)
  other.group_disp_kind = np.array([2, 0, 0, 0], dtype=np.int32)
  h2, _ = _native.compile_check_chroma(other, lim, source=src)
  assert h2 != h and 'T[] = {2, 0, 0, 0}' in h2


def test_cauchy_dip_between_samples_is_found():
  """n = A + B x + C x^2 in x = 1 / lambda^2 has its extremum at x = -B / (2 C): judged there exactly, not by samples"""
  # a dip to 0.99 at 600 nm, 0.2 nm wide at n = 1: between the 33 samples of [410, 2010] nm (50 nm apart: 560, 610)
  x0 = 1.0 / 0.6 ** 2
  k = 0.01 / (1.0 / 0.5999 ** 2 - x0) ** 2
  coef = np.zeros((1, 6))
  coef[0, :3] = [0.99 + k * x0 * x0, -2.0 * k * x0, k]
  assert abs(sp.cauchy(coef[0], 600.0) - 0.99) < 1e-6 and sp.cauchy(coef[0], 599.8) > 1.0 and sp.cauchy(coef[0], 600.2) > 1.0
  with pytest.raises(_native.NativeError, match=r'group 0: index 0\.99.* at 600'):
    _native.dispersion_check([2], coef, 410.0, 2010.0)
  _native.dispersion_check([2], coef, 710.0, 2010.0)


def test_symbols_and_abi():
  new = ('odw_set_dispersion', 'odw_set_spectrum', 'odw_trace_rays_spectral', 'odw_ray_wavelengths', 'odw_dispersion_index',
         'odw_dispersion_check', 'odw_spectrum_check', 'odw_compiled_chroma_info', 'odw_compile_check_chroma')
  header = open(_native._HEADER).read()
  for name in new:
    assert name in _native.SYMBOLS and hasattr(_native.lib(), name)
    assert f'int {name}(' in header, name
  assert _native.lib().odw_abi_version() == 12
  # the stream word of the wavelength draw is named in the device header, and no other draw uses it
  device = open(_native.CSRC + '/odw_device.h').read()
  assert '#define ODW_STREAM_WAVELENGTH 6u' in device and _native.STREAM_WAVELENGTH == 6
  kernels = open(_native.CSRC + '/odw_kernels.hip').read()
  used = {0, 1, 2, 17, 18, 3, 4, 5}             # generation; 1 + kind, 17 + kind (surface draws); the emitter
  for word, text in ((0, 'c2 = 0u, c3 = 0u'), (1, '1u + ODW_SURF_PRIMARY'), (2, '1u + ODW_SURF_MODIFY'), (17, 'm3 = stream + 16u'),
                     (3, 'attempt, 3u'), (4, 'attempt, 4u'), (5, '0u, 5u')):
    assert text in kernels, word
  assert _native.STREAM_WAVELENGTH not in used
