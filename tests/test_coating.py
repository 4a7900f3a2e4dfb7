"""Thin-film coatings on lens groups, the parts that need no GPU: the coated reflectance on the host
(`odw_coated_reflectance` without a context) against numpy's complex characteristic matrices and against closed forms, the
validation (`odw_coating_check`) and the bake's `group_coating` with their refusals, the property in a document read from
an FCStd file, and the header of the compiled kernel's COAT variant (hiprtc for gfx950)."""
import os

import numpy as np
import pytest

import coating_cases as cc
import fresnel_cases as fc
from conftest import SCENES
from freecad.optics_design_workbench_amd import _native
from freecad.optics_design_workbench_amd.freecad_elements import make
from freecad.optics_design_workbench_amd.scene import Document, bake, fcstd, open_fcstd
from test_dispersion_fcstd import _with_properties

TOL = 1e-12                     # the project's tolerance for the bare reflectance
ENTERING = np.cos(np.radians(np.linspace(0.0, 85.0, 86)))
LEAVING = np.cos(np.radians(np.linspace(0.0, 41.0, 42)))     # below the critical 41.81 degrees of glass 1.5


# ---- the host twin against numpy -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('stack', ['Q', 'V', 'W'])
def test_grid_against_numpy(native_lib, stack):
  """entering at 0 .. 85 degrees, leaving at 0 .. 41 degrees (the smallest root on that grid is 0.0316: no angle is left
  out), at 450, 550 and 650 nm"""
  layers = cc.STACKS[stack]
  assert abs(fc.root_of(cc.N_GLASS, 1.0, LEAVING).min() - 0.0316) < 1e-4
  for wl in cc.LINES:
    for n1, n2, cos_i, entering in ((1.0, cc.N_GLASS, ENTERING, True), (cc.N_GLASS, 1.0, LEAVING, False)):
      got = _native.coated_reflectance(n1, n2, cos_i, layers, wl, entering)
      want = cc.reflectance(n1, n2, cos_i, layers, wl, entering)
      err = np.abs(got - want).max()
      print(f'{stack} {wl:.0f} nm {"entering" if entering else "leaving"}: largest difference {err:.3g}')
      assert err < TOL
      assert np.all((got >= 0) & (got <= 1))


@pytest.mark.parametrize('stack', ['Q', 'V', 'W'])
def test_normal_incidence_values(native_lib, stack):
  got = [_native.coated_reflectance(1.0, cc.N_GLASS, [1.0], cc.STACKS[stack], wl)[0] for wl in cc.LINES]
  ref = [cc.reflectance(1.0, cc.N_GLASS, [1.0], cc.STACKS[stack], wl)[0] for wl in cc.LINES]
  assert np.abs(np.array(got) - cc.R_NORMAL[stack]).max() < 5e-9 and np.abs(np.array(ref) - cc.R_NORMAL[stack]).max() < 5e-9


def test_closed_forms(native_lib):
  # a quarter wave at its wavelength
  assert abs(cc.R_Q_550 - 0.014110458641778) < 1e-15
  assert abs(_native.coated_reflectance(1.0, 1.5, [1.0], cc.Q, 550.0)[0] - cc.R_Q_550) < TOL
  # a layer of no thickness: the bare surface
  for n1, n2, cos_i, entering in ((1.0, 1.5, ENTERING, True), (1.5, 1.0, LEAVING, False)):
    bare = _native.fresnel_reflectance(n1, n2, cos_i)
    assert np.abs(_native.coated_reflectance(n1, n2, cos_i, [(1.38, 0.0)], 550.0, entering) - bare).max() < 1e-15
    assert np.array_equal(_native.coated_reflectance(n1, n2, cos_i, [], 550.0, entering), bare)
  # a half wave at normal incidence: absent
  assert abs(_native.coated_reflectance(1.0, 1.5, [1.0], [(1.38, 550.0 / 2 / 1.38)], 550.0)[0] - 0.04) < TOL
  # the stack seen from the other side at the same transverse wave vector: entering at i, leaving at the refracted angle
  cos_t = np.sqrt(1.0 - (1.0 - ENTERING ** 2) / 1.5 ** 2)
  for layers in cc.STACKS.values():
    for wl in cc.LINES:
      a = _native.coated_reflectance(1.0, 1.5, ENTERING, layers, wl, True)
      b = _native.coated_reflectance(1.5, 1.0, cos_t, layers, wl, False)
      assert np.abs(a - b).max() < TOL
  # total reflection: 1, whatever the stack
  assert np.all(_native.coated_reflectance(1.5, 1.0, np.cos(np.radians([42.0, 60.0, 89.0])), cc.W, 550.0, False) == 1.0)


def test_orientation_matters(native_lib):
  """V at 450 nm from the glass: met in reverse 0.0075; met in listed order -- the forgotten reversal -- 0.1716"""
  right = _native.coated_reflectance(1.5, 1.0, [1.0], cc.V, 450.0, False)[0]
  wrong = _native.coated_reflectance(1.5, 1.0, [1.0], cc.V, 450.0, True)[0]
  assert abs(right - cc.reflectance(1.5, 1.0, [1.0], cc.V[::-1], 450.0, True)[0]) < TOL
  assert abs(right - 0.0075) < 1e-4 and abs(wrong - 0.1716) < 1e-4 and wrong - right > 0.1


def test_evanescent_layer_takes_the_bare_reflectance(native_lib):
  """glass 1.7 against glass 1.6 with a layer of 1.38 between: beyond 54.27 degrees the layer would hold an evanescent wave,
  up to 70.25 degrees the surface itself does not reflect totally"""
  cos_i = np.cos(np.radians(np.linspace(56.0, 69.0, 14)))
  got = _native.coated_reflectance(1.7, 1.6, cos_i, [(1.38, 100.0)], 550.0)
  bare = _native.fresnel_reflectance(1.7, 1.6, cos_i)
  assert np.array_equal(got, bare) and np.all(bare < 1.0)
  below = np.cos(np.radians([10.0, 50.0]))
  assert np.all(_native.coated_reflectance(1.7, 1.6, below, [(1.38, 100.0)], 550.0) != _native.fresnel_reflectance(1.7, 1.6, below))


# ---- validation ----------------------------------------------------------------------------------------------------------
def test_validation_of_the_library(native_lib):
  _native.coating_check([[], cc.Q, cc.W], [0, 1, 2])
  _native.coating_check([[], cc.Q, cc.W])                                    # (no modes at hand)
  _native.coating_check([[(1.0, 0.0)] * 4], [1])
  with pytest.raises(_native.NativeError, match='group 1: a coating on a group without a Fresnel mode'):
    _native.coating_check([[], cc.Q], [1, 0])
  with pytest.raises(_native.NativeError, match=r'group 0: 5 layers \(a coating has at most 4\)'):
    _native.coating_check([[(1.38, 100.0)] * 5], [1])
  with pytest.raises(_native.NativeError, match=r'group 1: layer 1: index 0.9 \(finite and at least 1\)'):
    _native.coating_check([[], [(1.38, 100.0), (0.9, 100.0)]], [0, 1])
  for bad in (np.nan, np.inf):
    with pytest.raises(_native.NativeError, match='group 0: layer 0: index'):
      _native.coating_check([[(bad, 100.0)]], [1])
    with pytest.raises(_native.NativeError, match='group 0: layer 0: thickness'):
      _native.coating_check([[(1.38, bad)]], [1])
  with pytest.raises(_native.NativeError, match=r'group 0: layer 0: thickness -1 nm \(finite and not negative\)'):
    _native.coating_check([[(1.38, -1.0)]], [1])
  # the reflectance entry point checks its stack likewise
  with pytest.raises(_native.NativeError, match='5 layers'):
    _native.coated_reflectance(1.0, 1.5, [1.0], [(1.38, 100.0)] * 5, 550.0)
  with pytest.raises(_native.NativeError, match='index 0.9'):
    _native.coated_reflectance(1.0, 1.5, [1.0], [(0.9, 100.0)], 550.0)
  with pytest.raises(_native.NativeError, match='odw_coated_reflectance: bad argument'):
    _native.coated_reflectance(1.0, 1.5, [1.0], cc.Q, 0.0)
  # ... and so does the compile check
  sc, lim, _ = cc.slab('Loss')
  with pytest.raises(_native.NativeError, match='group 0: a coating on a group without a Fresnel mode'):
    _native.compile_check_coating(sc, lim, coating=[cc.Q, cc.Q, []])
  with pytest.raises(ValueError, match='3 modes and 2 stacks for a scene of 3 groups'):
    _native.compile_check_coating(sc, lim, coating=[[], cc.Q])


def _one_lens(**props):
  doc = Document()
  make.makeLens(doc, [make.makeBox(doc, 'B', 1, 1, 1)], name='G_', **props)
  make.makeSimulationSettings(doc)
  return doc, make.makePointSource(doc)


@pytest.mark.parametrize('props, message', [
    (dict(Coating=cc.Q), 'G_: Coating on a group without a Fresnel mode'),
    (dict(Fresnel='Loss', Coating=[(1.38, 100.0)] * 5), r'G_: Coating: 5 layers \(at most 4\)'),
    (dict(Fresnel='Loss', Coating=[(0.9, 100.0)]), r'G_: Coating: layer 0: index 0.9 \(finite and at least 1\)'),
    (dict(Fresnel='Split', Coating=[(1.38, 100.0), (float('nan'), 1.0)]), 'G_: Coating: layer 1: index nan'),
    (dict(Fresnel='Loss', Coating=[(1.38, -2.0)]), r'G_: Coating: layer 0: thickness -2 nm \(finite and not negative\)'),
    (dict(Fresnel='Loss', Coating=[(1.38, float('inf'))]), 'G_: Coating: layer 0: thickness inf nm'),
    (dict(Fresnel='Loss', Coating=[1.38, 100.0, 2.0]), 'G_: Coating: 3 numbers'),
])
def test_refused_by_the_bake(props, message):
  doc, src = _one_lens(**props)
  with pytest.raises(ValueError, match=message):
    bake.bakeScene(doc, src)


def test_group_coating_values():
  sc = cc.slab('Loss', cc.Q, second='Split', second_coating=cc.W)[0]
  assert sc.group_coating.dtype == bake.COATING_DTYPE and sc.group_coating['n'].tolist() == [0, 1, 0, 3]
  assert sc.group_coating['layers'][1, 0].tolist() == [1.38, 550 / 4 / 1.38] and not sc.group_coating['layers'][1, 1:].any()
  assert sc.group_coating['layers'][3, :3].tolist() == [list(l) for l in cc.W]
  cnt, lay = _native.coating_tables(sc.group_coating)
  assert cnt.tolist() == [0, 1, 0, 3] and lay.shape == (4, 4, 2) and lay.dtype == np.float64 and cnt.dtype == np.int32
  # a document without the property: all zeros
  plain = fc.slab('Loss')[0]
  assert not plain.group_coating['n'].any() and not plain.group_coating['layers'].any()
  # the helpers
  assert make.MGF2 == 1.38 and make.quarterWave(make.MGF2, 550) == (1.38, 550 / (4 * 1.38))
  assert _native.COAT_LAYERS == bake.COAT_LAYERS == 4
  # a flat list (what an FCStd file stores) is the same stack
  doc, src = _one_lens(Fresnel='Loss', Coating=[1.38, 99.6, 2.1, 130.9])
  assert bake.bakeScene(doc, src).group_coating['layers'][0, :2].tolist() == [list(l) for l in cc.V]


# ---- FCStd ---------------------------------------------------------------------------------------------------------------
def test_a_document_carrying_the_property(tmp_path):
  src_path = os.path.join(SCENES, 'GettingStarted.FCStd')
  plain = open_fcstd(src_path)
  lens = next(o for o in bake.opticalObjects(plain) if o._props.get('OpticalType') == 'Lens')
  source = bake.lightSources(plain)[0]
  path = str(tmp_path / 'coated.FCStd')
  flat = [v for layer in cc.W for v in layer]
  _with_properties(src_path, path, {lens.Name: [('Fresnel', 'String', 'Loss'), ('Coating', 'FloatList', flat)]})
  doc = open_fcstd(path)
  assert doc.getObject(lens.Name)._props['Coating'] == flat
  sc, sc0 = bake.bakeScene(doc, doc.getObject(source.Name)), bake.bakeScene(plain, source)
  gi = sc.group_names.index(lens.Name)
  assert sc.group_coating['n'][gi] == 3 and sc.group_coating['n'].sum() == 3
  assert sc.group_coating['layers'][gi, :3].tolist() == [list(l) for l in cc.W]
  assert not sc0.group_coating['n'].any() and not sc0.group_coating['layers'].any()
  for name in ('prim_type', 'prim_xform', 'prim_params', 'group_type', 'group_ior', 'group_abslen'):
    assert np.asarray(getattr(sc, name)).tobytes() == np.asarray(getattr(sc0, name)).tobytes(), name


def test_the_property_is_optional_in_the_repair():
  group = fcstd._PROXY_PROPERTIES[('freecad.optics_design_workbench.freecad_elements.optical_group', 'OpticalGroupProxy')]
  assert 'Coating' in group and 'Coating' in fcstd._OPTIONAL_PROPERTIES
  for drop, extra, repaired in ((2, False, True), (3, False, False), (3, True, False)):
    doc = Document()
    g = make.makeLens(doc, [make.makeBox(doc, 'B', 1, 1, 1)], name='OpticalLensGroup')
    g._props['Proxy'] = None
    for k in fcstd._OPTIONAL_PROPERTIES:
      g._props.pop(k, None)
    if extra:
      g._props['Coating'] = [1.38, 99.6]
    for k in [n for n in group if n not in fcstd._OPTIONAL_PROPERTIES][1:1 + drop]:
      g._props.pop(k, None)
    fcstd.repairProxies(doc)
    assert bool(g.ProxyClass) == repaired, (drop, extra)


# ---- the compiled kernel's header ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['Loss', 'Split'])
def test_compile_check(native_lib, mode):
  """header + hiprtc compile for gfx950 of the COAT variant with Q on one slab and W on the other: the layer counts are
  constants of the header (part of the cache key), the thicknesses are values"""
  sc, lim, src = cc.slab(mode, cc.Q, second=mode, second_coating=cc.W)
  bare, bare_bytes = _native.compile_check_fresnel(sc, lim, source=src)
  none, _ = _native.compile_check_coating(sc, lim, source=src, coating=[[]] * 4)
  assert none == bare                                            # no coating: the FRESNEL header as a string
  header, code_bytes = _native.compile_check_coating(sc, lim, source=src)
  assert '  static constexpr int coat(int i) { constexpr int T[] = {0, 1, 0, 3}; return T[i]; }\n' in header
  assert '  static constexpr int cc(int i)' in header and '#define ODW_SPEC_COAT true\n' in header
  assert '#define ODW_SPEC_FRESNEL true\n' in header and 'coat(' not in bare and 'ODW_SPEC_COAT' not in bare
  assert code_bytes > 10000
  print(f'{mode}: FRESNEL {bare_bytes} bytes, COAT {code_bytes} bytes')
  # other thicknesses and indices: the same header (the same kernel)
  thicker = [[], [(1.45, 120.0)], [], [(1.4, 10.0), (2.2, 20.0), (1.7, 30.0)]]
  assert _native.compile_check_coating(sc, lim, source=src, coating=thicker)[0] == header
  # another layer count: another header
  fewer = [[], cc.Q, [], cc.V]
  assert _native.compile_check_coating(sc, lim, source=src, coating=fewer)[0] != header
