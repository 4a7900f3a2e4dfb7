"""Fresnel reflection at lens surfaces, the parts that need no GPU: the reflectance on the host (`odw_fresnel_reflectance`
without a context) against closed forms and against numpy, the bake's `group_fresnel` and its refusals, the property in a
document read from an FCStd file, and the header of the compiled kernel's FRESNEL variant (hiprtc for gfx950)."""
import os

import numpy as np
import pytest

import fresnel_cases as fc
from conftest import SCENES
from freecad.optics_design_workbench_amd import _native, scenes
from freecad.optics_design_workbench_amd.freecad_elements import make
from freecad.optics_design_workbench_amd.scene import Document, bake, fcstd, open_fcstd
from test_dispersion_fcstd import _with_properties

TOL = 1e-12


# ---- closed forms ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n1, n2', [(1.0, 1.5), (1.5, 1.0), (1.3, 1.9), (1.0, 1.0)])
def test_normal_incidence(native_lib, n1, n2):
  R = _native.fresnel_reflectance(n1, n2, [1.0])[0]
  assert abs(R - ((n1 - n2) / (n1 + n2)) ** 2) < TOL


@pytest.mark.parametrize('n1, n2', [(1.0, 1.5), (1.5, 1.0), (1.0, 1.9)])
def test_brewster(native_lib, n1, n2):
  """at tan(i) = n2 / n1 the p component vanishes: R = rs^2 / 2, rs = (n1 cos_i - n2 cos_t) / (n1 cos_i + n2 cos_t) with
  cos_t = sin_i there"""
  i = np.arctan2(n2, n1)
  cos_i, cos_t = np.cos(i), np.sin(i)
  rs = (n1 * cos_i - n2 * cos_t) / (n1 * cos_i + n2 * cos_t)
  R = _native.fresnel_reflectance(n1, n2, [cos_i])[0]
  assert abs(R - 0.5 * rs * rs) < TOL


def test_reciprocity(native_lib):
  """R(n1 -> n2, i) = R(n2 -> n1, t)"""
  for n in (1.3, 1.5, 1.9):
    i = np.radians(np.linspace(0.0, 89.0, 90))
    cos_t = np.sqrt(1.0 - (np.sin(i) / n) ** 2)
    a = _native.fresnel_reflectance(1.0, n, np.cos(i))
    b = _native.fresnel_reflectance(n, 1.0, cos_t)
    assert np.abs(a - b).max() < TOL, n


def test_grazing_and_total_reflection(native_lib):
  R = _native.fresnel_reflectance(1.0, 1.5, [1e-3, 1e-6, 1e-9, 0.0])
  assert np.all(np.diff(R) > 0) and abs(R[-1] - 1.0) < TOL and 1.0 - R[2] < 1e-8
  # beyond the critical angle of glass -> air (41.81 degrees): exactly 1
  i = np.radians(np.linspace(42.0, 90.0, 50))
  assert np.all(_native.fresnel_reflectance(1.5, 1.0, np.cos(i)) == 1.0)
  assert _native.fresnel_reflectance(1.5, 1.0, [np.cos(np.radians(41.0))])[0] < 1.0


def test_bad_arguments(native_lib):
  with pytest.raises(_native.NativeError, match='odw_fresnel_reflectance'):
    _native.fresnel_reflectance(0.0, 1.5, [1.0])


# ---- a grid against numpy ----------------------------------------------------------------------------------------------
def test_grid_against_numpy(native_lib):
  """1000 incidences 0 .. 89.9 degrees per index and direction against the angle form of the formula (sines and tangents of
  i -+ t: no expression shared with the library's amplitude form).  Inputs with |root| < 1e-3 are left out -- near the
  critical angle cos_t = sqrt(root) amplifies rounding without bound -- and they are at most 1 % of the grid."""
  i = np.radians(np.linspace(0.0, 89.9, 1000))
  cos_i = np.cos(i)
  total = kept = 0
  for n in (1.3, 1.5, 1.9):
    for n1, n2 in ((1.0, n), (n, 1.0)):
      keep = np.abs(fc.root_of(n1, n2, cos_i)) >= 1e-3
      total += len(cos_i)
      kept += int(keep.sum())
      got = _native.fresnel_reflectance(n1, n2, cos_i[keep])
      want = fc.reflectance(n1, n2, cos_i[keep])
      err = np.abs(got - want).max()
      print(f'{n1} -> {n2}: kept {int(keep.sum())} of {len(cos_i)}, largest difference {err:.3g}')
      assert err < TOL, (n1, n2)
      assert np.all((got >= 0) & (got <= 1))
  assert total - kept <= 0.01 * total, (total, kept)


# ---- bake --------------------------------------------------------------------------------------------------------------
def test_group_fresnel_values(native_lib):
  assert fc.slab('')[0].group_fresnel.tolist() == [0, 0, 0]
  assert fc.slab('Loss')[0].group_fresnel.tolist() == [0, 1, 0]
  sc = fc.slab('Split', second='Loss')[0]
  assert sc.group_fresnel.tolist() == [0, 2, 0, 1] and sc.group_fresnel.dtype == np.int32
  assert fc.singlet('Loss')[0].group_fresnel.tolist() == [1, 0, 0, 0]
  assert _native.FRESNEL_MODES['Loss'] == bake.FRESNEL_MODES['Loss'] == 1 and _native.FRESNEL_MODES['Split'] == bake.FRESNEL_MODES['Split'] == 2
  assert _native.STREAM_FRESNEL == 7


def _one_group(kind, **props):
  doc = Document()
  make.makeOpticalGroup(doc, kind, [make.makeBox(doc, 'B', 1, 1, 1)], name='G_', **props)
  make.makeSimulationSettings(doc)
  return doc, make.makePointSource(doc)


@pytest.mark.parametrize('kind, props', [('Mirror', {}), ('Absorber', {}), ('Vacuum', {}), ('Grating', dict(GratingType='Reflection')),
                                         ('Grating', dict(GratingType='Transmission'))])
def test_refused_on_a_group_that_is_not_a_lens(kind, props):
  doc, src = _one_group(kind, Fresnel='Loss', **props)
  with pytest.raises(ValueError, match='G_: Fresnel on a group that is not a lens'):
    bake.bakeScene(doc, src)
  doc, src = _one_group(kind, **props)                    # (without the property: baked as before)
  assert not bake.bakeScene(doc, src).group_fresnel.any()


def test_refused_unknown_mode():
  doc, src = _one_group('Lens', Fresnel='Coated')
  with pytest.raises(ValueError, match="G_: Fresnel 'Coated'"):
    bake.bakeScene(doc, src)


def test_validation_of_the_library(native_lib):
  lens, mirror = 1, 0                    # ODW_OPT_*
  _native.fresnel_check([0, 1, 2], [mirror, lens, lens])
  with pytest.raises(_native.NativeError, match='group 1: unknown Fresnel mode 3'):
    _native.fresnel_check([0, 3, 0])
  with pytest.raises(_native.NativeError, match='group 0: a Fresnel mode on a group that is not a lens'):
    _native.fresnel_check([2, 0], [mirror, lens])
  sc, lim, _ = fc.slab('Loss')
  with pytest.raises(_native.NativeError, match='group 0: a Fresnel mode on a group that is not a lens'):
    _native.compile_check_fresnel(sc, lim, modes=[1, 1, 0])
  with pytest.raises(ValueError, match='2 modes for a scene of 3 groups'):          # (one mode per group, checked before the call)
    _native.compile_check_fresnel(sc, lim, modes=[0, 1])


def test_fan_mode_refuses_split():
  from freecad.optics_design_workbench_amd.simulation import simulation_loop

  class NoTracer:                                         # (the refusal comes before the first launch)
    device = 0

    def __getattr__(self, name):
      return lambda *a, **k: None

  doc = fc.slab_document('Split')
  make.makeSimulationSettings(doc)
  make.makePointSource(doc)
  with pytest.raises(ValueError, match="Fresnel 'Split' is for the Monte-Carlo modes"):
    simulation_loop.runSimulation(doc, 'singlefans', tracer=NoTracer(), keepOnDevice=False)


# ---- FCStd ---------------------------------------------------------------------------------------------------------------
def test_a_document_carrying_the_property(tmp_path):
  src_path = os.path.join(SCENES, 'GettingStarted.FCStd')
  plain = open_fcstd(src_path)
  lens = next(o for o in bake.opticalObjects(plain) if o._props.get('OpticalType') == 'Lens')
  source = bake.lightSources(plain)[0]
  path = str(tmp_path / 'fresnel.FCStd')
  _with_properties(src_path, path, {lens.Name: [('Fresnel', 'String', 'Split')]})
  doc = open_fcstd(path)
  assert doc.getObject(lens.Name)._props['Fresnel'] == 'Split'
  sc, sc0 = bake.bakeScene(doc, doc.getObject(source.Name)), bake.bakeScene(plain, source)
  gi = sc.group_names.index(lens.Name)
  assert sc.group_fresnel[gi] == 2 and sc.group_fresnel.sum() == 2 and not sc0.group_fresnel.any()
  for name in ('prim_type', 'prim_xform', 'prim_params', 'group_type', 'group_ior', 'group_abslen'):
    assert np.asarray(getattr(sc, name)).tobytes() == np.asarray(getattr(sc0, name)).tobytes(), name


def test_the_property_is_optional_in_the_repair():
  group = fcstd._PROXY_PROPERTIES[('freecad.optics_design_workbench.freecad_elements.optical_group', 'OpticalGroupProxy')]
  assert 'Fresnel' in group and 'Fresnel' in fcstd._OPTIONAL_PROPERTIES
  # a group as the reference's workbench wrote it (none of this project's properties, two of its own missing, no proxy) is
  # repaired as before; with a third missing it is not, and a Fresnel property does not make up for it
  for drop, extra, repaired in ((2, False, True), (3, False, False), (3, True, False)):
    doc = Document()
    g = make.makeLens(doc, [make.makeBox(doc, 'B', 1, 1, 1)], name='OpticalLensGroup')
    g._props['Proxy'] = None
    for k in fcstd._OPTIONAL_PROPERTIES:
      g._props.pop(k, None)
    if extra:
      g._props['Fresnel'] = 'Loss'
    for k in [n for n in group if n not in fcstd._OPTIONAL_PROPERTIES][1:1 + drop]:
      g._props.pop(k, None)
    fcstd.repairProxies(doc)
    assert bool(g.ProxyClass) == repaired, (drop, extra)


# ---- the compiled kernel's header ----------------------------------------------------------------------------------------
def _golden_with_a_lens():
  proj = scenes.bakeProject(os.path.join(SCENES, 'lensesAndMirrors.FCStd'))
  lens = [g for g in range(proj.scene.n_groups) if proj.scene.group_type[g] == 1]
  assert lens
  return proj, lens


@pytest.mark.parametrize('case', ['slab', 'singlet', 'golden'])
def test_compile_check(native_lib, case):
  """header + hiprtc compile for gfx950 of the FRESNEL variant: the modes are constants of the header (part of the cache
  key), the rest of the header is the plain one, and a header without modes is the plain header as a string"""
  if case == 'slab':
    sc, lim, src = fc.slab('Split', second='Loss')
  elif case == 'singlet':
    sc, lim, src = fc.singlet('Loss')
  else:
    proj, lens = _golden_with_a_lens()
    sc, lim, src = proj.scene, proj.limits, proj.source
    sc.group_fresnel = np.zeros(sc.n_groups, np.int32)
    sc.group_fresnel[lens[0]] = 2
  plain, plain_bytes = _native.compile_check(sc, lim, 'structure', source=src)
  none, _ = _native.compile_check_fresnel(sc, lim, source=src, modes=np.zeros(sc.n_groups, np.int32))
  assert none == plain
  header, code_bytes = _native.compile_check_fresnel(sc, lim, source=src)
  table = '  static constexpr int fresnel(int i) { constexpr int T[] = {' + ', '.join(str(int(m)) for m in sc.group_fresnel) + '}; return T[i]; }\n'
  assert table in header and '#define ODW_SPEC_FRESNEL true\n' in header
  assert header.replace(table, '').replace('#define ODW_SPEC_FRESNEL true\n', '') == plain
  assert code_bytes > 10000
  print(f'{case}: plain {plain_bytes} bytes, FRESNEL {code_bytes} bytes')
  # other modes: another header (another kernel)
  other = np.where(np.asarray(sc.group_fresnel) == 2, 1, np.asarray(sc.group_fresnel) * 2).astype(np.int32)
  assert _native.compile_check_fresnel(sc, lim, source=src, modes=other)[0] != header
