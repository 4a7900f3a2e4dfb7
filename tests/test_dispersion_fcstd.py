"""Glasses and spectra in documents read from FCStd files (scene/fcstd.py): the new properties are read (strings, float
lists as members of the zip), they bake like those of a document built with `make`, and they are optional in the proxy
repair: which documents get their proxy back is what it was."""
import os
import shutil
import struct
import xml.etree.ElementTree as ET
import zipfile

import numpy as np

import spectral_cases as sp
from conftest import SCENES
from freecad.optics_design_workbench_amd.freecad_elements import make, point_source
from freecad.optics_design_workbench_amd.scene import Document, bake, fcstd, open_fcstd


def _float_list(values):
  return struct.pack('<I', len(values)) + np.asarray(values, dtype='<f8').tobytes()


def _with_properties(src_path, dst_path, per_object):
  """a copy of the FCStd file with properties added: {object name: [(name, 'String' | 'FloatList', value)]}"""
  with zipfile.ZipFile(src_path) as zin, zipfile.ZipFile(dst_path, 'w', zipfile.ZIP_DEFLATED) as zout:
    root = ET.fromstring(zin.read('Document.xml'))
    members = {}
    for o in root.find('ObjectData').findall('Object'):
      for name, kind, value in per_object.get(o.attrib['name'], []):
        p = ET.SubElement(o.find('Properties'), 'Property', name=name, type='App::Property' + kind)
        if kind == 'String':
          ET.SubElement(p, 'String', value=value)
        else:
          member = f'{o.attrib["name"]}.{name}'
          ET.SubElement(p, 'FloatList', file=member)
          members[member] = _float_list(value)
    for item in zin.infolist():
      if item.filename != 'Document.xml':
        zout.writestr(item, zin.read(item.filename))
    zout.writestr('Document.xml', ET.tostring(root, encoding='utf-8', xml_declaration=True))
    for member, data in members.items():
      zout.writestr(member, data)


def test_a_document_carrying_the_properties(tmp_path):
  src_path = os.path.join(SCENES, 'GettingStarted.FCStd')
  plain = open_fcstd(src_path)
  lens = next(o for o in bake.opticalObjects(plain) if o._props.get('OpticalType') == 'Lens')
  source = bake.lightSources(plain)[0]
  path = str(tmp_path / 'glass.FCStd')
  lines = [486.1327, 1.0, 587.5618, 2.0, 656.2725, 1.0]
  _with_properties(src_path, path, {
      lens.Name: [('Dispersion', 'String', 'Sellmeier'), ('DispersionCoefficients', 'FloatList', sp.BK7)],
      source.Name: [('Spectrum', 'FloatList', lines), ('SpectralDensity', 'String', '')]})
  doc = open_fcstd(path)
  g, s = doc.getObject(lens.Name), doc.getObject(source.Name)
  assert g._props['Dispersion'] == 'Sellmeier' and g._props['DispersionCoefficients'] == sp.BK7
  assert s._props['Spectrum'] == lines
  sc, sc0 = bake.bakeScene(doc, s), bake.bakeScene(plain, source)
  gi = sc.group_names.index(lens.Name)
  assert sc.group_disp_kind[gi] == 1 and sc.group_disp[gi].tolist() == sp.BK7
  assert sc.group_disp_kind.sum() == 1 and not sc0.group_disp_kind.any()
  for name in ('prim_type', 'prim_xform', 'prim_params', 'group_type', 'group_ior', 'group_abslen'):
    assert np.asarray(getattr(sc, name)).tobytes() == np.asarray(getattr(sc0, name)).tobytes(), name
  spec = point_source.bakeSpectrum(s)
  assert spec.mode == 'lines' and spec.wavelengths.tolist() == list(sp.LINES) and spec.cdf.tolist() == [0.25, 0.75, 1.0]
  assert point_source.bakeSpectrum(source) is None


def test_the_property_lists_name_them_and_the_repair_ignores_them():
  group = fcstd._PROXY_PROPERTIES[('freecad.optics_design_workbench.freecad_elements.optical_group', 'OpticalGroupProxy')]
  src = fcstd._PROXY_PROPERTIES[('freecad.optics_design_workbench.freecad_elements.point_source', 'PointSourceProxy')]
  assert {'Dispersion', 'DispersionCoefficients'} <= set(group)
  assert {'Spectrum', 'SpectralDensity', 'SpectrumDomain', 'SpectrumResolution'} <= set(src)
  new = fcstd._OPTIONAL_PROPERTIES
  # a group as the reference's workbench wrote it -- none of the new properties, two of its own missing, no proxy --
  # gets its proxy back as before; with a third one missing it does not, as before; and the new properties alone do not
  # make up for missing ones
  for drop, extra, repaired in ((2, False, True), (3, False, False), (3, True, False), (0, True, True)):
    doc = Document()
    g = make.makeLens(doc, [make.makeBox(doc, 'B', 1, 1, 1)], name='OpticalLensGroup', **(dict(make.N_BK7) if extra else {}))
    g._props['Proxy'] = None
    if not extra:
      for k in new:
        g._props.pop(k, None)
    for k in [n for n in group if n not in new][1:1 + drop]:
      g._props.pop(k, None)
    fcstd.repairProxies(doc)
    assert bool(g.ProxyClass) == repaired, (drop, extra)
