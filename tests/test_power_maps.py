"""Power-weighted detector maps, the part that needs no GPU: `Hits.histogram(weights='powers')` names a column of the
hit dictionary (the reference's Histogram hands `weights=` to numpy.histogram2d, histogram.py:54,78), and the C-ABI
carries the power plane (version 12: odw_enable_power_histogram, odw_fetch_power_histogram,
odw_device_power_histogram, odw_hits_bin_power).  The rows come from the CPU oracle on a scene whose hits really
differ in power (tests/power_scene.py)."""
import numpy as np
import pytest

import power_scene


@pytest.fixture(scope='module')
def oracle_rows(oracle):
  sc, lim = power_scene.scene()
  o, d = power_scene.rays(6000)
  rows = oracle.trace_rays(sc, lim, o, d)['hits']
  assert len(rows) > 6000
  assert len(np.unique(rows['power'])) > 100          # reflectivity and absorption really exercised
  return rows


def _hits(rows):
  from freecad.optics_design_workbench_amd.jupyter_utils import Hits
  return Hits(dict(points=np.ascontiguousarray(rows['point']), directions=np.ascontiguousarray(rows['direction']),
                   powers=np.ascontiguousarray(rows['power']), isEntering=(rows['tag'] >> np.uint64(63)).astype(np.int64)))


@pytest.mark.parametrize('kw', [dict(bins=24), dict(bins=(4, 30), binCoords='polar'),
                                dict(bins=[np.linspace(-20, 20, 33), np.linspace(-20, 20, 17)])],
                         ids=['cart24', 'polar4x30', 'edges'])
def test_weights_names_a_column_of_the_hits(oracle_rows, kw):
  hits = _hits(oracle_rows)
  plane = dict(planeNormal=np.array([0.0, 0.0, 1.0]), xInPlaneVec=np.array([1.0, 0.0, 0.0]))
  by_name = hits.histogram(weights='powers', **plane, **kw)
  by_array = hits.histogram(weights=hits.hits['powers'], **plane, **kw)
  counts = hits.histogram(**plane, **kw)
  assert np.array_equal(by_name.hist, by_array.hist)
  assert np.array_equal(by_name.binX, by_array.binX) and np.array_equal(by_name.binY, by_array.binY)
  assert not np.array_equal(by_name.hist, counts.hist)
  assert by_name.hist.sum() < counts.hist.sum()          # every power is <= 1, most are below
  assert by_name.powerQuanta is None and counts.powerQuanta is None      # (only the device route carries the raw plane)


def test_abi_carries_the_power_plane(native_lib):
  import re
  from conftest import ROOT
  from freecad.optics_design_workbench_amd import _native
  assert native_lib.odw_abi_version() == _native.ABI_VERSION == 12
  header = open(ROOT + '/include/odw_trace.h').read()
  assert re.search(r'#define\s+ODW_POWER_QUANTUM_BITS\s+32\b', header) and re.search(r'#define\s+ODW_TRACE_POWER_HISTOGRAM\s+0x8\b', header)
  assert _native.TRACE_POWER_HISTOGRAM == 8 and _native.POWER_QUANTUM_BITS == 32
  for name in ('odw_enable_power_histogram', 'odw_fetch_power_histogram', 'odw_device_power_histogram', 'odw_hits_bin_power',
               'odw_compiled_power_info'):
    assert name in _native.SYMBOLS and hasattr(native_lib, name), name
