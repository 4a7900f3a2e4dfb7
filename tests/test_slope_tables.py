"""The segment slopes the library stores behind the (cdf, edge) pairs of every inverse-CDF table it uploads
(csrc/odw_build.h: append_slopes, reached without a device through odw_table_slopes): numpy's own slope
(fp[j+1] - fp[j]) / (xp[j+1] - xp[j]) bit for bit, and the kernels' new form of the interpolation --
cdf[j] == u ? edge[j] : slope[j] * (u - cdf[j]) + edge[j], no division per sample -- equal to numpy.interp bit for
bit.  No GPU: the device evaluates the same three operations without contraction (test_sampler_bit_exact holds
that side)."""
import glob
import os

import numpy as np
import pytest

from conftest import GOLDEN

FILES = sorted(glob.glob(os.path.join(GOLDEN, 'sampler_*.npz')))


def numpy_slopes(cdf, edges):
  with np.errstate(divide='ignore', invalid='ignore'):
    s = (edges[1:] - edges[:-1]) / (cdf[..., 1:] - cdf[..., :-1])
  return np.concatenate([s, np.zeros(s.shape[:-1] + (1,))], axis=-1)     # the last knot has no segment


def bits(a):
  return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def tables():
  """(name, cdf rows, edges): the azimuth table and the theta rows of every golden sampler, and a table with a
  repeated cdf knot (a density that vanishes on a cell)"""
  out = []
  for f in FILES:
    d = np.load(f)
    name = os.path.basename(f)[len('sampler_'):-len('.npz')]
    out.append((name + '-phi', d['phi_cdf'][None, :], d['phi_edges']))
    out.append((name + '-theta', d['theta_cdf_knots'], d['theta_edges_knots']))
  out.append(('repeated-knot', np.array([[0.0, 0.25, 0.25, 0.25, 0.7, 1.0], [0.0, 0.0, 0.5, 0.5, 1.0, 1.0]]),
              np.array([-1.0, -0.5, 0.1, 0.3, 0.9, 2.0])))
  return out


TABLES = tables()


def test_golden_tables_are_there():
  assert len(FILES) >= 5


@pytest.mark.parametrize('name,cdf,edges', TABLES, ids=[t[0] for t in TABLES])
def test_host_slopes_are_numpys(native_lib, name, cdf, edges):
  from freecad.optics_design_workbench_amd import _native
  got = _native.table_slopes(cdf, edges)
  want = numpy_slopes(cdf, edges)
  assert got.shape == want.shape
  assert np.array_equal(bits(got), bits(want))
  if name == 'repeated-knot':
    assert np.isinf(got).sum() == 5 and not np.isnan(got).any()


def test_a_vanishing_segment_is_not_a_number(native_lib):
  """0 / 0 (a repeated knot in cdf AND edge) is NaN as in numpy; no sample lands on such a segment"""
  from freecad.optics_design_workbench_amd import _native
  got = _native.table_slopes([[0.0, 0.5, 0.5, 1.0]], [0.0, 1.0, 1.0, 2.0])
  assert np.isnan(got[0, 1]) and np.array_equal(bits(got[0, [0, 2, 3]]), bits([2.0, 2.0, 0.0]))


def test_bad_arguments_are_refused(native_lib):
  from freecad.optics_design_workbench_amd import _native
  with pytest.raises(_native.NativeError):
    _native.table_slopes([[0.0]], [1.0])


@pytest.mark.parametrize('name,cdf,edges', TABLES, ids=[t[0] for t in TABLES])
def test_slope_form_is_numpy_interp(native_lib, name, cdf, edges):
  """1e5 draws per table (spread over its rows): uniform ones, every knot value below 1, 0 and the largest double
  below 1"""
  from freecad.optics_design_workbench_amd import _native
  slopes = _native.table_slopes(cdf, edges)
  rng = np.random.default_rng(20240611)
  per_row = max(1, 100000 // len(cdf))
  for row, sl in zip(cdf, slopes):
    u = np.concatenate([rng.random(per_row), row[row < 1.0], [0.0, np.nextafter(1.0, 0.0)]])
    j = np.searchsorted(row, u, side='right') - 1            # the last knot with cdf <= u: what inv_cdf's search finds
    assert j.min() >= 0 and j.max() <= len(row) - 2
    with np.errstate(invalid='ignore'):
      got = np.where(row[j] == u, edges[j], sl[j] * (u - row[j]) + edges[j])
    want = np.interp(u, row, edges)
    assert np.isfinite(got).all()
    assert np.array_equal(bits(got), bits(want))
