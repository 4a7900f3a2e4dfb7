"""Point-source ray generation on the device -- ray_uniforms, sample_tables / inv_cdf, make_ray (odw_kernels.hip) -- held to
exact arithmetic on the cases of source_cases.py: the uniforms to an independent Philox, the inversion to the exact
piecewise-linear inverse (truth) and to numpy.interp bit for bit (contract), the search guides to plain binary searches,
the theta row to a full argmin, origins and directions to 200-bit / longdouble rays, every launch route to
generateRays(), and the tables the kernels cannot serve to a refusal by name.  At most 2^18 rays per launch."""
import copy
import dataclasses

import numpy as np
import pytest

import source_cases as sc
from conftest import project
from source_cases import EPS, L
from test_gpu_spec_source import PHI_DEPENDENT, baked, set_source_unguided, tracers, two_lens_doc  # noqa: F401 (tracers: a fixture)

pytestmark = pytest.mark.gpu

TABLE_CASES = sorted(sc.MAKERS)


@pytest.fixture(scope='module')
def tr(native_lib):
  from freecad.optics_design_workbench_amd.simulation.tracer import Tracer
  t = Tracer(0)
  yield t
  t.close()


_SAMPLED = {}


def get_case(name):
  if name == 'geometric-one-row':
    return sc.geometric_case(False)
  return sc.rows_case(name) if name in sc.ROW_CASES else sc.table_case(name)


def sampled(tr, name, guides=True):
  """(t, phi) of the case's rays from the device, one launch per (case, upload)"""
  if (name, guides) not in _SAMPLED:
    case = get_case(name)
    if guides:
      tr.setSource(sc.source_of(case))
    else:
      set_source_unguided(tr, sc.source_of(case))
    _SAMPLED[name, guides] = tr.sample(case.first, case.n, case.seed)
  return _SAMPLED[name, guides]


ALL_TABLES = TABLE_CASES + list(sc.ROW_CASES) + ['geometric-one-row']


# 1 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('first', sc.FIRSTS)
@pytest.mark.parametrize('seed', sc.SEEDS)
def test_uniforms(tr, first, seed):
  """identity tables: sample() returns (u_t, u_phi), the numpy Philox says what they are -- from ray 0, across ray 2^32
  (the counter's high word), at 2^40, with the key's high word set"""
  n = 4096 + 37
  tr.setSource(sc.source_of(sc.table_case('identity')))
  t, phi = tr.sample(first, n, seed)
  u_phi, u_t = sc.uniforms(first, n, seed)
  assert np.array_equal(t, u_t) and np.array_equal(phi, u_phi)


# 2 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ALL_TABLES)
def test_inversion_truth(tr, name):
  """|value - exact| <= 8 * 2^-53 * max(|e_j|, |e_j+1|) on both axes; a ray on a knot gets the knot's edge itself"""
  case = get_case(name)
  t, phi = sampled(tr, name)
  rows = sc.exact_row(case.phi_edges, phi) if len(case.t_cdf) > 1 else np.zeros(case.n, dtype=int)
  sc.check_inversion(case, t, phi, rows=rows)


# 3 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ALL_TABLES)
def test_inversion_contract(tr, name):
  """the documented contract of inv_cdf: numpy.interp(u, cdf, edges), bit for bit"""
  case = get_case(name)
  t, phi = sampled(tr, name)
  t0, phi0 = sc.host_draw(case)
  assert np.array_equal(phi, phi0)
  assert np.array_equal(t, t0)


# 4 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ALL_TABLES)
def test_guides(tr, name):
  """the guides change how a knot is found, never which: odw_upload_source_unguided gives the same values"""
  t, phi = sampled(tr, name)
  t1, phi1 = sampled(tr, name, guides=False)
  assert np.array_equal(phi1, phi) and np.array_equal(t1, t)


# 5 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('guides', [True, False], ids=['guides', 'no-guides'])
@pytest.mark.parametrize('name', sc.ROW_CASES)
def test_rows(tr, name, guides):
  """the theta row of every ray is the full argmin's, the rays whose phi is exactly an edge included"""
  case = get_case(name)
  t, phi = sampled(tr, name, guides)
  want = sc.exact_row(case.phi_edges, phi)
  got = sc.row_of_value(case, t)
  assert np.isin(phi, case.phi_edges[1:-1]).sum() >= len(case.phi_edges) - 2
  if name.endswith('narrow'):
    assert (phi == case.phi_edges[0]).any() and (phi == case.phi_edges[-1]).any()
  assert np.array_equal(got, want), (int((got != want).sum()), 'rays in another row')


# 6 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fr,focal', sc.RAY_SOURCES, ids=[f'{a}-f{b:g}' for a, b in sc.RAY_SOURCES])
def test_rays(tr, fr, focal):
  """generateRays() against exact_ray: |dir - exact|_inf <= C 2^-53 (1 + |origin|_inf), |origin - exact|_inf <=
  C 2^-53 (|origin|_inf + |f|), |dir| = 1 within 4 * 2^-53; C = 4 C_HOST (source_cases.py)"""
  case = sc.ray_case(bool(np.isfinite(focal)))
  tr.setSource(sc.source_of(case, sc.FRAMES[fr], focal))
  t, phi = sc.host_draw(case)
  st, sphi = tr.sample(case.first, case.n, case.seed)
  assert np.array_equal(st, t) and np.array_equal(sphi, phi)        # (the chosen angles reach make_ray bit for bit)
  o, d = tr.generateRays(case.first, case.n, case.seed)
  eo, ed = sc.exact_ray(sc.FRAMES[fr], focal, t, phi)
  for i in range(len(case.pairs)):                                  # (200 bits on the rays of the chosen angles)
    mo, md = sc.exact_ray_mp(sc.FRAMES[fr], focal, t[i], phi[i])
    eo[i], ed[i] = [sc._mp_to_long(v) for v in mo], [sc._mp_to_long(v) for v in md]
  rd, ro = sc.ray_ratios(focal, t, o, d, eo, ed)
  norm = np.abs(np.sqrt((d.astype(L) ** 2).sum(axis=1)) - 1).astype(np.float64).max() / EPS
  print(f'device {fr} f={focal:g}: direction {rd.max():.3f}, origin {ro.max():.3f} (x 2^-53 x scale; C = {sc.C:g}), |dir| - 1: {norm:.3f} x 2^-53')
  assert rd.max() <= sc.C, (int(rd.argmax()), t[rd.argmax()], phi[rd.argmax()])
  assert ro.max() <= sc.C, (int(ro.argmax()), t[ro.argmax()], phi[ro.argmax()])
  assert norm <= 4


# 7 ------------------------------------------------------------------------------------------------------------
def shell_doc(radius):
  """one recording absorbing sphere around the source: a ray's only row carries its direction as generated"""
  from freecad.optics_design_workbench_amd.freecad_elements import make
  from freecad.optics_design_workbench_amd.scene import Document
  doc = Document()
  make.makeAbsorber(doc, [make.makeSphere(doc, 'Shell', radius)], RecordHits=True)
  make.makeSimulationSettings(doc)
  return doc


@pytest.mark.parametrize('fr', ['identity', 'quarter-z', 'general'])
def test_routes(tracers, fr):
  """the generic flat kernel, the kernel compiled against the source and a batch launch (odw_batch_rays_kernel) start
  their rays in the directions of generateRays(), bit for bit (-0.0 == 0.0: xf_comb)"""
  case = sc.table_case('dense')
  src = sc.source_of(case, sc.FRAMES[fr], 2.5)
  pr = baked(shell_doc(120.0), source=src)
  other = baked(shell_doc(125.0), source=src)
  n, cap = case.n, case.n + 1024
  ref = tracers('off')
  ref.setSource(src)
  _, want = ref.generateRays(case.first, n, case.seed)
  assert np.all(np.isfinite(want)) and len(np.unique(want[:, 0])) > n // 2

  def launch(t):
    t.setScene(pr.scene)
    t.setSource(src)
    t.setLimits(pr.limits)
    t.setDetector(None)
    t.reserveHits(cap)
    t.reset()
    t.trace(case.first, n, case.seed)
    t.sync()
    return t.hits(), t.compiledInfo()
  rows, info = launch(ref)
  assert info['mode'] == 0 and len(rows) == n
  assert np.array_equal(rows['direction'], want)
  rows, info = launch(tracers('structure'))
  assert info['mode'] == 1 and info['source'] != 0 and len(rows) == n
  assert np.array_equal(rows['direction'], want)
  bt = tracers('off')
  bt.setLimits(pr.limits)
  bt.setSource(src)
  bt.setSceneBatch([pr.scene, other.scene])
  bt.reset()
  bt.traceBatch(case.first, n, case.seed, cap)
  bt.sync()
  for k in (0, 1):
    bt.batchSelect(k)
    rows = bt.hits()
    assert len(rows) == n and np.array_equal(rows['direction'], want)
  bt.batchSelect(None)


# 8 ------------------------------------------------------------------------------------------------------------
def test_refusals(tr):
  """tables sample_tables cannot serve are refused by name; what the product makes is accepted"""
  from freecad.optics_design_workbench_amd import _native
  geo = sc.source_of(sc.geometric_case(True))
  with pytest.raises(_native.NativeError, match='invalid.*odw_upload_source: phi_edges.*equidistant'):
    tr.setSource(geo)
  with pytest.raises(_native.NativeError, match='phi_edges.*equidistant'):
    set_source_unguided(tr, geo)
  tr.setSource(sc.source_of(sc.geometric_case(False)))             # one theta table: no row is looked for (test 2 holds on it)
  rows = sc.source_of(sc.rows_case('rows-24'))
  tr.setSource(rows)
  bad = copy.copy(rows)
  bad.tables = copy.copy(rows.tables)
  bad.tables.phi_cdf = rows.tables.phi_cdf.copy()
  bad.tables.phi_cdf[7] = bad.tables.phi_cdf[5]                      # (decreases from knot 6 to knot 7)
  assert bad.tables.phi_cdf[7] < bad.tables.phi_cdf[6]
  with pytest.raises(_native.NativeError, match='invalid.*odw_upload_source: phi_cdf decreases'):
    tr.setSource(bad)
  for nudge, what in ((8.0, 'equidistant'), (np.nan, 'equidistant')):     # one edge 8 ulp of the larger end off; not a number
    bad = copy.copy(rows)
    bad.tables = copy.copy(rows.tables)
    bad.tables.phi_edges = rows.tables.phi_edges.copy()
    bad.tables.phi_edges[3] += nudge * np.spacing(rows.tables.phi_edges[-1])
    with pytest.raises(_native.NativeError, match=what):
      tr.setSource(bad)
  ok = copy.copy(rows)                                                # 3 ulp off: still the edges of a linspace
  ok.tables = copy.copy(rows.tables)
  ok.tables.phi_edges = rows.tables.phi_edges.copy()
  ok.tables.phi_edges[3] += 3.0 * np.spacing(rows.tables.phi_edges[-1])
  tr.setSource(ok)
  # the benchmark sources, a source with a theta table per azimuth cell as VectorRandomVariable.tables() makes it
  for scene in ('lensesAndMirrors', 'hugeArray', 'GettingStarted'):
    tr.setSource(project(scene).source)
  per_cell = baked(two_lens_doc(), **PHI_DEPENDENT).source
  assert per_cell.tables.t_cdf.shape[0] == len(per_cell.tables.phi_edges) - 1 > 1
  tr.setSource(per_cell)
  # ... and decreasing edges, which numpy.linspace makes as well
  back = copy.copy(rows)
  back.tables = copy.copy(rows.tables)
  back.tables.phi_edges = np.linspace(2 * np.pi, 0.0, len(rows.tables.phi_edges))
  tr.setSource(back)


def test_surface_sampler_refusals(tr):
  """the stochastic-surface tables feed the same sample_tables: the same rules at odw_upload_surface_samplers"""
  from freecad.optics_design_workbench_amd import _native
  pr = project('mirror-diffuse')
  tr.setScene(pr.scene)                                               # what the bake makes is accepted
  s0 = pr.scene.surface_samplers[0]
  nf, cells = s0.n_family, 11
  geo = np.concatenate([[0.0], np.geomspace(0.01, 2 * np.pi, cells)])
  phi_cdf = np.tile(np.linspace(0.0, 1.0, cells + 1), (nf, 1))
  t_edges = np.array([0.0, 0.1, 0.2])

  def scene_with(phi_edges, phi_cdf, rows):
    t_cdf = np.tile(np.array([0.0, 0.5, 1.0]), (nf, rows, 1))
    s = dataclasses.replace(s0, phi_edges=phi_edges, phi_cdf=phi_cdf, t_edges=t_edges, t_cdf=t_cdf,
                            atom_mass=None, atom_theta=None, atom_phi=None)
    scene = copy.copy(pr.scene)
    scene.surface_samplers = [s]
    return scene
  with pytest.raises(_native.NativeError, match='invalid.*surface sampler: phi_edges.*equidistant'):
    tr.setScene(scene_with(geo, phi_cdf, cells))
  tr.setScene(scene_with(geo, phi_cdf, 1))
  tr.setScene(scene_with(np.linspace(0.0, 2 * np.pi, cells + 1), phi_cdf, cells))
  falling = phi_cdf.copy()
  falling[-1, 4] = falling[-1, 2]
  with pytest.raises(_native.NativeError, match='invalid.*surface sampler: phi_cdf decreases'):
    tr.setScene(scene_with(np.linspace(0.0, 2 * np.pi, cells + 1), falling, cells))
  tr.setScene(pr.scene)
