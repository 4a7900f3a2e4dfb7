"""The generation side on the CPU: the oracle (capi.sample, capi.make_rays), SamplerTables.draw and the host makeRay held
to the exact references of source_cases.py on every case the device is held to (test_gpu_source.py), the numpy Philox
held to the Random123 known answers, and C_HOST -- the error of the float64 host makeRay the device's bound rests on --
measured."""
import numpy as np
import pytest

import source_cases as sc
from source_cases import EPS, L

TABLE_CASES = sorted(sc.MAKERS)


def test_numpy_philox_known_answers():
  # Random123 kat_vectors, philox4x32 10 rounds
  def words(ctr, key):
    return [int(w[0]) for w in sc.philox4x32_10(ctr, key)]
  assert words([0, 0, 0, 0], [0, 0]) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
  assert words([0xffffffff] * 4, [0xffffffff] * 2) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
  assert words([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0]) == \
      [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


@pytest.mark.parametrize('first', sc.FIRSTS)
@pytest.mark.parametrize('seed', sc.SEEDS)
def test_identity_tables_show_the_uniforms(oracle, first, seed):
  """across ray 2^32 (the counter's high word) and with the key's high word set"""
  case = sc.table_case('identity')
  u_phi, u_t = sc.uniforms(first, 4096, seed)
  assert u_phi.min() >= 0.0 and u_phi.max() < 1.0 and len(np.unique(np.concatenate([u_phi, u_t]))) == 8192
  t, phi = oracle.sample(sc.source_of(case), first, 4096, seed)
  assert np.array_equal(t, u_t) and np.array_equal(phi, u_phi)


@pytest.mark.parametrize('name', TABLE_CASES)
def test_tables_oracle_and_host(oracle, name):
  case = sc.table_case(name)
  src = sc.source_of(case)
  t, phi = oracle.sample(src, case.first, case.n, case.seed)
  t0, phi0 = sc.host_draw(case)
  assert np.array_equal(t, t0) and np.array_equal(phi, phi0)              # the contract: numpy.interp, bit for bit
  t1, phi1 = src.tables.draw(case.u_phi, case.u_t)
  assert np.array_equal(t1, t0) and np.array_equal(phi1, phi0)
  sc.check_inversion(case, t, phi, rows=np.zeros(case.n, dtype=int))


def test_cases_put_rays_where_they_are_meant_to_be():
  """the makers do what they say: rays on knots, below and above them, on plateaus, in the crammed cells"""
  c = sc.table_case('on_rays')
  ex = sc.exact_inverse(c.t_cdf[0], c.t_edges, c.u_t)
  assert ex.on_knot.sum() >= 600 and ex.near.sum() >= 1800 and len(c.t_cdf[0]) >= 2050
  assert (np.diff(c.t_cdf[0]) == 0).sum() >= 30
  assert c.t_edges[-1] / c.t_edges[0] == pytest.approx(1e6)
  p = sc.table_case('plateaus')
  assert p.t_cdf[0][2] == 0.0 and p.t_cdf[0][-4] == 1.0 and (np.diff(p.t_cdf[0]) == 0).sum() >= 6
  assert len(sc.table_case('dense').t_cdf[0]) == 200001
  for name, lo, hi in (('crammed_low', 0.0, 2.0 ** -16), ('crammed_high', 1.0 - 2.0 ** -16, 1.0)):
    k = sc.table_case(name).t_cdf[0][1:-1]
    assert lo <= k.min() and k.max() <= hi and len(k) > 200
    k = sc.table_case(name).phi_cdf[1:-1]
    assert (lo > 0) * (1.0 - 2.0 ** -8) <= k.min() and k.max() <= (2.0 ** -8 if lo == 0 else 1.0)
  b = sc.table_case('at_guide_borders')
  for cdf, g in ((b.t_cdf[0], sc.T_GUIDE), (b.phi_cdf, sc.PHI_GUIDE)):
    for k in (1, g // 2, g - 1):
      assert {k / g, np.nextafter(k / g, 2.0), np.nextafter(k / g, -1.0)} <= set(cdf.tolist())
    assert cdf[1] == 5e-324


@pytest.mark.parametrize('name', sc.ROW_CASES)
def test_rows_oracle_and_host(oracle, name):
  case = sc.rows_case(name)
  src = sc.source_of(case)
  t, phi = oracle.sample(src, case.first, case.n, case.seed)
  want = sc.exact_row(case.phi_edges, phi)
  assert np.array_equal(sc.row_of_value(case, t), want)
  t1, phi1 = src.tables.draw(case.u_phi, case.u_t)
  assert np.array_equal(phi1, phi) and np.array_equal(sc.row_of_value(case, t1), want)
  # rays whose phi is an edge: interior ones (the tie between two rows) and, in the narrow table, both ends
  on_edge = np.isin(phi, case.phi_edges[1:-1])
  assert on_edge.sum() >= len(case.phi_edges) - 2
  if name.endswith('narrow'):
    assert (phi == case.phi_edges[0]).any() and (phi == case.phi_edges[-1]).any()
  assert len(np.unique(want)) == len(case.t_cdf)
  sc.check_inversion(case, t, phi, rows=want)


def test_geometric_azimuth_edges_oracle_and_host(oracle):
  """edges no window of three serves: the oracle and SamplerTables.draw pick the full argmin's row all the same"""
  case = sc.geometric_case(True)
  src = sc.source_of(case)
  t, phi = oracle.sample(src, case.first, case.n, case.seed)
  want = sc.exact_row(case.phi_edges, phi)
  assert np.array_equal(sc.row_of_value(case, t), want)
  t1, _ = src.tables.draw(case.u_phi, case.u_t)
  assert np.array_equal(sc.row_of_value(case, t1), want)
  # the cell floor((phi - e0) / (e1 - e0) * rows) and its neighbours miss the row for most rays
  e0, e1, rows = case.phi_edges[0], case.phi_edges[-1], len(case.t_cdf)
  guess = np.clip(np.floor((phi - e0) / (e1 - e0) * rows), 0, rows - 1)
  assert (np.abs(guess - want) > 1).mean() > 0.5


def host_rays(src, t, phi):
  from freecad.optics_design_workbench_amd.freecad_elements.point_source import makeRay
  rays = [makeRay(src, a, b) for a, b in zip(t, phi)]
  return np.array([r[0] for r in rays]), np.array([r[1] for r in rays])


@pytest.fixture(scope='module')
def measured():
  return dict(host=[0.0, 0.0], oracle=[0.0, 0.0])


@pytest.mark.parametrize('fr,focal', sc.RAY_SOURCES, ids=[f'{a}-f{b:g}' for a, b in sc.RAY_SOURCES])
def test_rays_oracle_and_host(oracle, measured, fr, focal):
  case = sc.ray_case(bool(np.isfinite(focal)))
  src = sc.source_of(case, sc.FRAMES[fr], focal)
  t, phi = sc.host_draw(case)
  # the chosen angles are on their rays bit for bit
  assert np.array_equal(t[:len(case.pairs)], [p[0] for p in case.pairs])
  assert np.array_equal(phi[:len(case.pairs)], [p[1] for p in case.pairs])
  assert np.abs(t).max() <= 1e3 and np.abs(phi).max() <= 64.0
  eo, ed = sc.exact_ray(src.xform, focal, t, phi)
  # (the longdouble reference against 200 bits, on the rays of the chosen angles)
  for i in range(len(case.pairs)):
    mo, md = sc.exact_ray_mp(src.xform, focal, t[i], phi[i])
    for k in range(3):
      assert abs(sc._mp_to_long(md[k]) - ed[i, k]) <= 2.0 ** -61
      assert abs(sc._mp_to_long(mo[k]) - eo[i, k]) <= 2.0 ** -61 * (np.abs(eo[i]).max() + (abs(focal) if np.isfinite(focal) else abs(t[i])) + 1e-300)
  for who, (o, d) in (('host', host_rays(src, t, phi)), ('oracle', oracle.make_rays(src, case.first, case.n, case.seed))):
    rd, ro = sc.ray_ratios(focal, t, o, d, eo, ed)
    print(f'{who} {fr} f={focal:g}: direction {rd.max():.3f}, origin {ro.max():.3f} (x 2^-53 x scale)')
    measured[who][0] = max(measured[who][0], rd.max())
    measured[who][1] = max(measured[who][1], ro.max())
    # the host is what C rests on: C_HOST <= C / 4; the oracle (1 / length multiplied in, where the host divides) is
    # held to twice the host's figure
    lim = sc.C_HOST if who == 'host' else 2 * sc.C_HOST
    assert rd.max() <= lim and ro.max() <= lim, (who, rd.max(), ro.max())
    assert np.all(np.abs(np.sqrt((d.astype(L) ** 2).sum(axis=1)) - 1) <= 4 * EPS)


def test_c_host_is_what_was_measured(measured):
  """runs after the cases above: the constant in source_cases.py is the measured figure rounded up, not a guess"""
  assert sc.C_HOST == sc.C / 4
  worst = max(measured['host'])
  print('C_host measured', measured, 'C_HOST', sc.C_HOST, 'C', sc.C)
  if worst:                                  # (the ray cases ran in this session)
    assert worst <= sc.C_HOST
    assert sc.C_HOST <= 2 * worst + 1        # (not a bound so wide that it says nothing)
