"""Scenes and rays for the box screens and box faces of the compiled kernels' general loop (odw_kernels.hip: spec_prim with
LEAN -- ray_box_centred on |1/d| and -(o/d) handed in as values (spec_reciprocals), the flat entry faces of an untrimmed
box in intersect_prim).  Neither changes a value: a compiled kernel's rows are the generic kernel's.  Built with the
helpers of spec_image_cases and spec_isolated_cases; shared by tests/test_spec_screens_build.py (CPU: every header
compiles, the oracle records rows for every case, the census of the headline kernel) and tests/test_gpu_spec_screens.py
(compiled rows against generic rows as byte strings)."""
import os

import numpy as np

import spec_image_cases as cases
import spec_isolated_cases as ic

N = 20000
SEED = 0x0D15EA5E
TOL = 1e-6
SCENES = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'scenes')


def golden(name):
  from freecad.optics_design_workbench_amd import scenes
  return scenes.bakeProject(os.path.join(SCENES, name + '.FCStd'))


def source_frame(pr):
  """(origin, x, y, z) of the project's point source: the columns of its 3 x 4 frame"""
  m = np.asarray(pr.source.xform, np.float64).reshape(3, 4)
  return m[:, 3].copy(), m[:, 0].copy(), m[:, 1].copy(), m[:, 2].copy()


# ---- (a) lensesAndMirrors -----------------------------------------------------------------------------------------------
def rays_headline(pr, seed=51, n=N, mixed=False):
  """a coherent beam from the project's source along its axis; mixed: neighbouring ray indices alternate between the
  beam, a start moved 12 mm sideways and a direction tilted by 0.35 rad -- three different paths"""
  rs = np.random.RandomState(seed)
  o0, ex, ey, ez = source_frame(pr)
  a, b = rs.normal(0, 0.01, n), rs.normal(0, 0.01, n)
  o = np.tile(o0, (n, 1))
  if mixed:
    k = np.arange(n) % 3
    o[k == 1] += 12.0 * ex
    a[k == 2] += 0.35
  d = ez[None, :] + a[:, None] * ex[None, :] + b[:, None] * ey[None, :]
  return o, cases.unit(d)


# ---- (b) lens trains: 7 and 13 primitives with a box of their own ------------------------------------------------------
def train(n_own):
  """a lens train with n_own box-owning primitives: n_own - 2 lenses (three operands share one box each), a mirror, a screen"""
  return cases.lens_train(n_own - 2)


def own_boxes(native, pr):
  info = native.spec_image(pr.scene, pr.limits)
  box_of = np.asarray(info['box_of'])
  return int(np.count_nonzero((box_of == np.arange(len(box_of))) & (np.asarray(info['box']) >= 0))), bool(info['in_arguments'])


def rays_train(seed=52, n=N):
  rs = np.random.RandomState(seed)
  o = np.c_[rs.normal(0, 2.5, n), rs.normal(0, 2.5, n), np.zeros(n)]
  d = np.c_[rs.normal(0, 0.03, n), rs.normal(0, 0.03, n), np.ones(n)]
  wide = np.arange(n) % 4 == 3                        # (onto the mirror beside the axis and past the lenses)
  d[wide] = np.c_[rs.normal(0.25, 0.1, n), rs.normal(0, 0.1, n), np.ones(n)][wide]
  return o, cases.unit(d)


# ---- (c) zero components, origins on box planes, grazed edges ----------------------------------------------------------
GRAZE = (0.0, 2.0, -2.0)        # of distTol


def rays_edges_exact(seed=53, n=N):
  """rays along the edges of small_scene's axis-aligned box, 0 and +-2 distTol off them: along +z past its x and y
  edges, along +x over its z edges, and diagonally in the x-z plane onto its edge lines"""
  g = cases.SMALL
  rs = np.random.RandomState(seed)
  delta = np.asarray(GRAZE)[np.arange(n) % len(GRAZE)] * TOL
  k = (np.arange(n) // len(GRAZE)) % 4
  x0, y0, z0 = g['box_lo']
  sx, sy, sz = g['box_size']
  o = np.zeros((n, 3))
  d = np.tile([0.0, 0.0, 1.0], (n, 1))
  o[k == 0] = np.c_[x0 + rs.choice([0.0, sx], n) + delta, rs.uniform(y0, y0 + sy, n), np.zeros(n)][k == 0]
  o[k == 1] = np.c_[rs.uniform(x0, x0 + sx, n), y0 + rs.choice([0.0, sy], n) + delta, np.zeros(n)][k == 1]
  m = k == 2
  o[m] = np.c_[np.full(n, x0 - 20.0), rs.uniform(y0, y0 + sy, n), z0 + rs.choice([0.0, sz], n) + delta][m]
  d[m] = [1.0, 0.0, 0.0]
  m = k == 3                                          # 45 degrees in the x-z plane through the edge x = x0, z = z0 (+ delta)
  o[m] = np.c_[np.full(n, x0 - 15.0) + delta, rs.uniform(y0, y0 + sy, n), np.full(n, z0 - 15.0)][m]
  d[m] = [1.0, 0.0, 1.0]
  return o, cases.unit(d)


def special_rays(native, pr, kind):
  rs = np.random.RandomState(dict(zero1=54, zero2=55, origins=56, edges=57)[kind])
  if kind == 'zero1':
    return cases.rays_zero_components(rs, N, 1)
  if kind == 'zero2':
    return cases.rays_zero_components(rs, N, 2)
  if kind == 'origins':
    boxes = native.spec_image(pr.scene, pr.limits)['boxes']
    return cases.rays_special_origins(rs, N, boxes[boxes[:, 0] < 1e29])
  return rays_edges_exact()


SPECIAL = ('zero1', 'zero2', 'origins', 'edges')


# ---- (d) a ray leaving a convex lens whose operands share a box --------------------------------------------------------
def rays_leaving(seed=58, n=N):
  """origins inside lens A of spec_isolated_cases' bench: the first hit leaves the lens, and on the next segment the
  lens is the skipped solid while its sphere's box block is still the one its cylinder shares"""
  return ic.rays_inside(seed, n)


# ---- (f) a batch of three scenes whose boxes differ --------------------------------------------------------------------
def batch():
  return [ic.bench(side_mirror=x) for x in (ic.AWAY, ic.AWAY + 3.0, ic.AWAY + 7.5)]
