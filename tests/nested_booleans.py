"""Nested booleans (trimming lists of several clauses) for the tests: the per-clause expansion of a baked scene, the
reference form the frozen oracle can trace, and random nested trees.  TEST INFRASTRUCTURE.

A face whose trimming condition is a disjunction of conjunctions (Cut(Fuse(A, B), C): the faces of C are kept inside A
OR inside B) is baked as ONE primitive whose cond list holds several clauses (cond_inside bit 1 opens a clause).  The
oracle reads every list as one conjunction.  `expand` turns each primitive of k > 1 clauses into k primitives of one
clause each -- the original row keeps the first clause, copies of it (same kind, frame, parameters, group, solid,
flags and face mask) carry the others and are appended at the end; every other primitive's conditions still point at
the original row.  In default (non-strict) mode the expansion traces what the clause list traces:
  - the union of the copies' acceptance sets is the clause list's acceptance set;
  - two copies that accept the same point give the same distance and face, so the nearest-hit selection produces the
    same event;
  - the copy left behind at the new segment's start lies within distTol of it and is skipped like the original.
Tags carry ray | group | isEntering and no primitive index: the rows compare as they are."""
import copy

import numpy as np

from freecad.optics_design_workbench_amd.freecad_elements import make
from freecad.optics_design_workbench_amd.scene import Document, Placement, bake

from random_scenes import solid


def clauses_of(cond_inside, off, end):
  """[(first, end)] of the clauses of one list (bit 1 opens a clause; a list without it is one clause)"""
  starts = [c for c in range(off, end) if int(cond_inside[c]) & 2]
  if not starts:
    return [(off, end)] if end > off else []
  assert starts[0] == off, 'a list of several clauses marks its first condition too'
  return list(zip(starts, starts[1:] + [end]))


def n_clauses(scene):
  return [len(clauses_of(scene.cond_inside, int(scene.prim_cond_off[p]), int(scene.prim_cond_off[p + 1])))
          for p in range(scene.n_prims)]


def assert_conjunctive(scene):
  """what the oracle can be handed: no condition opens a clause (cond_inside 0 / 1 only)"""
  ci = np.asarray(scene.cond_inside)
  assert ci.size == 0 or set(np.unique(ci).tolist()) <= {0, 1}, sorted(set(ci.tolist()))


def expand(scene):
  """the per-clause expansion (module doc); a scene without clauses comes back equal"""
  n = scene.n_prims
  rows = list(range(n))                                   # row of the expansion -> row of the scene
  conds = []                                              # per row: [(prim, inside)]
  extra = []
  for p in range(n):
    cl = clauses_of(scene.cond_inside, int(scene.prim_cond_off[p]), int(scene.prim_cond_off[p + 1]))
    lits = [[(int(scene.cond_prim[c]), int(scene.cond_inside[c]) & 1) for c in range(a, b)] for a, b in cl]
    conds.append(lits[0] if lits else [])
    for more in lits[1:]:
      extra.append((p, more))
  for p, more in extra:
    rows.append(p)
    conds.append(more)
  idx = np.array(rows, dtype=np.int64)
  sc = copy.copy(scene)
  for name in ('prim_type', 'prim_group', 'prim_solid', 'prim_flags', 'prim_xform', 'prim_params'):
    setattr(sc, name, np.ascontiguousarray(np.asarray(getattr(scene, name))[idx]))
  for name in ('tri_normals', 'tri_edges'):
    if getattr(scene, name) is not None:
      setattr(sc, name, np.ascontiguousarray(np.asarray(getattr(scene, name))[idx]))
  sc.prim_sources = [scene.prim_sources[i] for i in rows] if scene.prim_sources else scene.prim_sources
  sc.prim_to_world = [scene.prim_to_world[i] for i in rows] if scene.prim_to_world else scene.prim_to_world
  off = [0]
  for lits in conds:
    off.append(off[-1] + len(lits))
  sc.prim_cond_off = np.array(off, dtype=np.int32)
  sc.cond_prim = np.array([q for lits in conds for q, _ in lits], dtype=np.int32)
  sc.cond_inside = np.array([i for lits in conds for _, i in lits], dtype=np.int32)
  assert_conjunctive(sc)
  return sc


# ---------------------------------------------------------------------------
# nested trees
# ---------------------------------------------------------------------------
PATTERNS = ['cut_fuse', 'common_fuse', 'cut_common', 'fuse_cut']


def nested_tree(doc, rs, tag, centre, pattern=None, depth=2):
  """one solid of the four disjunctive patterns -- Cut(Fuse(A, B), C), Common(Fuse(A, B), C), Cut(C, Common(A, B)),
  Fuse(Cut(A, B), D) --, operands placed off the axes around `centre`; depth 3 nests a pattern as an operand"""
  pattern = pattern or PATTERNS[rs.randint(len(PATTERNS))]
  k = [0]

  def leaf(spread=1.5):
    k[0] += 1
    return solid(doc, rs, f'{tag}_{k[0]}', centre + rs.normal(0, spread, 3))

  def operand():
    if depth > 2 and rs.rand() < 0.5:
      return nested_tree(doc, rs, f'{tag}n{k[0]}', centre + rs.normal(0, 1.0, 3), depth=depth - 1)
    return leaf()
  if pattern == 'cut_fuse':
    return make.makeCut(doc, make.makeFuse(doc, [operand(), leaf()], f'{tag}F'), leaf(1.0), f'{tag}X')
  if pattern == 'common_fuse':
    return make.makeCommon(doc, [make.makeFuse(doc, [operand(), leaf()], f'{tag}F'), leaf(1.0)], f'{tag}X')
  if pattern == 'cut_common':
    return make.makeCut(doc, leaf(1.0), make.makeCommon(doc, [operand(), leaf()], f'{tag}M'), f'{tag}X')
  return make.makeFuse(doc, [make.makeCut(doc, operand(), leaf(), f'{tag}C'), leaf()], f'{tag}X')


def nested_scene(rs, n_groups=None, optical=True, dist_tol=None):
  """-> (scene, limits, targets): 1-4 groups of one nested solid each (optical=False: all Vacuum), every group
  recording (a draw may simplify to plain conjunctions: callers count the scenes with clauses)"""
  doc = Document()
  targets = []
  for g in range(n_groups or rs.randint(1, 5)):
    centre = rs.uniform(-14, 14, 3)
    targets.append(centre)
    elem = nested_tree(doc, rs, f'G{g}', centre, depth=int(rs.choice([2, 3])))
    kind = rs.choice(['Mirror', 'Lens', 'Absorber', 'Vacuum'], p=[0.3, 0.4, 0.15, 0.15]) if optical else 'Vacuum'
    props = dict(RefractiveIndex=float(rs.uniform(1.2, 2.0))) if kind == 'Lens' else {}
    make.makeOpticalGroup(doc, kind, [elem], **props)
  settings = dict(MaxIntersections=float(rs.choice([6, 12, 30])))
  if dist_tol:
    settings['DistanceTolerance'] = dist_tol
  make.makeSimulationSettings(doc, **settings)
  src = make.makePointSource(doc)
  sc = bake.bakeScene(doc, src)
  sc.group_record = np.ones_like(sc.group_record)
  return sc, bake.bakeLimits(doc, src), np.array(targets), doc


def mount(doc, bore=2.5, base=(0.0, 0.0, 40.0), name='Mount'):
  """a lens mount: a tube fused with a flange, bored through along z (Cut(Fuse(tube, flange), bore)), off the axes"""
  pl = lambda *b: dict(placement=Placement(base=tuple(np.add(base, b))))
  tube = make.makeCylinder(doc, f'{name}Tube', 6.0, 12.0, **pl(0.0, 0.0, 0.0))
  flange = make.makeBox(doc, f'{name}Flange', 20.0, 20.0, 3.0, **pl(-10.0, -10.0, 0.0))
  hole = make.makeCylinder(doc, f'{name}Bore', bore, 30.0, **pl(0.4, -0.3, -9.0))
  return make.makeCut(doc, make.makeFuse(doc, [tube, flange], f'{name}Body'), hole, name)
