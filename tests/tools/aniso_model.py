"""Compiled models with anisotropic link and cube inertias: the test models of tests/test_aniso_inertia_*.py.

Every shipped asset gives every link and the cube three equal principal inertias, so R diag(I) R^T = I 1 whatever R is and
w x I w = 0: a transposed rotation, a principal value read twice or a missing gyroscopic term cannot move any output of the shipped
models.  with_inertias replaces desc.inertia and desc.cube_inertia -- three independent values per body, as include/kmanip.h
documents them -- and everything the model compiler derives from them; aniso is the canonical test model."""
import copy
import dataclasses
import itertools

import numpy as np

from gym_kmanip_amd.model import KModelDesc, invweight0

FACTORS = (0.6, 1.0, 1.5)                 # x the shipped value: every triple stays a physical inertia (1.5 <= 0.6 + 1.0)
CUBE_INERTIA = (0.001, 0.002, 0.0028)     # distinct, 0.0028 <= 0.001 + 0.002; the shipped cube is (0.002, 0.002, 0.002)
PERMUTATIONS = tuple(itertools.permutations(range(3)))


def is_physical(triple):
    """Each principal value at most the sum of the other two (the triangle inequalities of a mass distribution), all positive."""
    a, b, c = (float(x) for x in triple)
    return min(a, b, c) > 0 and a <= b + c and b <= a + c and c <= a + b


def with_inertias(cm, link_inertia, cube_inertia):
    """A copy of `cm` (as model.with_env_params makes one) whose desc has inertia[i] = link_inertia[i] and cube_inertia replaced,
    with everything model.invweight0 derives from them recomputed (dof_invweight0, body_invweight0, cube_invweight0, meaninertia),
    and a deep copy of the asset whose diaginertia entries say the same, so oracle.ik_scipy.NumpyArm and tools/mjcf_export.py see
    the same model.  With the shipped values the desc is byte-identical to cm.desc."""
    link_inertia = np.asarray(link_inertia, dtype=np.float64)
    cube_inertia = np.asarray(cube_inertia, dtype=np.float64)
    nl = cm.nlink
    assert link_inertia.shape == (nl, 3) and cube_inertia.shape == (3,)
    assert all(is_physical(t) for t in link_inertia) and is_physical(cube_inertia)
    d = KModelDesc.from_buffer_copy(cm.desc)
    for i in range(nl):
        for k in range(3):
            d.inertia[i][k] = link_inertia[i, k]
    for k in range(3):
        d.cube_inertia[k] = cube_inertia[k]
    dofw, bodyw, cubew, meaninertia = invweight0(d)
    for i in range(nl):
        d.dof_invweight0[i] = dofw[i]
        d.body_invweight0[i][0], d.body_invweight0[i][1] = bodyw[i]
    d.cube_invweight0[0], d.cube_invweight0[1] = cubew
    d.meaninertia = meaninertia
    asset = copy.deepcopy(cm.asset)
    for i, l in enumerate(asset["links"]):
        l["inertial"]["diaginertia"] = [float(x) for x in link_inertia[i]]
    asset["cube"]["diaginertia"] = [float(x) for x in cube_inertia]
    return dataclasses.replace(cm, desc=d, asset=asset)


def inertias(cm):
    """(link_inertia[nlink, 3], cube_inertia[3]) of a compiled model's desc."""
    d = cm.desc
    return np.array([list(d.inertia[i]) for i in range(cm.nlink)]), np.array(list(d.cube_inertia))


def permutations(nlink, seed=0):
    """One permutation of (0, 1, 2) per link, seeded, never the same for two consecutive links."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(nlink):
        choice = [p for p in PERMUTATIONS if not out or p != out[-1]]
        out.append(choice[int(rng.integers(len(choice)))])
    return out


def random_states(cm, n, seed):
    """(qpos[n, nq], qvel[n, nv]): hinges within 0.4 rad and finger slides within 4 mm of home, the cube at a random orientation over the table,
    and 0.5 .. 2.5 (rad/s, m/s) of either sign on EVERY dof, the cube's angular velocity included -- so every link turns about
    an axis that is not one of its own principal axes."""
    d = cm.desc
    nl = cm.nlink
    rng = np.random.default_rng(seed)
    qpos, qvel = np.zeros((n, cm.nq)), np.zeros((n, cm.nv))
    for e in range(n):
        qpos[e, :nl] = np.array(d.q_home[:nl]) + rng.uniform(-0.4, 0.4, nl) * np.where([d.jnt_type[i] == 1 for i in range(nl)], 0.01, 1.0)
        qpos[e, nl:nl + 3] = [0.5 * (d.table_rect[0] + d.table_rect[1]), 0.5 * (d.table_rect[2] + d.table_rect[3]), d.table_z + 0.2]
        q = rng.normal(size=4)
        qpos[e, nl + 3:nl + 7] = q / np.linalg.norm(q) * (1.0 if q[0] >= 0 else -1.0)
        qvel[e] = rng.uniform(0.5, 2.5, cm.nv) * rng.choice([-1.0, 1.0], cm.nv)
    return qpos, qvel


def aniso(cm, seed=0):
    """The canonical anisotropic test model: link i's three shipped values times FACTORS in the order permutations(nlink, seed)[i],
    the cube CUBE_INERTIA."""
    link0, _ = inertias(cm)
    f = np.array([[FACTORS[k] for k in p] for p in permutations(cm.nlink, seed)])
    return with_inertias(cm, link0 * f, CUBE_INERTIA)
