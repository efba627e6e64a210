"""M and qfrc_bias of a state from the Lagrange equations, in NumPy float64: a reference that shares nothing with CRBA or RNE.

The only thing taken from the C oracle is Oracle.fk (link origins and quaternions), which the fk_* fixtures and the
central-difference Jacobian tests already pin.  From it, for every body b with mass m_b, centre of mass c_b, rotation R_b and principal
inertias I_b about the link-frame axes:
    M(q)   = sum_b  m_b Jp_b^T Jp_b  +  Jr_b^T R_b diag(I_b) R_b^T Jr_b          (geometric centre-of-mass Jacobians)
    V(q)   = - sum_b m_b g . c_b,        dV/dq_i = - sum_b m_b g . Jp_b[:, i]
    bias_i = sum_jk dM_ij/dq_k v_k v_j  -  1/2 sum_jk dM_jk/dq_i v_j v_k  +  dV/dq_i       (arm dofs)
dM/dq_k comes from central differences of M at the steps h and h / 2 and is Richardson-extrapolated, (4 D(h/2) - D(h)) / 3; the
distance |bias(h) - bias(h/2)| between the two unextrapolated evaluations is the reference's own error estimate (it bounds the error
of the coarser of the two, so it overstates that of the extrapolated value).  The cube is a free body whose angular velocity is
held in its body frame: its block of M is diag(m, m, m, I_0, I_1, I_2) and its bias rows are [-m g, w x (I w)].

M is linear in the principal inertias, and so is the bias: a State keeps the mass part and one part per (link, axis), so the same
evaluation serves any inertia assignment -- the sensitivity controls of tests/test_aniso_inertia_cpu.py swap principal values in
the reference without touching the code under test."""
import numpy as np

from regime_states import quat2mat

H = 1e-4          # central-difference steps H and H / 2 on the joint positions (rad, m)


class Tree:
    """The constants of a compiled model's kinematic tree that the Lagrange equations need."""

    def __init__(self, cm):
        d = cm.desc
        nl = self.nl = cm.nlink
        self.nv = cm.nv
        self.mass = np.array([d.mass[i] for i in range(nl)])
        self.com = np.array([list(d.com[i]) for i in range(nl)])
        self.axis = np.array([list(d.jnt_axis[i]) for i in range(nl)])
        self.slide = np.array([d.jnt_type[i] == 1 for i in range(nl)])
        self.gravity = np.array(list(d.gravity))
        self.cube_mass = float(d.cube_mass)
        self.anc = np.zeros((nl, nl))                       # anc[b, j] = 1: joint j moves body b
        for b in range(nl):
            j = b
            while j >= 0:
                self.anc[b, j] = 1.0
                j = d.link_parent[j]


def parts(tree, orc, qpos):
    """(Mm[nl, nl], A[nl, 3, nl, nl], dV[nl]) at qpos: M = Mm + sum_bk I_bk A[b, k] over the arm dofs, and the gravity forces."""
    xpos, xquat, _, _ = orc.fk(qpos)
    xmat = np.stack([quat2mat(q) for q in xquat])                                # [b, 3, 3]
    axis = np.einsum("jrc,jc->jr", xmat, tree.axis)                              # world joint axes [j, 3]
    cpos = xpos + np.einsum("brc,bc->br", xmat, tree.com)
    arm = cpos[:, None, :] - xpos[None, :, :]                                    # [b, j, 3]: joint j's origin to body b's centre of mass
    jp = np.where(tree.slide[None, :, None], axis[None, :, :], np.cross(axis[None, :, :], arm)) * tree.anc[:, :, None]      # [b, j, 3]
    jr = np.where(tree.slide[None, :, None], 0.0, axis[None, :, :]) * tree.anc[:, :, None]
    Mm = np.einsum("b,bic,bjc->ij", tree.mass, jp, jp)
    u = np.einsum("brk,bjr->bkj", xmat, jr)                                      # u[b, k] = Jr_b^T R_b e_k
    A = np.einsum("bki,bkj->bkij", u, u)
    dV = -np.einsum("b,c,bjc->j", tree.mass, tree.gravity, jp)
    return Mm, A, dV


def _velocity_products(D, v):
    """c_i = sum_jk D[k, i, j] v_k v_j - 1/2 sum_jk D[i, j, k] v_j v_k for D[k] = dM/dq_k; any leading axes of M ride along."""
    return np.einsum("k...ij,k,j->...i", D, v, v) - 0.5 * np.einsum("i...jk,j,k->...i", D, v, v)


class State:
    """The Lagrange reference at one state, for any inertia assignment."""

    def __init__(self, tree, orc, qpos, qvel, h=H):
        nl = tree.nl
        self.tree = tree
        self.qvel = np.asarray(qvel, dtype=np.float64)
        qpos = np.asarray(qpos, dtype=np.float64)
        v = self.qvel[:nl]
        self.Mm, self.A, self.dV = parts(tree, orc, qpos)
        self.cm_, self.cA = [], []                          # velocity products of the mass part and of every (link, axis) part at h, h / 2
        for step in (h, 0.5 * h):
            Dm, DA = np.zeros((nl, nl, nl)), np.zeros((nl, nl, 3, nl, nl))
            for k in range(nl):
                qa, qb = qpos.copy(), qpos.copy()
                qa[k] += step; qb[k] -= step
                ma, aa, _ = parts(tree, orc, qa)
                mb, ab, _ = parts(tree, orc, qb)
                Dm[k], DA[k] = (ma - mb) / (2 * step), (aa - ab) / (2 * step)
            self.cm_.append(_velocity_products(Dm, v))
            self.cA.append(_velocity_products(DA, v))

    def M(self, link_inertia, cube_inertia):
        t = self.tree
        M = np.zeros((t.nv, t.nv))
        M[:t.nl, :t.nl] = self.Mm + np.einsum("bk,bkij->ij", np.asarray(link_inertia), self.A)
        M[t.nl:, t.nl:] = np.diag([t.cube_mass] * 3 + list(cube_inertia))
        return M

    def cube_euler(self, cube_inertia):
        w = self.qvel[self.tree.nl + 3:self.tree.nl + 6]
        return np.cross(w, np.asarray(cube_inertia) * w)

    def bias(self, link_inertia, cube_inertia, euler_sign=1.0):
        """(bias[nv], err): the Richardson-extrapolated bias and |bias(h) - bias(h / 2)|, the largest entry."""
        t = self.tree
        I = np.asarray(link_inertia)
        at = [self.cm_[s] + np.einsum("bk,bki->i", I, self.cA[s]) for s in range(2)]
        out = np.zeros(t.nv)
        out[:t.nl] = (4.0 * at[1] - at[0]) / 3.0 + self.dV
        out[t.nl:t.nl + 3] = -t.cube_mass * t.gravity
        out[t.nl + 3:] = euler_sign * self.cube_euler(cube_inertia)
        return out, float(np.abs(at[0] - at[1]).max())


def reference(cm, orc, qpos, qvel, h=H):
    """dict(M, bias, err, state) of one state for the compiled model's own inertias."""
    d = cm.desc
    I = np.array([list(d.inertia[i]) for i in range(cm.nlink)])
    Ic = np.array(list(d.cube_inertia))
    st = State(Tree(cm), orc, qpos, qvel, h)
    b, err = st.bias(I, Ic)
    return dict(M=st.M(I, Ic), bias=b, err=err, state=st)
