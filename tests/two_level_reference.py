"""scipy restatement of the two-level preconditioner of the Newton-Raphson CG solve (pinn_fem_amd/coarse.py on the
host, pf_pcg2_* in pinn_fem_amd/csrc/pf_pcg.hip on the device):

    M^-1 r = D^-1 r + Z (Z^T K Z)^-1 Z^T r,   D = diag(K_ff)

Test infrastructure only: used on the CPU by tests/test_two_level_host.py and on the GPU by tests/test_pcg_two_level.py.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import f64_reference as ref

RTOL = 1e-13


def z_matrix(cs):
    """Z [n_dofs, n_coarse] as CSR, built entry by entry from the per-dof coefficient layout (independent of
    CoarseSpace.to_sparse)."""
    rows, cols, vals = [], [], []
    for node in range(cs.n_nodes):
        a = int(cs.node_agg[node])
        off, k = int(cs.agg_off[a]), int(cs.agg_off[a + 1] - cs.agg_off[a])
        for c in range(cs.dim):
            dof = node * cs.dim + c
            for m in range(k):
                rows.append(dof); cols.append(off + m); vals.append(cs.zcoef[dof, m])
    return sp.csr_matrix((vals, (rows, cols)), shape=(cs.n_nodes * cs.dim, cs.n_coarse))


class TwoLevel:
    """The preconditioner from CPU matrices: K (all dofs, CSR), the fixed mask and a CoarseSpace.  a_inv: use this
    inverse (e.g. the one a device engine uploaded) instead of the host pipeline's own."""

    def __init__(self, K, mask, cs, a_inv=None):
        from pinn_fem_amd.coarse import coarse_inverse
        self.n = K.shape[0]
        self.cs, self.mask = cs, np.asarray(mask, dtype=bool)
        self.Z = z_matrix(cs)
        self.Kff = ref.restrict_ff(K, self.mask)
        self.dinv = ref.jacobi_dinv(K, self.mask)
        self.A = (self.Z.T @ (self.Kff @ self.Z)).toarray() if cs.n_coarse else np.zeros((0, 0))
        self.a_inv = coarse_inverse(self.A) if a_inv is None else np.asarray(a_inv, dtype=np.float64)

    def apply(self, r):
        r = np.where(self.mask, 0.0, r)
        return self.dinv * r + self.Z @ (self.a_inv @ (self.Z.T @ r))

    def apply_abs(self, r):
        """|D^-1||r| + |Z| |A^-1| |Z|^T |r|: the scale of the round-off of one application."""
        r = np.abs(np.where(self.mask, 0.0, r))
        Za = abs(self.Z)
        return self.dinv * r + Za @ (np.abs(self.a_inv) @ (Za.T @ r))

    def operator(self):
        return spla.LinearOperator((self.n, self.n), matvec=self.apply, dtype=np.float64)


def cg(Kff, b, M, maxiter):
    """scipy's CG at rtol 1e-13 with a counting callback: (x, iterations, info)."""
    n_it = [0]
    y, info = spla.cg(Kff, b, rtol=RTOL, atol=0.0, maxiter=maxiter, M=M,
                      callback=lambda _: n_it.__setitem__(0, n_it[0] + 1))
    return y, n_it[0], info


def jacobi_operator(K, mask):
    dinv = ref.jacobi_dinv(K, mask)
    return spla.LinearOperator(K.shape, matvec=lambda v: dinv * v, dtype=np.float64)


def direct_solve(K, mask, b):
    free = np.flatnonzero(~np.asarray(mask, dtype=bool))
    out = np.zeros(K.shape[0])
    out[free] = spla.spsolve(K[free][:, free].tocsc(), np.asarray(b, dtype=np.float64)[free])
    return out


def mesh_system(nodes, el, fixed, dim, ea=1.0):
    """(K CSR over all dofs, fixed mask) of a truss with E*A = ea from its float64 coordinates."""
    nodes = np.asarray(nodes, dtype=np.float64)
    n_nodes = len(nodes)
    geo = ref.geo_f64(nodes, el, dim)
    K = ref.k_csr(geo, el, ea / geo[:, 3], dim, n_nodes)
    mask = np.zeros(n_nodes * dim, dtype=bool)
    mask[np.asarray(fixed, dtype=int)] = True
    return K, mask
