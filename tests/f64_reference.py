"""CPU float64 reference of the Newton-Raphson linear algebra (pinn_fem_amd/csrc/pf_pcg.hip): the truss
stiffness as a scipy CSR matrix, a plain NumPy restatement of the Jacobi-PCG recurrence, and a vectorised
generator of well-conditioned test trusses.  Test infrastructure only; verified on the CPU by
tests/test_f64_reference.py, used on the GPU by tests/test_pcg_f64.py.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp


def geo_f64(nodes, conn, dim):
    """Per-element (c2, cs, s2, l0) in float64 from float64 node coordinates (1-D: 1, 0, 0, |xj - xi|)."""
    nodes = np.asarray(nodes, dtype=np.float64)
    conn = np.asarray(conn, dtype=np.int64)
    if dim == 1:
        l0 = np.abs(nodes[conn[:, 1]] - nodes[conn[:, 0]])
        return np.stack([np.ones_like(l0), np.zeros_like(l0), np.zeros_like(l0), l0], axis=1)
    d = nodes[conn[:, 1]] - nodes[conn[:, 0]]
    l0 = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    cx, cy = d[:, 0] / l0, d[:, 1] / l0
    return np.stack([cx * cx, cx * cy, cy * cy, l0], axis=1)


def _k_coo(geo, conn, s, dim, n_nodes, absolute):
    geo = np.asarray(geo, dtype=np.float64)
    conn = np.asarray(conn, dtype=np.int64)
    s = np.asarray(s, dtype=np.float64)
    ni, nj = conn[:, 0], conn[:, 1]
    if dim == 1:
        dofs = np.stack([ni, nj], axis=1)                                     # [ne, 2]
        pat = np.array([[1.0, -1.0], [-1.0, 1.0]])
        ke = s[:, None, None] * pat[None]
    else:
        c2, cs, s2 = geo[:, 0], geo[:, 1], geo[:, 2]
        dofs = np.stack([2 * ni, 2 * ni + 1, 2 * nj, 2 * nj + 1], axis=1)     # [ne, 4]
        blk = np.stack([np.stack([c2, cs], -1), np.stack([cs, s2], -1)], -2)  # [ne, 2, 2]
        pat = np.concatenate([np.concatenate([blk, -blk], -1), np.concatenate([-blk, blk], -1)], -2)
        ke = s[:, None, None] * pat
    if absolute:
        ke = np.abs(ke)
    nd = dofs.shape[1]
    rows = np.repeat(dofs, nd, axis=1).reshape(-1)
    cols = np.tile(dofs, (1, nd)).reshape(-1)
    n = n_nodes * dim
    return sp.coo_matrix((ke.reshape(-1), (rows, cols)), shape=(n, n))


def k_csr(geo, conn, s, dim, n_nodes=None):
    """K = sum of s_e * pattern_e as a float64 CSR matrix [n_dofs, n_dofs].  geo: [ne, 4] (c2, cs, s2, l0),
    s: [ne] = E*A/l0.  2-D pattern: [[B, -B], [-B, B]], B = [[c2, cs], [cs, s2]]; 1-D: [[1, -1], [-1, 1]]."""
    n_nodes = int(np.max(conn)) + 1 if n_nodes is None else int(n_nodes)
    K = _k_coo(geo, conn, s, dim, n_nodes, False).tocsr()
    # scipy sums duplicate entries in no particular order; the diagonal (the only entry with more than one
    # contribution unless two elements join the same nodes) is summed here in ascending element id, the order
    # pf_pcg.hip documents, so that 1/diag can be compared to the last bits whatever the node degree
    d = element_order_diagonal(geo, conn, s, dim, n_nodes)
    K = (K + sp.diags(d - K.diagonal())).tocsr()          # d - K_ii is exact (Sterbenz), and so is K_ii + it
    return K


def element_order_diagonal(geo, conn, s, dim, n_nodes):
    """diag(K), each dof's sum taken over its elements in ascending element id (np.bincount adds in input order)."""
    geo = np.asarray(geo, dtype=np.float64)
    conn = np.asarray(conn, dtype=np.int64)
    s = np.asarray(s, dtype=np.float64)
    elem_major = conn.reshape(-1)                           # e0.i, e0.j, e1.i, e1.j, ...
    if dim == 1:
        return np.bincount(elem_major, weights=np.repeat(s, 2), minlength=n_nodes)
    out = np.zeros(2 * n_nodes)
    out[0::2] = np.bincount(elem_major, weights=np.repeat(s * geo[:, 0], 2), minlength=n_nodes)
    out[1::2] = np.bincount(elem_major, weights=np.repeat(s * geo[:, 2], 2), minlength=n_nodes)
    return out


def abs_k_csr(geo, conn, s, dim, n_nodes=None):
    """sum of |ke| per element: (|K| |v|) from it is the scale of the round-off of K v."""
    n_nodes = int(np.max(conn)) + 1 if n_nodes is None else int(n_nodes)
    return _k_coo(geo, conn, s, dim, n_nodes, True).tocsr()


def restrict_ff(K, fixed_mask):
    """K_ff embedded in the full dof numbering: rows and columns of fixed dofs zeroed (the device carries
    fixed dofs as zeros instead of dropping them)."""
    free = sp.diags((~np.asarray(fixed_mask, dtype=bool)).astype(np.float64))
    out = (free @ K @ free).tocsr()
    out.eliminate_zeros()
    return out


def jacobi_dinv(K, fixed_mask):
    """1 / diag(K_ff); 0 on fixed dofs and where the diagonal is 0 (pf_pcg.hip: k_pcg_init)."""
    d = np.asarray(K.diagonal(), dtype=np.float64)
    ok = (~np.asarray(fixed_mask, dtype=bool)) & (d != 0.0)
    out = np.zeros_like(d)
    out[ok] = 1.0 / d[ok]
    return out


def pcg_reference(Kff, dinv, b, rtol, n_iter, snapshots=()):
    """The recurrence of pf_pcg.hip in plain NumPy float64.
      start  x = 0, r = b, z = dinv*r, p = z; stopped at once when b.b = 0
      step   alpha = r.z / p.Ap (0 if p.Ap = 0); x += alpha p; r -= alpha Ap; z = dinv*r;
             beta = r.z_new / r.z (0 if r.z = 0); stop when r.r <= rtol^2 b.b or r.z_new = 0;
             p = z + beta p unless stopped
    b must be zero on fixed dofs (the caller masks it).  Returns x, r, p, state = (iterations, stopped,
    r.r, b.b), the iteration at which it stopped (None if it did not within n_iter) and a dict
    {k: (x, r.r)} for every k in `snapshots` that was reached."""
    b = np.asarray(b, dtype=np.float64)
    x = np.zeros_like(b)
    r = b.copy()
    z = dinv * r
    p = z.copy()
    rz, bb = float(r @ z), float(b @ b)
    rr = bb
    done = bb == 0.0
    it = 0
    snaps = {}
    want = set(int(k) for k in snapshots)
    while it < n_iter and not done:
        ap = Kff @ p
        pap = float(p @ ap)
        alpha = rz / pap if pap != 0.0 else 0.0
        x += alpha * p
        r -= alpha * ap
        z = dinv * r
        rz_new, rr = float(r @ z), float(r @ r)
        beta = rz_new / rz if rz != 0.0 else 0.0
        rz = rz_new
        it += 1
        done = rr <= rtol * rtol * bb or rz_new == 0.0
        if not done:
            p = z + beta * p
        if it in want:
            snaps[it] = (x.copy(), rr)
    return x, r, p, (it, bool(done), rr, bb), (it if done else None), snaps


def pinned_grid_truss(side, rng, pin=8, jitter=0.3):
    """Jittered side x side grid truss: elements to the (1,0), (0,1), (1,1), (1,-1) neighbours, element
    order shuffled, orientation flipped at random, every `pin`-th node in both directions fully fixed.
    Every free node is then at most `pin` grid steps from a support, so the Jacobi-preconditioned
    condition number does not grow with `side`.  Returns (nodes [n, 2], elements [ne, 2], fixed dofs)."""
    side = int(side)
    i, j = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    i, j = i.reshape(-1), j.reshape(-1)
    nodes = np.stack([i, j], axis=1) + rng.uniform(-jitter, jitter, (side * side, 2))
    node_id = i * side + j
    parts = []
    for di, dj in ((1, 0), (0, 1), (1, 1), (1, -1)):
        ok = (i + di < side) & (j + dj < side) & (j + dj >= 0)
        parts.append(np.stack([node_id[ok], (i[ok] + di) * side + (j[ok] + dj)], axis=1))
    el = np.concatenate(parts, axis=0)
    el = el[rng.permutation(len(el))]
    flip = rng.random(len(el)) < 0.5
    el[flip] = el[flip][:, ::-1]
    pinned = node_id[(i % pin == 0) & (j % pin == 0)]
    fixed = np.sort(np.concatenate([2 * pinned, 2 * pinned + 1]))
    return nodes, np.ascontiguousarray(el), fixed


def pinned_bar(n_nodes, rng, pin=64):
    """Non-uniform 1-D bar (element lengths U(0.5, 1.5)) with every `pin`-th node fixed."""
    x = np.concatenate([[0.0], np.cumsum(0.5 + rng.random(n_nodes - 1))])
    e = np.arange(n_nodes - 1, dtype=np.int64)
    return x, np.stack([e, e + 1], axis=1), np.arange(0, n_nodes, pin, dtype=np.int64)
