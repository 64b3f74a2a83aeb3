"""Coarse space of the two-level preconditioner of the Newton-Raphson CG solve (host, float64).

    M^-1 r = D^-1 r + Z (Z^T K Z)^-1 Z^T r,    D = diag(K_ff)

Z holds, per aggregate of nodes, the rigid-body modes of that aggregate (2-D: two translations and the rotation
about the aggregate's centroid; 1-D: the translation), zero on fixed dofs.  What survives the masking is decided
per aggregate from the 3 x 3 Gram matrix of its masked columns; the survivors are orthonormalised.  Z is never
formed on the device: it is held as per-dof coefficients (at most 3 coarse columns touch a dof).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

MAX_AGGREGATES = 256           # coarse dimension <= 768: the device kernels size their LDS by it
MODES = 3                      # coarse columns per aggregate at most (pf_coarse.zcoef is [n_dofs][3])
GRAM_DROP = 1e-12              # directions below this fraction of the aggregate's largest Gram eigenvalue are dropped
# "two-level-updated": the two-level preconditioner of the Green-Lagrange tangent solve, its columns rebuilt on the current
# configuration X + u and Z^T K_t Z re-formed and re-factored at every Newton iteration (update_coarse_space)
PRECONDITIONERS = ("jacobi", "two-level", "two-level-updated")


@dataclass
class CoarseSpace:
    dim: int
    n_nodes: int
    n_agg: int
    n_coarse: int              # columns of Z
    node_agg: np.ndarray       # int32 [n_nodes] aggregate of every node
    agg_off: np.ndarray        # int32 [n_agg+1] first coarse column of every aggregate
    zcoef: np.ndarray          # float64 [n_dofs, 3]: Z[dof, agg_off[a] + k] = zcoef[dof, k], a = aggregate of the dof's node
    agg_ptr: np.ndarray        # int32 [n_agg+1] aggregate -> its nodes in agg_nodes
    agg_nodes: np.ndarray      # int32 [n_nodes] node ids, ascending inside an aggregate (fixed summation order)

    def columns_of(self, a: int) -> int:
        return int(self.agg_off[a + 1] - self.agg_off[a])

    def to_sparse(self):
        """Z as a scipy CSR matrix [n_dofs, n_coarse] (tests and host-side checks; the device never forms it)."""
        import scipy.sparse as sp
        n_dofs = self.n_nodes * self.dim
        dof_agg = np.repeat(self.node_agg.astype(np.int64), self.dim)
        ncols = (self.agg_off[1:] - self.agg_off[:-1]).astype(np.int64)
        rows, cols, vals = [], [], []
        for k in range(MODES):
            ok = ncols[dof_agg] > k
            rows.append(np.flatnonzero(ok))
            cols.append(self.agg_off[dof_agg[ok]].astype(np.int64) + k)
            vals.append(self.zcoef[ok, k])
        return sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))),
                             shape=(n_dofs, self.n_coarse))


def check_preconditioner(name) -> str:
    if name not in PRECONDITIONERS:
        raise ValueError(f"unknown preconditioner {name!r}: expected one of {PRECONDITIONERS}")
    return name


def default_aggregate_count(n_nodes: int) -> int:
    return min(MAX_AGGREGATES, max(1, int(n_nodes) // 8))


def _coords(nodes, dim):
    x = np.asarray(nodes, dtype=np.float64)
    return x.reshape(-1, 1) if dim == 1 else x.reshape(-1, dim)


def strip_aggregates(nodes, dim: int, n_aggregates: Optional[int] = None) -> np.ndarray:
    """Equal-count strips along the coordinate axis of largest extent: node -> aggregate, int32.  The nodes are
    ranked by a stable sort on that coordinate (ties go to the other coordinate, then to the node id), so the map
    follows the geometry and not the node numbering.  n_aggregates above the node count is clamped; above
    MAX_AGGREGATES it raises."""
    x = _coords(nodes, dim)
    n = x.shape[0]
    if n_aggregates is None:
        n_aggregates = default_aggregate_count(n)
    n_aggregates = int(n_aggregates)
    if n_aggregates < 1:
        raise ValueError(f"n_aggregates must be >= 1, got {n_aggregates}")
    if n_aggregates > MAX_AGGREGATES:
        raise ValueError(f"n_aggregates must be <= {MAX_AGGREGATES}, got {n_aggregates}")
    n_aggregates = max(1, min(n_aggregates, n))
    if n == 0:
        return np.zeros(0, dtype=np.int32)
    axis = int(np.argmax(np.ptp(x, axis=0)))
    keys = [x[:, c] for c in range(x.shape[1]) if c != axis] + [x[:, axis]]      # lexsort: last key is the primary one
    order = np.lexsort(keys)
    out = np.empty(n, dtype=np.int32)
    out[order] = (np.arange(n, dtype=np.int64) * n_aggregates) // n
    return out


def build_coarse_space(nodes, dim: int, fixed_mask, n_aggregates: Optional[int] = None,
                       aggregates=None) -> CoarseSpace:
    """nodes: [n_nodes, dim] ([n_nodes] in 1-D); fixed_mask: bool [n_dofs].  aggregates: the caller's own
    node -> aggregate map (any integer labels, at most MAX_AGGREGATES distinct ones) instead of the strips."""
    x = _coords(nodes, dim)
    n = x.shape[0]
    fixed = np.asarray(fixed_mask, dtype=bool).reshape(n, dim)
    if aggregates is not None:
        labels = np.asarray(aggregates).reshape(-1)
        if labels.size != n:
            raise ValueError(f"aggregates must hold one entry per node ({n}), got {labels.size}")
        uniq, node_agg = np.unique(labels, return_inverse=True)
        if uniq.size > MAX_AGGREGATES:
            raise ValueError(f"aggregates name {uniq.size} aggregates; at most {MAX_AGGREGATES} are supported")
        node_agg = node_agg.astype(np.int32)
    else:
        node_agg = strip_aggregates(x if dim > 1 else x[:, 0], dim, n_aggregates)
    n_agg = int(node_agg.max()) + 1 if n else 1
    agg_nodes = np.argsort(node_agg, kind="stable").astype(np.int32)            # ascending node id inside an aggregate
    agg_ptr = np.zeros(n_agg + 1, dtype=np.int32)
    np.cumsum(np.bincount(node_agg, minlength=n_agg), out=agg_ptr[1:])
    zcoef = np.zeros((n * dim, MODES), dtype=np.float64)
    agg_off = np.zeros(n_agg + 1, dtype=np.int32)
    free = (~fixed).astype(np.float64)
    for a in range(n_agg):
        ids = agg_nodes[agg_ptr[a]:agg_ptr[a + 1]]
        raw = np.zeros((len(ids), dim, MODES))
        raw[:, 0, 0] = 1.0
        if dim == 2:
            raw[:, 1, 1] = 1.0
            d = x[ids] - x[ids].mean(axis=0)
            extent = float(np.max(np.abs(d))) if len(ids) else 0.0
            if extent > 0.0:                                  # lever arms over the extent: columns of comparable size
                raw[:, 0, 2] = -d[:, 1] / extent
                raw[:, 1, 2] = d[:, 0] / extent
        raw *= free[ids][:, :, None]
        R = raw.reshape(-1, MODES)
        lam, V = np.linalg.eigh(R.T @ R)
        keep = (lam > GRAM_DROP * lam[-1]) & (lam > 0.0) if lam[-1] > 0.0 else np.zeros(MODES, dtype=bool)
        k = int(keep.sum())
        cols = (R @ V[:, keep][:, ::-1]) / np.sqrt(lam[keep][::-1])             # largest direction first
        dofs = (ids.astype(np.int64)[:, None] * dim + np.arange(dim)[None, :]).reshape(-1)
        zcoef[dofs, :k] = cols
        agg_off[a + 1] = agg_off[a] + k
    zcoef[fixed.reshape(-1)] = 0.0
    return CoarseSpace(dim=dim, n_nodes=n, n_agg=n_agg, n_coarse=int(agg_off[-1]), node_agg=node_agg,
                       agg_off=agg_off, zcoef=np.ascontiguousarray(zcoef), agg_ptr=agg_ptr, agg_nodes=agg_nodes)


def update_coarse_space(coords, dim: int, fixed_mask, node_agg) -> CoarseSpace:
    """The coarse space on other coordinates with a FIXED node -> aggregate map: the rigid-body modes of every
    aggregate as it lies at `coords` (the current configuration X + u of a large-displacement solve, where the
    near-null space of the tangent is the rigid motions of the deformed body, not of the reference one).

    node_agg comes from the reference configuration, once per solve (strip_aggregates(X, ...) or the node_agg of the
    CoarseSpace built on X): the aggregates, and with them agg_ptr and agg_nodes, then stay what they are while the
    columns follow the body.  The per-aggregate column count may still differ between configurations, because the
    Gram drop is decided on the masked columns at the coordinates given (an aggregate whose free nodes line up under
    a centroid shift, for one): agg_off and n_coarse are therefore refreshed together with zcoef, never carried over."""
    return build_coarse_space(coords, dim, fixed_mask, aggregates=np.asarray(node_agg))


def coarse_inverse(a_c: np.ndarray) -> np.ndarray:
    """(Z^T K Z)^-1 from the matrix the device formed: symmetrise, Cholesky in float64, explicit inverse,
    symmetrise again.  Raises numpy.linalg.LinAlgError when the matrix is not positive definite."""
    a = np.asarray(a_c, dtype=np.float64)
    if a.size == 0:
        return np.zeros((0, 0))
    if not np.all(np.isfinite(a)):
        raise np.linalg.LinAlgError("coarse matrix holds non-finite entries")
    a = 0.5 * (a + a.T)
    L = np.linalg.cholesky(a)
    l_inv = np.linalg.solve(L, np.eye(a.shape[0]))
    inv = l_inv.T @ l_inv
    return 0.5 * (inv + inv.T)
