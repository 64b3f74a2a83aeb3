"""Float64 restatement of the mesh steps of one float32 gradient-descent iteration (support module, no tests).

What the node and element kernels of pf_mesh.hip compute from the per-element fields the nets would have written
(k_node_residual, k_elem_adjoint, k_node_gradu with and without the fused Adam step, k_finalize, k_reset, k_adam,
k_diag_k, k_coo_k), restated in numpy float64 from exactly the float32 values the device reads, widened: the plan's
geometry (c2, cs, s2, l0), connectivity, dof flags, f_ext and meas_val; u; E and A per element (or the scalar `scale` of
a property without a net); and the stiffness record (E*A)/l0 times c2, cs, s2, each product rounded to float32 as
elem_k_from (pf_common.h) does, so the record's own rounding is an INPUT of the comparison, not part of its error.

It also holds
  * a float32 stand-in of the gathers (numpy float32, ascending element id, an fma emulated as one float64 multiply-add
    rounded to float32) that the host test holds to the same bounds and mutates (Incidences);
  * the bounds, each derived from rounding counts next to its function;
  * the mesh, field and flag builders the host and the device tests share.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from helpers import _random_truss

f32, f64 = np.float32, np.float64
EPS32 = 2.0 ** -24
PF_DOF_FIXED, PF_DOF_MEASURED = 1, 2
B1, B2, ADAM_EPS = 0.9, 0.999, 1e-8
NODE_THREADS, NODE_BLOCK_CAP = 256, 1024      # PF_NODE_THREADS, pf_node_blocks (pf_mesh.hip)


# ---------------------------------------------------------------------------------------------------
# the mesh as the device reads it
# ---------------------------------------------------------------------------------------------------
@dataclass
class Mesh:
    """The arrays of a pinn_fem_amd.plan.HostPlan the mesh kernels read, and the incidences in gather order."""
    dim: int
    n_nodes: int
    n_elems: int
    conn: np.ndarray          # int64 [n_elems, 2]
    egeo: np.ndarray          # float32 [n_elems, 4]: c2, cs, s2, l0
    flags: np.ndarray         # uint8 [n_dofs]
    f_ext: np.ndarray         # float32 [n_dofs]
    meas_val: np.ndarray      # float32 [n_dofs]
    n_meas: int
    adj_ptr: np.ndarray       # int64 [n_nodes + 1]
    inc_node: np.ndarray      # int64 [2 n_elems]: the incidences, node by node, ascending element id inside a node
    inc_elem: np.ndarray
    inc_end: np.ndarray       # 0: the node is the element's i end, 1: its j end
    inc_other: np.ndarray     # the node at the element's other end

    @property
    def n_dofs(self):
        return self.n_nodes * self.dim

    @property
    def degree(self):
        return np.diff(self.adj_ptr)

    @property
    def fixed(self):
        return (self.flags & PF_DOF_FIXED) != 0

    @property
    def measured(self):
        return (self.flags & PF_DOF_MEASURED) != 0

    def dof_degree(self):
        return np.repeat(self.degree, self.dim)


def mesh_from_plan(hp) -> Mesh:
    adj = np.asarray(hp.adj, dtype=np.int64)
    ptr = np.asarray(hp.adj_ptr, dtype=np.int64)
    return Mesh(dim=hp.dim, n_nodes=hp.n_nodes, n_elems=hp.n_elems, conn=np.asarray(hp.conn, dtype=np.int64).reshape(-1, 2),
                egeo=np.asarray(hp.egeo, dtype=f32).reshape(-1, 4), flags=np.asarray(hp.dof_flags, dtype=np.uint8),
                f_ext=np.asarray(hp.f_ext, dtype=f32), meas_val=np.asarray(hp.meas_val, dtype=f32), n_meas=int(hp.n_meas),
                adj_ptr=ptr, inc_node=np.repeat(np.arange(hp.n_nodes, dtype=np.int64), np.diff(ptr)), inc_elem=adj >> 1,
                inc_end=adj & 1, inc_other=np.asarray(hp.adj_other, dtype=np.int64))


def records(mesh: Mesh, E, A) -> np.ndarray:
    """The stiffness record of every element [n_elems, 3] in float32, by the device's operations (elem_stiffness,
    elem_k_from): s = (E * A) / l0, then s c2, s cs, s s2 (1-D: s, 0, 0), every operation rounded to float32.  E, A: float32
    per element, or a scalar (a property without a net: its `scale`)."""
    E = np.broadcast_to(np.asarray(E, dtype=f32), (mesh.n_elems,))
    A = np.broadcast_to(np.asarray(A, dtype=f32), (mesh.n_elems,))
    s = ((E * A).astype(f32) / mesh.egeo[:, 3]).astype(f32)
    if mesh.dim == 1:
        z = np.zeros_like(s)
        return np.stack([s, z, z], axis=1)
    return np.stack([(s * mesh.egeo[:, k]).astype(f32) for k in range(3)], axis=1)


def record_image(mesh: Mesh, rec: np.ndarray) -> np.ndarray:
    """pf_problem.elem_k's layout: 3 floats per element in 2-D, 1 in 1-D."""
    return np.ascontiguousarray(rec if mesh.dim == 2 else rec[:, 0], dtype=f32).reshape(-1)


# ---------------------------------------------------------------------------------------------------
# the gather (K v)[node] = sum over the node's incidences of the element's rows at that end
# ---------------------------------------------------------------------------------------------------
@dataclass
class Incidences:
    """What each incidence of the stand-in's gather reads; the defaults restate the kernel, a mutant changes one entry."""
    rec_of: np.ndarray        # element whose record the incidence reads
    sign: np.ndarray          # +1; -1 negates the incidence's rows
    s2_as_cs: np.ndarray      # True: row 1 reads cs where it should read s2
    keep: np.ndarray          # False: the incidence is left out of the sum


def incidences(mesh: Mesh) -> Incidences:
    n = mesh.inc_elem.size
    return Incidences(mesh.inc_elem.copy(), np.ones(n), np.zeros(n, dtype=bool), np.ones(n, dtype=bool))


def _ends(mesh: Mesh, v, dtype):
    """(v at the element's i end, at its j end) for every incidence, [n_inc, dim]."""
    v = np.asarray(v, dtype=dtype).reshape(mesh.n_nodes, mesh.dim)
    own, oth = v[mesh.inc_node], v[mesh.inc_other]
    e1 = (mesh.inc_end == 1)[:, None]
    return np.where(e1, oth, own), np.where(e1, own, oth)


def gather64(mesh: Mesh, rec: np.ndarray, v):
    """(K v, S) per dof in float64 from the float32 records and v, widened.  S is the scale of the dof's round-off:
    sum over the node's incidences of |ke_ab| (|v_i,b| + |v_j,b|) over the row's entries b."""
    k = rec.astype(f64)[mesh.inc_elem]
    vi, vj = _ends(mesh, v, f64)
    sg = np.where(mesh.inc_end == 1, -1.0, 1.0)
    av = np.abs(vi) + np.abs(vj)
    if mesh.dim == 2:
        row0 = sg * (k[:, 0] * (vi[:, 0] - vj[:, 0]) + k[:, 1] * (vi[:, 1] - vj[:, 1]))
        row1 = sg * (k[:, 1] * (vi[:, 0] - vj[:, 0]) + k[:, 2] * (vi[:, 1] - vj[:, 1]))
        fe = np.stack([row0, row1], axis=1)
        mag = np.stack([np.abs(k[:, 0]) * av[:, 0] + np.abs(k[:, 1]) * av[:, 1],
                        np.abs(k[:, 1]) * av[:, 0] + np.abs(k[:, 2]) * av[:, 1]], axis=1)
    else:
        fe = (sg * k[:, 0] * (vi[:, 0] - vj[:, 0]))[:, None]
        mag = (np.abs(k[:, 0]) * av[:, 0])[:, None]
    out, S = np.zeros((mesh.n_nodes, mesh.dim)), np.zeros((mesh.n_nodes, mesh.dim))
    for c in range(mesh.dim):
        out[:, c] = np.bincount(mesh.inc_node, weights=fe[:, c], minlength=mesh.n_nodes)
        S[:, c] = np.bincount(mesh.inc_node, weights=mag[:, c], minlength=mesh.n_nodes)
    return out.reshape(-1), S.reshape(-1)


def gather_bound(mesh: Mesh, S):
    """(degree + 8) 2^-24 S per dof.  A record entry carries three roundings (E A, / l0, times the pattern entry), but the
    reference is GIVEN the rounded record, so they cost nothing here; the row of an incidence is one product and three fma
    (fe_mode 0; fe_mode 1: two differences, a product and an fma), at most four roundings, each of a partial sum no larger
    than the incidence's share of S; the `degree` accumulations round partial sums no larger than S.  4 + degree, held at
    degree + 8 (the count the record's three would have brought, plus one: the margin is stated, not fitted)."""
    return (mesh.dof_degree() + 8.0) * EPS32 * np.asarray(S, dtype=f64)


def _fma32(a, b, c):
    """fmaf on float32 arrays: the float64 product of two float32 is exact, one float64 add, one rounding to float32."""
    return (a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(f32)


def incidence_rows32(mesh: Mesh, rec: np.ndarray, v, fe_mode: int, inc: Optional[Incidences] = None) -> np.ndarray:
    """ke_rows_times (pf_common.h) of every incidence in float32, [n_inc, dim]."""
    inc = inc or incidences(mesh)
    k = np.asarray(rec, dtype=f32)[inc.rec_of]
    vi, vj = _ends(mesh, v, f32)
    sg = (np.where(mesh.inc_end == 1, -1.0, 1.0) * inc.sign).astype(f32)
    if mesh.dim == 1:
        kc = (sg * k[:, 0]).astype(f32)
        if fe_mode == 1:
            return ((-kc) * (vj[:, 0] - vi[:, 0]).astype(f32)).astype(f32)[:, None]
        return _fma32(-kc, vj[:, 0], (kc * vi[:, 0]).astype(f32))[:, None]
    c2, cs = k[:, 0], k[:, 1]
    s2 = np.where(inc.s2_as_cs, k[:, 1], k[:, 2])
    if fe_mode == 1:
        d0, d1 = (vj[:, 0] - vi[:, 0]).astype(f32), (vj[:, 1] - vi[:, 1]).astype(f32)
        q0 = _fma32(cs, d1, (c2 * d0).astype(f32))
        q1 = _fma32(s2, d1, (cs * d0).astype(f32))
        return np.stack([(-sg * q0).astype(f32), (-sg * q1).astype(f32)], axis=1)
    a, b, c = (sg * c2).astype(f32), (sg * cs).astype(f32), (sg * s2).astype(f32)
    r0 = _fma32(-b, vj[:, 1], _fma32(-a, vj[:, 0], _fma32(b, vi[:, 1], (a * vi[:, 0]).astype(f32))))
    r1 = _fma32(-c, vj[:, 1], _fma32(-b, vj[:, 0], _fma32(c, vi[:, 1], (b * vi[:, 0]).astype(f32))))
    return np.stack([r0, r1], axis=1)


def gather32(mesh: Mesh, rec: np.ndarray, v, fe_mode: int = 0, inc: Optional[Incidences] = None) -> np.ndarray:
    """The float32 stand-in of gather_kv: every incidence's rows in float32, added in ascending element id, one float32
    addition each, starting from 0."""
    inc = inc or incidences(mesh)
    fe = incidence_rows32(mesh, rec, v, fe_mode, inc)
    acc = np.zeros((mesh.n_nodes, mesh.dim), dtype=f32)
    deg, ptr = mesh.degree, mesh.adj_ptr[:-1]
    for k in range(int(deg.max()) if deg.size else 0):
        nodes = np.flatnonzero(deg > k)
        idx = ptr[nodes] + k
        live = inc.keep[idx]
        nodes, idx = nodes[live], idx[live]
        acc[nodes] = (acc[nodes] + fe[idx]).astype(f32)
    return acc.reshape(-1)


# ---------------------------------------------------------------------------------------------------
# residual, loss sums, monitors
# ---------------------------------------------------------------------------------------------------
def residual64(mesh: Mesh, f_int, lam, alpha_physics):
    """(r, g_f) per dof in float64 (dof_residual, pf_node.h): 0 on fixed dofs; lam and alpha_physics as the float32 the
    record holds."""
    lam, ap = f64(f32(lam)), f64(f32(alpha_physics))
    r = np.where(mesh.fixed, 0.0, np.asarray(f_int, dtype=f64) - lam * mesh.f_ext.astype(f64))
    return r, ap * r


def residual_bound(mesh: Mesh, f_int, S, lam, alpha_physics):
    """Bound on |g_f - alpha r|: the gather's bound on f, then three roundings (lam fx, the difference, the product with
    alpha), each of a value no larger than |f| + |lam fx|; all of it times alpha.  0 on fixed dofs: they must be exact."""
    lam, ap = f64(f32(lam)), abs(f64(f32(alpha_physics)))
    b = ap * (gather_bound(mesh, S) + 3.0 * EPS32 * (np.abs(np.asarray(f_int, dtype=f64)) + np.abs(lam * mesh.f_ext.astype(f64))))
    return np.where(mesh.fixed, 0.0, b)


def residual32(mesh: Mesh, f_int32, lam, alpha_physics, leak_fixed: Optional[int] = None):
    """Stand-in of dof_residual in float32.  leak_fixed (mutant): this fixed dof keeps its residual in g_f."""
    lam, ap = f32(lam), f32(alpha_physics)
    r = (np.asarray(f_int32, dtype=f32) - (lam * mesh.f_ext).astype(f32)).astype(f32)
    live = ~mesh.fixed
    if leak_fixed is not None:
        live = live.copy()
        live[leak_fixed] = True
    r = np.where(live, r, f32(0.0))
    return r, (ap * r).astype(f32)


def terms_per_thread(mesh: Mesh) -> int:
    """How many dof terms one thread of a node kernel adds to its float32 sum: its nodes of the grid-stride walk."""
    nb = min(max((mesh.n_nodes + NODE_THREADS - 1) // NODE_THREADS, 1), NODE_BLOCK_CAP)
    return -(-mesh.n_nodes // (nb * NODE_THREADS)) * mesh.dim


def sum_bound(mesh: Mesh) -> float:
    """Relative bound of a loss sum or monitor: (terms per thread + 12) 2^-24.  Every term is a square, so a rounding of any
    partial sum is relative to the total.  A term's product is 1 rounding and the thread's chain 1 per term; the wave tree 6
    (64 lanes); the block's 4 waves 3 (4 counted with the first addition to 0); the double combine of the block partials
    adds nothing visible; its cast to float 1.  That is terms + 11 for sum r^2, sum d^2, sum u^2; every monitor adds at most
    one more RELATIVE rounding to what it is compared on (0.5 s is exact, sqrt halves the error of s and rounds once,
    s / n_meas rounds once); loss_total is compared through its two terms (total_bound)."""
    return (terms_per_thread(mesh) + 12.0) * EPS32


def loss_terms64(mesh: Mesh, g_f_dev, u, use_data: bool, alpha_physics, alpha_data):
    """The monitors of finalize_body in float64 from the device's own g_f (alpha_physics = 1: g_f is r to the bit;
    otherwise g_f / alpha) and d formed in float64."""
    ap, ad = f64(f32(alpha_physics)), f64(f32(alpha_data))
    r = np.asarray(g_f_dev, dtype=f64) / ap
    sum_r2 = float(np.sum(np.where(mesh.fixed, 0.0, r * r)))
    sum_d2 = 0.0
    if use_data:
        d = mesh.meas_val.astype(f64) - np.asarray(u, dtype=f64)
        sum_d2 = float(np.sum(np.where(mesh.measured, d * d, 0.0)))
    lp = 0.5 * sum_r2
    ld = sum_d2 / mesh.n_meas if use_data else 0.0
    return dict(sum_r2=sum_r2, sum_d2=sum_d2, loss_physics=lp, loss_data=ld,
                loss_total=ap * lp + (ad * ld if use_data else 0.0), residual_norm=float(np.sqrt(sum_r2)))


def total_bound(mesh: Mesh, ref: dict, use_data: bool, alpha_physics, alpha_data) -> float:
    """Absolute bound of loss_total = alpha_p loss_p + alpha_d loss_d: both terms' relative bounds, and 3 more roundings
    (two products, the sum) of values no larger than the sum of the two terms."""
    ap, ad = abs(f64(f32(alpha_physics))), abs(f64(f32(alpha_data)))
    tot = ap * ref["loss_physics"] + (ad * ref["loss_data"] if use_data else 0.0)
    return (sum_bound(mesh) + 3.0 * EPS32) * tot


# ---------------------------------------------------------------------------------------------------
# element adjoint
# ---------------------------------------------------------------------------------------------------
def gea64(mesh: Mesh, g_f, u):
    """(g_ea, bound) per element (pf_elem_gea): sum_ab g_a pattern_ab u_b / l0 in float64 from the float32 pattern, and
    12 2^-24 sum |g_a| |pattern_ab| |u_b| / l0.  Count: a row of pattern @ u_e is a product and three fma (4), the two dots
    with g add four fma (4), the division 1: 9 in the longest chain through any term, in fe_mode 1 fewer; held at 12."""
    g = np.asarray(g_f, dtype=f64).reshape(mesh.n_nodes, mesh.dim)
    uu = np.asarray(u, dtype=f64).reshape(mesh.n_nodes, mesh.dim)
    i, j = mesh.conn[:, 0], mesh.conn[:, 1]
    geo = mesh.egeo.astype(f64)
    l0 = geo[:, 3]
    if mesh.dim == 1:
        pu = uu[i, 0] - uu[j, 0]
        val = (g[i, 0] - g[j, 0]) * pu
        mag = (np.abs(g[i, 0]) + np.abs(g[j, 0])) * (np.abs(uu[i, 0]) + np.abs(uu[j, 0]))
        return val / l0, 12.0 * EPS32 * mag / l0
    c2, cs, s2 = geo[:, 0], geo[:, 1], geo[:, 2]
    d0, d1 = uu[i, 0] - uu[j, 0], uu[i, 1] - uu[j, 1]
    a0, a1 = np.abs(uu[i, 0]) + np.abs(uu[j, 0]), np.abs(uu[i, 1]) + np.abs(uu[j, 1])
    p0, p1 = c2 * d0 + cs * d1, cs * d0 + s2 * d1
    m0, m1 = np.abs(c2) * a0 + np.abs(cs) * a1, np.abs(cs) * a0 + np.abs(s2) * a1
    val = (g[i, 0] - g[j, 0]) * p0 + (g[i, 1] - g[j, 1]) * p1
    mag = (np.abs(g[i, 0]) + np.abs(g[j, 0])) * m0 + (np.abs(g[i, 1]) + np.abs(g[j, 1])) * m1
    return val / l0, 12.0 * EPS32 * mag / l0


# ---------------------------------------------------------------------------------------------------
# dL/du, Adam
# ---------------------------------------------------------------------------------------------------
def data_term64(mesh: Mesh, u, use_data: bool, alpha_data):
    """-(alpha_d / n_meas) 2 (meas - u) on the measured dofs with use_data, else 0 (dof_grad_u)."""
    if not use_data or mesh.n_meas == 0:
        return np.zeros(mesh.n_dofs)
    d = mesh.meas_val.astype(f64) - np.asarray(u, dtype=f64)
    return np.where(mesh.measured, -(f64(f32(alpha_data)) / mesh.n_meas) * 2.0 * d, 0.0)


def grad_u64(mesh: Mesh, rec, g_f, u, use_data: bool, alpha_data):
    """(grad_u, bound) per dof: K^T g_f by the same gather (K symmetric) + the data term.  The bound is the gather's, whose
    spare rounding covers the final addition on the gather's scale, plus 4 ulp of the data term: the difference d, the
    quotient alpha_d / n_meas, their product (2 d is exact) and the final addition on the data term's scale."""
    g, S = gather64(mesh, rec, g_f)
    dt = data_term64(mesh, u, use_data, alpha_data)
    return g + dt, gather_bound(mesh, S) + 4.0 * EPS32 * np.abs(dt)


def grad_u32(mesh: Mesh, rec, g_f32, u32, use_data: bool, alpha_data, fe_mode=0, inc=None, force_data_on: Optional[int] = None):
    """Stand-in of k_node_gradu's gradient in float32.  force_data_on (mutant): this dof gets the data term whatever
    use_data says."""
    g = gather32(mesh, rec, g_f32, fe_mode, inc)
    on = mesh.measured & bool(use_data)
    if force_data_on is not None:
        on = on.copy()
        on[force_data_on] = True
    dcoef = f32(alpha_data) / f32(mesh.n_meas) if mesh.n_meas else f32(0.0)
    d = (mesh.meas_val - np.asarray(u32, dtype=f32)).astype(f32)
    t = (-(dcoef * (f32(2.0) * d).astype(f32)).astype(f32)).astype(f32)
    return np.where(on, (g + t).astype(f32), g)


def adam_scalars(lr, t: int):
    """(step_size, bc2_sqrt) of Adam step t >= 1 as k_reset (t = 1) and finalize_body form them: double arithmetic on the
    float32 learning rate, cast to float."""
    bc1, bc2 = 1.0 - B1 ** t, 1.0 - B2 ** t
    return f32(f64(f32(lr)) / bc1), f32(np.sqrt(bc2))


def adam64(p, m, v, g, step_size, bc2s):
    """One torch.optim.Adam step in float64 (dof_adam_u, k_adam) from float32 state, the given gradient and the step's two
    float32 scalars.  Returns (p, m, v, bound_p, bound_m, bound_v).  Bounds, from the kernel's operations (no contraction:
    PF_NO_CONTRACT), each rounding relative to the magnitudes it acts on:
      m = m + b1w (g - m): difference, product, sum and the constant b1w rounded to float: 4 of |m| + |g|;
      v = v b2 + (b2w g) g: three products, a sum and the two constants: 6 of |v| + g^2;
      p = p - step (m / (sqrt(v) / bc2s + eps)): sqrt, quotient, sum, quotient, product, sum and eps rounded to float: 7,
        held at 9, of |p| + step |m| / denom; plus what the moments' own errors move m / denom."""
    p, m, v, g = (np.asarray(x, dtype=f64) for x in (p, m, v, g))
    step, bc2s = f64(step_size), f64(bc2s)
    m1 = m + (1.0 - B1) * (g - m)
    v1 = v * B2 + (1.0 - B2) * g * g
    sq = np.sqrt(v1)
    denom = sq / bc2s + ADAM_EPS
    ratio = m1 / denom
    p1 = p - step * ratio
    bm = 4.0 * EPS32 * (np.abs(m) + np.abs(g))
    bv = 6.0 * EPS32 * (np.abs(v) + g * g)
    d_denom = np.where(sq > 0, bv / (2.0 * np.where(sq > 0, sq, 1.0)) / bc2s, np.sqrt(bv) / bc2s)
    bp = 9.0 * EPS32 * (np.abs(p) + step * np.abs(ratio)) + step * (bm / denom + np.abs(ratio) * d_denom / denom)
    return p1, m1, v1, bp, bm, bv


def adam32(p, m, v, g, step_size, bc2s):
    """Stand-in of dof_adam_u in float32: every operation rounded once, in the kernel's order."""
    p, m, v, g = (np.asarray(x, dtype=f32) for x in (p, m, v, g))
    b1w, b2, b2w, eps = f32(1.0 - B1), f32(B2), f32(1.0 - B2), f32(ADAM_EPS)
    m1 = (m + (b1w * (g - m).astype(f32)).astype(f32)).astype(f32)
    v1 = (v * b2).astype(f32)
    v1 = (v1 + ((b2w * g).astype(f32) * g).astype(f32)).astype(f32)
    denom = ((np.sqrt(v1).astype(f32) / f32(bc2s)).astype(f32) + eps).astype(f32)
    p1 = (p + ((-f32(step_size)) * (m1 / denom).astype(f32)).astype(f32)).astype(f32)
    return p1, m1, v1


def gea32(mesh: Mesh, g_f32, u32, fe_mode=0):
    """Stand-in of pf_elem_gea in float32: the unit-stiffness rows at both ends, two fma dots, one division."""
    unit = np.stack([mesh.egeo[:, 0], mesh.egeo[:, 1], mesh.egeo[:, 2]], axis=1) if mesh.dim == 2 else \
        np.stack([np.ones(mesh.n_elems, dtype=f32)] + [np.zeros(mesh.n_elems, dtype=f32)] * 2, axis=1)
    # an element-ordered view of incidence_rows32: incidence 2e is element e's i end, 2e + 1 its j end
    em = Mesh(mesh.dim, mesh.n_nodes, mesh.n_elems, mesh.conn, mesh.egeo, mesh.flags, mesh.f_ext, mesh.meas_val, mesh.n_meas,
              mesh.adj_ptr, mesh.conn.reshape(-1), np.repeat(np.arange(mesh.n_elems), 2),
              np.tile(np.array([0, 1]), mesh.n_elems), mesh.conn[:, ::-1].reshape(-1))
    pu = incidence_rows32(em, unit, u32, fe_mode).reshape(mesh.n_elems, 2, mesh.dim)
    g = np.asarray(g_f32, dtype=f32).reshape(mesh.n_nodes, mesh.dim)
    gs = np.zeros(mesh.n_elems, dtype=f32)
    for end in (0, 1):
        for c in range(mesh.dim):
            gs = _fma32(g[mesh.conn[:, end], c], pu[:, end, c], gs)
    return (gs / mesh.egeo[:, 3]).astype(f32)


def ulp32(x):
    return np.spacing(np.abs(f32(x)))


# ---------------------------------------------------------------------------------------------------
# diag(K), K in coordinate format
# ---------------------------------------------------------------------------------------------------
def diag64(mesh: Mesh, rec):
    """(diag K, bound) per dof (k_diag_k): the sum of the record's c2 (dof x) or s2 (dof y) over the node's incidences;
    (degree + 4) 2^-24 sum |ke_ii|: one rounding per accumulation, the record's own roundings being inputs."""
    k = rec.astype(f64)[mesh.inc_elem]
    cols = [k[:, 0], k[:, 2]] if mesh.dim == 2 else [k[:, 0]]
    out = np.stack([np.bincount(mesh.inc_node, weights=c, minlength=mesh.n_nodes) for c in cols], axis=1).reshape(-1)
    mag = np.stack([np.bincount(mesh.inc_node, weights=np.abs(c), minlength=mesh.n_nodes) for c in cols], axis=1).reshape(-1)
    return out, (mesh.dof_degree() + 4.0) * EPS32 * mag


def coo64(mesh: Mesh, rec):
    """(rows, cols, vals) of k_coo_k: entry a * nd + b of element e at e * nd^2 + that, nd = 2 dim."""
    nd = 2 * mesh.dim
    k = rec.astype(f64)
    rows = np.zeros((mesh.n_elems, nd, nd), dtype=np.int64)
    cols, vals = np.zeros_like(rows), np.zeros((mesh.n_elems, nd, nd))
    for a in range(nd):
        for b in range(nd):
            na, nb = mesh.conn[:, a // mesh.dim], mesh.conn[:, b // mesh.dim]
            ca, cb = a % mesh.dim, b % mesh.dim
            rows[:, a, b], cols[:, a, b] = na * mesh.dim + ca, nb * mesh.dim + cb
            base = k[:, 0] if mesh.dim == 1 or (ca == 0 and cb == 0) else (k[:, 2] if ca and cb else k[:, 1])
            vals[:, a, b] = base if (a // mesh.dim) == (b // mesh.dim) else -base
    return rows.reshape(-1), cols.reshape(-1), vals.reshape(-1)


# ---------------------------------------------------------------------------------------------------
# meshes, flags, fields
# ---------------------------------------------------------------------------------------------------
@dataclass
class Case:
    """A mesh with its loads, supports and measurements, as build_host_plan / FEMModel take them."""
    name: str
    dim: int
    nodes: np.ndarray
    elements: np.ndarray
    loads: np.ndarray
    fixed: np.ndarray
    meas_vals: np.ndarray
    meas_dofs: np.ndarray
    u: np.ndarray = field(default=None)       # float32 displacements of the case
    notes: dict = field(default_factory=dict)

    def plan(self, with_meas=True):
        from pinn_fem_amd.plan import build_host_plan
        return build_host_plan(self.nodes, self.elements, self.loads, self.fixed, self.dim,
                               self.meas_vals if with_meas else None, self.meas_dofs if with_meas else None)

    def mesh(self, with_meas=True) -> Mesh:
        return mesh_from_plan(self.plan(with_meas))


SMALL_SIZES = (2, 3, 255, 256, 257, 511, 513)     # node counts on both sides of one and two 256-thread blocks
LONG_NODES = 786_509      # 1024 blocks x 256 threads x 2 nodes cover 524 288: a second trip whose second node 77 threads have


def _dress(name, dim, nodes, elements, rng, ramp=False) -> Case:
    """Loads, supports, measurements and u of a case: f_ext non-zero on every dof, the fixed ones included; fixed dofs
    (node 0 and every 17th dof) with non-zero u; every third dof measured, one of them fixed as well."""
    n_nodes = len(nodes)
    n_dofs = n_nodes * dim
    loads = rng.standard_normal(n_dofs)
    loads[np.abs(loads) < 0.05] = 0.5
    fixed = np.unique(np.concatenate([np.arange(dim), np.arange(5, n_dofs, 17)]))
    md = np.unique(np.concatenate([np.arange(0, n_dofs, 3), fixed[-1:]]))
    u = rng.standard_normal(n_dofs)
    u[np.abs(u) < 0.05] = 0.25
    if ramp:
        # the cancellation case of the chain tests: u grows to 700 along the chain with O(1) differences between neighbours
        x = np.arange(n_nodes) / max(n_nodes - 1, 1)
        u = u.reshape(n_nodes, dim)
        u[:, 0] = 700.0 * x * (1.0 + 0.05 * np.sin(7.0 * x)) + 0.3 * u[:, 0]
        u = u.reshape(-1)
    u = u.astype(f32)
    mv = u[md].astype(f64) + 0.1 * rng.standard_normal(md.size)
    return Case(name, dim, nodes, np.asarray(elements, dtype=np.int64), loads, fixed, mv, md, u)


def grid_case(n_nodes, seed=0) -> Case:
    rng = np.random.default_rng(1000 + n_nodes + seed)
    nodes, el = _random_truss(n_nodes, rng)
    return _dress(f"grid{n_nodes}", 2, nodes, el, rng)


def chain_case(n_nodes, dim, seed=0, ramp=False) -> Case:
    """An open path in node order (element e joins node e to node e + 1); 2-D: the nodes wander off the axis, so that cs
    and s2 are non-zero."""
    rng = np.random.default_rng(2000 + n_nodes + 7 * dim + seed)
    x = np.arange(n_nodes, dtype=f64) + rng.uniform(-0.2, 0.2, n_nodes)
    nodes = x if dim == 1 else np.stack([x, rng.uniform(-0.5, 0.5, n_nodes)], axis=1)
    e = np.arange(n_nodes - 1, dtype=np.int64)
    return _dress(f"chain{dim}d{n_nodes}" + ("ramp" if ramp else ""), dim, nodes, np.stack([e, e + 1], axis=1), rng, ramp)


def hub_case(seed=0) -> Case:
    """600 nodes: a 590-node jittered grid truss and ten more nodes: a hub joined to 301 grid nodes, nodes of degree 1, 2,
    3, 64 and 65, one node that no element touches, two nodes joined by two elements of which one is reversed (each of them
    tied to the grid by one more), and one of degree 2.  Element order shuffled, orientation random."""
    rng = np.random.default_rng(3000 + seed)
    n_grid = 590
    nodes, el = _random_truss(n_grid, rng)
    side = int(np.ceil(np.sqrt(n_grid)))
    extra = rng.uniform(0.0, side, (10, 2)) + 0.37          # off the grid's jitter boxes: no zero length
    nodes = np.concatenate([nodes, extra])
    hub, lonely, pa, pb = 590, 596, 597, 598
    want = {590: 301, 591: 1, 592: 2, 593: 3, 594: 64, 595: 65, 599: 2, pa: 1, pb: 1}
    new = []
    for n, deg in want.items():
        new += [(n, int(q)) for q in rng.choice(n_grid, size=deg, replace=False)]
    el = np.concatenate([el, np.array(new), np.array([[pa, pb], [pa, pb]])])
    rng.shuffle(el)
    flip = rng.random(len(el)) < 0.5
    el[flip] = el[flip][:, ::-1]
    twin = np.flatnonzero(((el[:, 0] == pa) & (el[:, 1] == pb)) | ((el[:, 0] == pb) & (el[:, 1] == pa)))
    el[twin[0]], el[twin[1]] = (pa, pb), (pb, pa)
    case = _dress("hub600", 2, nodes, el, rng)
    case.notes = dict(hub=hub, lonely=lonely, twin=(pa, pb), degrees={590: 301, 591: 1, 592: 2, 593: 3, 594: 64, 595: 65})
    return case


def fields(kind: str, n_elems: int, seed=0):
    """(E, A) per element in float32.  "decades": E = 10^U(-3,3), A = 10^U(-1,1); "uniform": within 5 % of 1; "softzone": a
    contiguous tenth of the elements at 1e-4 of the rest (the rest within 5 % of 1)."""
    rng = np.random.default_rng(4000 + seed + n_elems)
    if kind == "decades":
        return (10.0 ** rng.uniform(-3, 3, n_elems)).astype(f32), (10.0 ** rng.uniform(-1, 1, n_elems)).astype(f32)
    E = 1.0 + rng.uniform(-0.05, 0.05, n_elems)
    A = 1.0 + rng.uniform(-0.05, 0.05, n_elems)
    if kind == "softzone":
        lo = (4 * n_elems) // 10
        E[lo:lo + max(n_elems // 10, 1)] *= 1e-4
    elif kind != "uniform":
        raise ValueError(kind)
    return E.astype(f32), A.astype(f32)


def worst_ratio(err, bound):
    """max err / bound over the entries with a positive bound; an entry whose bound is 0 must be exact (else inf)."""
    err, bound = np.abs(np.asarray(err, dtype=f64)).reshape(-1), np.asarray(bound, dtype=f64).reshape(-1)
    pos = bound > 0
    if np.any(err[~pos] != 0):
        return np.inf
    return float(np.max(err[pos] / bound[pos])) if pos.any() else 0.0


def standin_ratios(mesh: Mesh, rec, u, lam, alpha_physics, alpha_data, use_data: bool, fe_mode: int, seed=0) -> dict:
    """Worst error / bound of the float32 stand-in per quantity on one case: the yardstick a device ratio is read against."""
    u = np.asarray(u, dtype=f32)
    out = {}
    f64_, S = gather64(mesh, rec, u)
    f32_ = gather32(mesh, rec, u, fe_mode)
    out["f_int"] = worst_ratio(f32_ - f64_, gather_bound(mesh, S))
    _, g64 = residual64(mesh, f64_, lam, alpha_physics)
    _, g32 = residual32(mesh, f32_, lam, alpha_physics)
    out["g_f"] = worst_ratio(g32 - g64, residual_bound(mesh, f64_, S, lam, alpha_physics))
    ge64, ge_b = gea64(mesh, g32, u)
    out["g_ea"] = worst_ratio(gea32(mesh, g32, u, fe_mode) - ge64, ge_b)
    gu64, gu_b = grad_u64(mesh, rec, g32, u, use_data, alpha_data)
    gu32 = grad_u32(mesh, rec, g32, u, use_data, alpha_data, fe_mode)
    out["grad_u"] = worst_ratio(gu32 - gu64, gu_b)
    rng = np.random.default_rng(5000 + seed)
    m0 = (0.1 * rng.standard_normal(mesh.n_dofs)).astype(f32)
    v0 = (0.01 * rng.random(mesh.n_dofs)).astype(f32)
    step, bc2s = adam_scalars(1e-3, 1)
    p64, m64, v64, bp, bm, bv = adam64(u, m0, v0, gu32, step, bc2s)
    p32, m32, v32 = adam32(u, m0, v0, gu32, step, bc2s)
    out["adam_u"], out["adam_m"], out["adam_v"] = worst_ratio(p32 - p64, bp), worst_ratio(m32 - m64, bm), worst_ratio(v32 - v64, bv)
    return out
