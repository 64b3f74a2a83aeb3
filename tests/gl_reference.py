"""The total-Lagrangian (Green-Lagrange) truss element in numpy / scipy float64: element state, internal force, tangent
as CSR, a Newton loop with a sparse direct solve, each with the initial (eigen-) strain as the keyword e0; the element-level
sensitivities, right-hand sides and strain maps the identification (tests/identify_reference.py) is built from; and the
closed forms the tests pin the element to.  Written from the virtual-work derivation, vectorised over elements with
scatter-adds; it shares no code with the kernels (which gather per node) or with pinn_fem_amd/fem.  tests/test_gl_host.py
checks it against finite differences, rigid motions and the two-bar closed form, tests/test_gl_e0_host.py with an e0.

  W(u) = sum_e  E A l0 (e - e0)^2 / 2,   e = (|d|^2 - |d0|^2) / (2 l0^2),  d = d0 + du
  N = E A (e - e0),   dW/du_j = (N / l0) d = fe,    d fe / d du = (E A / l0^3) d d^T + (N / l0) I = B
e0 < 0 is a pretension (T = -E A e0), thermal loading is e0 = alpha dT, lack of fit e0 = (L_natural - l0) / l0.  e0 acts
in full at every load factor.
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla


def _as2d(nodes, dim):
    return np.asarray(nodes, dtype=np.float64).reshape(-1, dim)


def element_state(nodes, el, u, ea, dim, e0=None):
    """(strain [ne] (the total strain e), fe [ne, dim], B [ne, dim, dim], terms) with `ea` and the initial strain `e0` a
    scalar or [ne]; e0 None: no initial strain, the bytes of e0 = 0.0.  `terms` holds what the round-off bounds of the GPU
    tests are stated in: d0, du, d, l0^2, l0, ea, the axial force n = E A (e - e0), e0 [ne] and
    e_abs = (2 |d0|.|du| + |du|.|du|) / (2 l0^2)."""
    X, el = _as2d(nodes, dim), np.asarray(el, dtype=np.int64)
    U = np.asarray(u, dtype=np.float64).reshape(-1, dim)
    d0 = X[el[:, 1]] - X[el[:, 0]]
    du = U[el[:, 1]] - U[el[:, 0]]
    d = d0 + du
    l02 = np.sum(d0 * d0, axis=1)
    l0 = np.sqrt(l02)
    # the difference of squares written out: |d|^2 - |d0|^2 = 2 d0.du + du.du
    strain = (2.0 * np.sum(d0 * du, axis=1) + np.sum(du * du, axis=1)) / (2.0 * l02)
    ea = np.broadcast_to(np.asarray(ea, dtype=np.float64), strain.shape)
    e0 = np.broadcast_to(np.asarray(0.0 if e0 is None else e0, dtype=np.float64), strain.shape)
    n = ea * (strain - e0)
    n_l0 = n / l0
    fe = n_l0[:, None] * d
    B = (ea / (l02 * l0))[:, None, None] * (d[:, :, None] * d[:, None, :]) + n_l0[:, None, None] * np.eye(dim)
    e_abs = (2.0 * np.sum(np.abs(d0) * np.abs(du), axis=1) + np.sum(du * du, axis=1)) / (2.0 * l02)
    return strain, fe, B, dict(d0=d0, du=du, d=d, l02=l02, l0=l0, ea=ea, n=n, e0=e0, e_abs=e_abs)


def axial_forces(nodes, el, u, ea, dim, e0=None):
    return element_state(nodes, el, u, ea, dim, e0)[3]["n"]


def energy(nodes, el, u, ea, dim, e0=None):
    strain, _, _, t = element_state(nodes, el, u, ea, dim, e0)
    return float(np.sum(t["ea"] * t["l0"] * (strain - t["e0"]) ** 2) / 2.0)


def _scatter(n_nodes, dim, el, term, sign):
    """[n_dofs]: per element, term [ne, dim] added at the second node and sign * term at the first."""
    out = np.zeros((n_nodes, dim))
    np.add.at(out, el[:, 1], term)
    np.add.at(out, el[:, 0], sign * term)
    return out.reshape(-1)


def f_int(nodes, el, u, ea, dim, absolute=False, e0=None):
    """Internal force [n_dofs]; absolute: the sum of the magnitudes of the same terms (the unit of round-off bounds)."""
    X, el = _as2d(nodes, dim), np.asarray(el, dtype=np.int64)
    fe = element_state(nodes, el, u, ea, dim, e0)[1]
    return _scatter(len(X), dim, el, np.abs(fe), 1.0) if absolute else _scatter(len(X), dim, el, fe, -1.0)


def f_int_scale(nodes, el, u, ea, dim, e0=None):
    """Per dof, the sum over the node's elements of |E A| (e_abs + |e0|) |d_c| / l0: the magnitude of the terms f_int is
    summed from, in front of the cancellation of e - e0 and of the sum over the node's elements, which does not vanish
    where the terms cancel (rigid motions)."""
    X, el = _as2d(nodes, dim), np.asarray(el, dtype=np.int64)
    t = element_state(nodes, el, u, ea, dim, e0)[3]
    mag = (np.abs(t["ea"]) * (t["e_abs"] + np.abs(t["e0"])) / t["l0"])[:, None] * np.abs(t["d"])
    return _scatter(len(X), dim, el, mag, 1.0)


def blocks_csr(B, el, n_nodes, dim, absolute=False):
    """Assemble element blocks B [ne, dim, dim]: [[B, -B], [-B, B]] on (i, j)."""
    el = np.asarray(el, dtype=np.int64)
    rows, cols, vals = [], [], []
    for a, sa in ((0, -1.0), (1, 1.0)):
        for b, sb in ((0, -1.0), (1, 1.0)):
            for r in range(dim):
                for c in range(dim):
                    rows.append(el[:, a] * dim + r)
                    cols.append(el[:, b] * dim + c)
                    v = B[:, r, c] * (sa * sb)
                    vals.append(np.abs(v) if absolute else v)
    n = n_nodes * dim
    return sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsr()


def k_t(nodes, el, u, ea, dim, absolute=False, e0=None):
    X = _as2d(nodes, dim)
    return blocks_csr(element_state(nodes, el, u, ea, dim, e0)[2], el, len(X), dim, absolute)


def free_mask(n, fixed):
    m = np.ones(n, dtype=bool)
    m[np.asarray(fixed, dtype=int)] = False
    return m


def restrict(K, free):
    idx = np.flatnonzero(free)
    return K[idx][:, idx].tocsc()


def min_eig_ff(K, free):
    """Smallest eigenvalue of K on the free dofs (dense: small systems only)."""
    return float(np.linalg.eigvalsh(restrict(K, free).toarray())[0])


def jacobi_cg(rtol=1e-13):
    """A linear solver for newton(): scipy's CG with the diag(K_ff) preconditioner, the device solve's yardstick."""
    def solve(Kff, rhs):
        dinv = 1.0 / Kff.diagonal()
        n = len(rhs)
        M = spla.LinearOperator((n, n), matvec=lambda v: dinv * v, dtype=np.float64)
        y, info = spla.cg(Kff.tocsr(), rhs, rtol=rtol, atol=0.0, maxiter=40 * n + 2000, M=M)
        assert info == 0
        return y
    return solve


def newton(nodes, el, loads, fixed, ea, dim, lam=1.0, u0=None, tol=1e-10, max_iter=50, min_den=1e-10, on_iterate=None,
           linear_solve=spla.spsolve, e0=None):
    """solve_nr's loop with a sparse direct solve: u += K_t(u)^-1 (lam f_ext - f_int(u)) until
    |du| / max(|u|, min_den) <= tol.  The load factor scales the loads only: the initial strain e0 acts in full.
    on_iterate(u, K, free, rhs) sees every iterate.  Returns (u, iterations, converged)."""
    n = len(_as2d(nodes, dim)) * dim
    free = free_mask(n, fixed)
    f = lam * np.asarray(loads, dtype=np.float64).reshape(-1)
    u = np.zeros(n) if u0 is None else np.where(free, np.asarray(u0, dtype=np.float64).reshape(-1), 0.0)
    for it in range(max_iter):
        K = k_t(nodes, el, u, ea, dim, e0=e0)
        rhs = f - f_int(nodes, el, u, ea, dim, e0=e0)
        if on_iterate is not None:
            on_iterate(u, K, free, rhs)
        du = np.zeros(n)
        du[free] = linear_solve(restrict(K, free), rhs[free])
        u = u + du
        if np.linalg.norm(du) / max(np.linalg.norm(u), min_den) <= tol:
            return u, it + 1, True
    return u, max_iter, False


def incremental(nodes, el, loads, fixed, ea, dim, n_inc, **kw):
    """solve()'s driver: n_inc equal load steps, each started from the last.  Returns (u, iterations per increment)."""
    u, its = None, []
    for k in range(1, n_inc + 1):
        u, it, ok = newton(nodes, el, loads, fixed, ea, dim, lam=k / n_inc, u0=u, **kw)
        assert ok, f"reference Newton did not converge in increment {k}"
        its.append(it)
    return u, its


# ---- what the identification is built from: sensitivities, right-hand sides, B = d e / d u ------------------------------
def element_sensitivity(nodes, el, u, a, dim, e0=None):
    """-((e - e0) / l0) d.(a_j - a_i) per element (d f_int / d ea_e = fe_e / ea_e, which does not contain ea)."""
    strain, _, _, t = element_state(nodes, el, u, 1.0, dim, e0)
    A = np.asarray(a, dtype=np.float64).reshape(-1, dim)
    el = np.asarray(el, dtype=np.int64)
    return -((strain - t["e0"]) / t["l0"]) * np.sum(t["d"] * (A[el[:, 1]] - A[el[:, 0]]), axis=1)


def sensitivity_scale(nodes, el, u, a, dim, e0=None):
    """The magnitude of the terms element_sensitivity is summed from, in front of any cancellation (of e - e0 as well):
    ((e_abs + |e0|) / l0) sum_c |d_c| (|a_j,c| + |a_i,c|)."""
    t = element_state(nodes, el, u, 1.0, dim, e0)[3]
    A = np.abs(np.asarray(a, dtype=np.float64).reshape(-1, dim))
    el = np.asarray(el, dtype=np.int64)
    return ((t["e_abs"] + np.abs(t["e0"])) / t["l0"]) * np.sum(np.abs(t["d"]) * (A[el[:, 1]] + A[el[:, 0]]), axis=1)


def group_rhs(nodes, el, u, ea, dim, groups, n_groups, fixed, e0=None):
    """[G, n_dofs]: minus the internal force of the elements of every group alone, zero on the fixed dofs."""
    ea = np.broadcast_to(np.asarray(ea, dtype=np.float64), (len(el),))
    groups = np.asarray(groups, dtype=int)
    out = np.stack([-f_int(nodes, el, u, np.where(groups == g, ea, 0.0), dim, e0=e0) for g in range(n_groups)])
    out[:, np.asarray(fixed, dtype=int)] = 0.0
    return out


def _abs_d(nodes, el, u, dim):
    """|d0_c| + |u_j,c| + |u_i,c| per element and component: the magnitude d = d0 + (u_j - u_i) is summed from."""
    t = element_state(nodes, el, u, 1.0, dim)[3]
    U = np.abs(np.asarray(u, dtype=np.float64).reshape(-1, dim))
    el = np.asarray(el, dtype=np.int64)
    return np.abs(t["d0"]) + U[el[:, 1]] + U[el[:, 0]], t


def _group_rows(nodes, el, dim, term, pgroups, n_t, sign):
    """[n_t, n_dofs]: row h is _scatter over the elements of group h alone."""
    el, n_nodes = np.asarray(el, dtype=np.int64), len(_as2d(nodes, dim))
    picks = [np.flatnonzero(np.asarray(pgroups) == h) for h in range(n_t)]
    return np.stack([_scatter(n_nodes, dim, el[pick], term[pick], sign) for pick in picks])


def prestress_rhs(nodes, el, u, ea, pgroups, n_t, dim):
    """[n_t, n_dofs], every row (fixed dofs included): with e0_e = base_e + t_h(e) and d fe / d e0 = -(ea / l0) d, row h =
    -d f_int / d t_h = the sum over the elements of group h of +-(ea_e / l0_e) d_e, + at the second node, - at the first."""
    t = element_state(nodes, el, u, ea, dim)[3]
    return _group_rows(nodes, el, dim, (t["ea"] / t["l0"])[:, None] * t["d"], pgroups, n_t, -1.0)


def prestress_rhs_scale(nodes, el, u, ea, pgroups, n_t, dim):
    """Per row and dof, the sum over the node's elements of group h of (|ea_e| / l0_e) (|d0_c| + |u_j,c| + |u_i,c|): the
    magnitude of the terms prestress_rhs is summed from, in front of any cancellation (in d as well)."""
    mag_d, t = _abs_d(nodes, el, u, dim)
    ea = np.abs(np.broadcast_to(np.asarray(ea, dtype=np.float64), t["l0"].shape))
    return _group_rows(nodes, el, dim, (ea / t["l0"])[:, None] * mag_d, pgroups, n_t, 1.0)


def strains(nodes, el, u, dim):
    return element_state(nodes, el, u, 1.0, dim)[0]


def bt_c(nodes, el, u, c, dim):
    """B^T c [n_dofs] with B = d e / d u (d e_e / d u_j = +d / l0^2, d e_e / d u_i = -d / l0^2): +(c_e / l0^2) d_e at the
    element's second node, - at its first, every row (fixed dofs included)."""
    t = element_state(nodes, el, u, 1.0, dim)[3]
    term = (np.asarray(c, dtype=np.float64) / t["l02"])[:, None] * t["d"]
    return _scatter(len(_as2d(nodes, dim)), dim, np.asarray(el, dtype=np.int64), term, -1.0)


def bt_c_scale(nodes, el, u, c, dim):
    """Per dof, the sum over the node's elements of (|c_e| / l0^2) (|d0_c| + |u_j,c| + |u_i,c|): the magnitude of the terms
    bt_c is summed from, in front of any cancellation (in d as well)."""
    mag_d, t = _abs_d(nodes, el, u, dim)
    term = (np.abs(np.asarray(c, dtype=np.float64)) / t["l02"])[:, None] * mag_d
    return _scatter(len(_as2d(nodes, dim)), dim, np.asarray(el, dtype=np.int64), term, 1.0)


def b_v(nodes, el, u, elements, v, dim):
    """(B v)[i] = (d_e / l0^2).(v_j - v_i) for e = elements[i]."""
    t = element_state(nodes, el, u, 1.0, dim)[3]
    V = np.asarray(v, dtype=np.float64).reshape(-1, dim)
    pick = np.asarray(elements, dtype=int)
    el = np.asarray(el, dtype=np.int64)[pick]
    return np.sum(t["d"][pick] * (V[el[:, 1]] - V[el[:, 0]]), axis=1) / t["l02"][pick]


def b_v_scale(nodes, el, u, elements, v, dim):
    """sum_c (|d0_c| + |u_j,c| + |u_i,c|) (|v_j,c| + |v_i,c|) / l0^2 per gauge: b_v's terms in front of any cancellation."""
    mag_d, t = _abs_d(nodes, el, u, dim)
    V = np.abs(np.asarray(v, dtype=np.float64).reshape(-1, dim))
    pick = np.asarray(elements, dtype=int)
    el = np.asarray(el, dtype=np.int64)[pick]
    return np.sum(mag_d[pick] * (V[el[:, 1]] + V[el[:, 0]]), axis=1) / t["l02"][pick]


# ---- closed forms ---------------------------------------------------------------------------------------------------
class TwoBar:
    """Supports at (-a, 0) and (a, 0), apex at (0, h), both bars E*A = ea, load P downward at the apex.  With the apex
    drop w:  e = (w^2 - 2 h w) / (2 l0^2),  P(w) = ea (2 h w - w^2)(h - w) / l0^3,  limit point at w = h (1 - 1/sqrt 3)."""

    def __init__(self, a=10.0, h=1.0, ea=1000.0):
        self.a, self.h, self.ea = float(a), float(h), float(ea)
        self.l0 = float(np.hypot(a, h))
        self.nodes = np.array([[-a, 0.0], [a, 0.0], [0.0, h]])
        self.el = np.array([[0, 2], [1, 2]])
        self.fixed = np.array([0, 1, 2, 3])
        self.w_lim = h * (1.0 - 1.0 / np.sqrt(3.0))
        self.p_lim = self.load(self.w_lim)

    def load(self, w):
        return self.ea * (2.0 * self.h * w - w * w) * (self.h - w) / self.l0 ** 3

    def strain(self, w):
        return (w * w - 2.0 * self.h * w) / (2.0 * self.l0 ** 2)

    def tangent(self, w):
        """dP/dw: the vertical tangent stiffness at the apex."""
        return self.ea * (2.0 * self.h * self.h - 6.0 * self.h * w + 3.0 * w * w) / self.l0 ** 3

    def loads(self, p):
        out = np.zeros(6)
        out[5] = -p
        return out

    def linear_drop(self, p):
        """Small-displacement answer: w = P l0^3 / (2 ea h^2)."""
        return p * self.l0 ** 3 / (2.0 * self.ea * self.h ** 2)


def bar_1d_load(ea, l0, u):
    """One bar of length l0 fixed at one end, end displacement u: f = ea e (l0 + u) / l0, e = (2 l0 u + u^2) / (2 l0^2)."""
    e = (2.0 * l0 * u + u * u) / (2.0 * l0 * l0)
    return ea * e * (l0 + u) / l0


# ---- meshes ---------------------------------------------------------------------------------------------------------
def cantilever_warren(n_panels, h=1.0, height=1.0):
    """Warren girder clamped at its left end (bottom node 0 and top node 0 pinned), tip load downward at the last
    bottom node.  Returns (nodes, el, loads for a unit tip load, fixed, tip dof)."""
    n = int(n_panels)
    nodes = np.zeros((2 * n + 1, 2))
    nodes[0::2, 0] = np.arange(n + 1) * h
    nodes[1::2, 0] = (np.arange(n) + 0.5) * h
    nodes[1::2, 1] = height
    el = []
    for i in range(n):
        el += [(2 * i, 2 * i + 2), (2 * i, 2 * i + 1), (2 * i + 1, 2 * i + 2)]
        if i + 1 < n:
            el.append((2 * i + 1, 2 * i + 3))
    loads = np.zeros(2 * len(nodes))
    tip = 2 * (2 * n) + 1
    loads[tip] = -1.0
    return nodes, np.array(el), loads, np.array([0, 1, 2, 3]), tip


def irregular_truss(n_elems, rng, hub_degree=6):
    """Planar truss with exactly n_elems elements: jittered-grid nodes in shuffled numbering, neighbour elements in
    shuffled order and random orientation, plus a hub node of degree >= hub_degree when the count allows."""
    if n_elems == 1:
        return np.array([[0.3, -0.2], [1.1, 0.5]]), np.array([[1, 0]])
    side = max(3, int(np.ceil(np.sqrt(n_elems / 3.0))) + 1)
    ij = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2)
    nodes = ij + rng.uniform(-0.3, 0.3, ij.shape)
    idx = {tuple(p): k for k, p in enumerate(ij)}
    cand = []
    for k, (i, j) in enumerate(ij):
        for di, dj in ((1, 0), (0, 1), (1, 1), (1, -1)):
            q = idx.get((i + di, j + dj))
            if q is not None:
                cand.append((k, q))
    hub = [(0, int(q)) for q in rng.choice(np.arange(side + 2, len(ij)), size=hub_degree, replace=False)]
    hub = [p for p in hub if p not in cand]
    rng.shuffle(cand)
    el = np.array((hub + cand)[:n_elems])
    assert len(el) == n_elems
    used = np.unique(el)                                  # drop unused nodes, shuffle the numbering
    perm = rng.permutation(len(used))
    new_id = np.full(len(ij), -1)
    new_id[used] = perm
    out_nodes = np.empty((len(used), 2))
    out_nodes[perm] = nodes[used]
    el = new_id[el]
    rng.shuffle(el)
    flip = rng.random(len(el)) < 0.5
    el[flip] = el[flip][:, ::-1]
    return out_nodes, el


def f_int_exact(nodes, el, u, ea, dim):
    """f_int of the float64 data as given (d0 = fl(X_j - X_i) as the kernels receive it, u as it is), in rational
    arithmetic up to the last step: every term E A e d_c is an exact Fraction, rounded once, divided by l0 (two more
    roundings) and the terms of a dof added with math.fsum.  Its error is 3 * 2^-53 of each term's own (not its
    parts') magnitude: where the parts cancel it stays exact to that."""
    import math
    from fractions import Fraction
    X, U = _as2d(nodes, dim), np.asarray(u, dtype=np.float64).reshape(-1, dim)
    terms = [[[] for _ in range(dim)] for _ in range(len(X))]
    ea = np.broadcast_to(np.asarray(ea, dtype=np.float64), (len(el),))
    for k, (i, j) in enumerate(np.asarray(el, dtype=np.int64)):
        d0 = [Fraction(float(X[j, c] - X[i, c])) for c in range(dim)]
        du = [Fraction(float(U[j, c])) - Fraction(float(U[i, c])) for c in range(dim)]
        l02 = sum(a * a for a in d0)
        e = (2 * sum(a * b for a, b in zip(d0, du)) + sum(b * b for b in du)) / (2 * l02)
        l0 = math.sqrt(float(l02))
        for c in range(dim):
            t = float(Fraction(float(ea[k])) * e * (d0[c] + du[c])) / l0
            terms[j][c].append(t)
            terms[i][c].append(-t)
    return np.array([[math.fsum(t) for t in row] for row in terms]).reshape(-1)


def rigid_motion(nodes, angle, shift):
    """u of a rotation by `angle` about the origin plus a translation (2-D), rounded to float64: each component carries
    the roundings of two products and three sums, up to 4 * 2^-53 (|X_x| + |X_y| + |shift_c|) (rigid_motion_rounding),
    so the field is rigid only to that."""
    X = _as2d(nodes, 2)
    c, s = np.cos(angle), np.sin(angle)
    R = np.array([[c, -s], [s, c]])
    return (X @ R.T + np.asarray(shift) - X).reshape(-1)


def quarter_turn(nodes, shift):
    """u of a rotation by 90 degrees about the origin plus a translation.  With coordinates on a 2^-20 grid and a dyadic
    shift every operation here and in the element's strain is exact in float64: an exactly rigid field."""
    X = _as2d(nodes, 2)
    return (np.stack([-X[:, 1], X[:, 0]], axis=1) + np.asarray(shift, dtype=np.float64) - X).reshape(-1)


def rigid_motion_rounding(nodes, shift):
    """Bound of what rounding leaves of rigid_motion's field, per dof."""
    X = _as2d(nodes, 2)
    return (4.0 * 2.0 ** -53 * (np.abs(X).sum(axis=1)[:, None] + np.abs(np.asarray(shift, dtype=np.float64))[None, :])).reshape(-1)
