"""Identification of element stiffness through the Green-Lagrange Newton solve in numpy / scipy float64, on top of
tests/gl_reference.py: the displacement misfit over several load levels, its gradient with respect to every element's
E*A by one adjoint solve per level, the group reduction, and the L-BFGS loop on log-factors.  Sparse direct solves by
default; it shares no code with the kernels or with pinn_fem_amd/fem/identify.py.

  J = sum_k mean_{m in m_k} (u_k[m] - ubar_k[m])^2,      f_int(u_k; ea) = lam_k f on the free dofs
  K_t(u_k) a_k = g_k,   g_k[m] = 2 (u_k[m] - ubar_k[m]) / |m_k|
  dJ/d ea_e = - sum_k (e / l0) d.(a_j - a_i)             (d f_int / d ea_e = fe_e / ea_e, which does not contain ea)
  ea_e = ea0 exp(q_group(e)),   dJ/dq_g = sum_{e in g} ea_e dJ/d ea_e
"""
import functools
import math
from dataclasses import dataclass

import numpy as np
import scipy.sparse.linalg as spla

import gl_reference as gl

TRUE_FACTORS = (1.0, 0.7, 1.3, 0.85)
LOAD_FACTORS = (1.0 / 3.0, 2.0 / 3.0, 1.0)
LBFGS = dict(lr=1, max_iter=60, history_size=10, line_search_fn="strong_wolfe", tolerance_grad=1e-14, tolerance_change=1e-18)


def element_sensitivity(nodes, el, u, a, dim):
    """-(e / l0) d.(a_j - a_i) per element."""
    strain, _, _, t = gl.element_state(nodes, el, u, 1.0, dim)
    A = np.asarray(a, dtype=np.float64).reshape(-1, dim)
    el = np.asarray(el, dtype=np.int64)
    da = A[el[:, 1]] - A[el[:, 0]]
    return -(strain / t["l0"]) * np.sum(t["d"] * da, axis=1)


def sensitivity_scale(nodes, el, u, a, dim):
    """The magnitude of the terms element_sensitivity is summed from, in front of any cancellation:
    (e_abs / l0) sum_c |d_c| (|a_j,c| + |a_i,c|) with e_abs = (2 |d0|.|du| + |du|.|du|) / (2 l0^2)."""
    t = gl.element_state(nodes, el, u, 1.0, dim)[3]
    A = np.abs(np.asarray(a, dtype=np.float64).reshape(-1, dim))
    el = np.asarray(el, dtype=np.int64)
    e_abs = (2.0 * np.sum(np.abs(t["d0"]) * np.abs(t["du"]), axis=1) + np.sum(t["du"] ** 2, axis=1)) / (2.0 * t["l02"])
    return (e_abs / t["l0"]) * np.sum(np.abs(t["d"]) * (A[el[:, 1]] + A[el[:, 0]]), axis=1)


def misfit_and_gradient(nodes, el, loads, fixed, ea, dim, levels, tol=1e-10, linear_solve=spla.spsolve):
    """levels: [(load factor, measured dofs, measured values)], taken in ascending order of load factor, each Newton
    solve started from the last.  Returns (J, dJ/d ea [ne], displacements per level in that order, Newton iterations)."""
    n = len(np.asarray(nodes, dtype=float).reshape(-1, dim)) * dim
    free = gl.free_mask(n, fixed)
    idx = np.flatnonzero(free)
    J, grad, us, its, u = 0.0, np.zeros(len(el)), [], [], None
    for lam, dofs, ubar in sorted(levels, key=lambda lv: lv[0]):
        u, it, ok = gl.newton(nodes, el, loads, fixed, ea, dim, lam=lam, u0=u, tol=tol, linear_solve=linear_solve)
        assert ok, f"reference Newton did not converge at load factor {lam}"
        dofs, ubar = np.asarray(dofs, dtype=int), np.asarray(ubar, dtype=np.float64)
        r = u[dofs] - ubar
        J += float(np.mean(r * r))
        g = np.zeros(n)
        np.add.at(g, dofs, 2.0 * r / len(dofs))
        a = np.zeros(n)
        a[idx] = linear_solve(gl.restrict(gl.k_t(nodes, el, u, ea, dim), free), g[idx])
        grad += element_sensitivity(nodes, el, u, a, dim)
        us.append(u)
        its.append(it)
    return J, grad, us, its


def group_reduce(values, weights, groups, n_groups):
    """out[g] = fsum of values[e] * weights[e] over the elements of group g."""
    v = np.asarray(values, dtype=np.float64) * (1.0 if weights is None else np.asarray(weights, dtype=np.float64))
    groups = np.asarray(groups, dtype=int)
    return np.array([math.fsum(v[groups == g]) for g in range(n_groups)])


# ---- the two-bar closed form -----------------------------------------------------------------------------------------
def two_bar_closed_form(tb, p, w, w_bar):
    """dJ/d(ea) of J = (w - w_bar)^2 at fixed load P with both bars at ea: P = ea phi(w), so
    dw/d(ea) = -phi / (ea phi') = -P / (ea * tangent(w))."""
    return 2.0 * (w - w_bar) * (-p / (tb.ea * tb.tangent(w)))


def two_bar_bound(tb, w, w_bar, tol):
    """Relative bound of the closed form evaluated at a Newton iterate: the loop stops at |du| <= tol |u|, so w is off
    by at most tol * w, which enters (w - w_bar) and tangent(w): tol w (1 / |w - w_bar| + |tangent'| / |tangent|), and as
    much again for the adjoint gradient, which is formed at the same iterate; plus 1e-12 for the round-off of both."""
    d_tangent = tb.ea * (6.0 * w - 6.0 * tb.h) / tb.l0 ** 3
    return 2.0 * tol * w * (1.0 / abs(w - w_bar) + abs(d_tangent / tb.tangent(w))) + 1e-12


@dataclass
class Case:
    nodes: np.ndarray
    el: np.ndarray
    loads: np.ndarray          # at load factor 1
    fixed: np.ndarray
    tip: int
    ea0: float
    groups: np.ndarray         # [ne] group of every element
    factors: np.ndarray        # the true factor of every group
    levels: list               # [(load factor, dofs, measured values)]

    @property
    def n_groups(self):
        return len(self.factors)

    def ea(self, q):
        return self.ea0 * np.exp(np.asarray(q, dtype=np.float64))[self.groups]

    def objective(self, q, **kw):
        """(J, dJ/dq) at the log-factors q."""
        ea = self.ea(q)
        J, g_ea, _, _ = misfit_and_gradient(self.nodes, self.el, self.loads, self.fixed, ea, 2, self.levels, **kw)
        return J, group_reduce(g_ea, ea, self.groups, self.n_groups)


def span_groups(nodes, el, n_groups):
    """Group of every element by the part of the span its centre x lies in (equal parts)."""
    X = np.asarray(nodes, dtype=float).reshape(-1, 2)
    xc = 0.5 * (X[el[:, 0], 0] + X[el[:, 1], 0])
    span = X[:, 0].max() - X[:, 0].min()
    return np.minimum((n_groups * (xc - X[:, 0].min()) / span).astype(int), n_groups - 1)


def warren_case(n_panels, factors=TRUE_FACTORS, load_factors=LOAD_FACTORS, ea0=1000.0, deflection=0.15):
    """cantilever_warren(n_panels) with the tip load at which the LINEAR tip deflection is `deflection` of the span,
    groups by equal parts of the span, and every free dof measured at every load level on the structure with the true
    factors (synthetic measurements from the restatement's own Newton solve)."""
    nodes, el, unit, fixed, tip = gl.cantilever_warren(n_panels)
    free = gl.free_mask(len(unit), fixed)
    idx = np.flatnonzero(free)
    u_lin = np.zeros(len(unit))
    u_lin[idx] = spla.spsolve(gl.restrict(gl.k_t(nodes, el, np.zeros(len(unit)), ea0, 2), free), unit[idx])
    loads = unit * (deflection * float(n_panels) / abs(u_lin[tip]))
    factors = np.asarray(factors, dtype=np.float64)
    groups = span_groups(nodes, el, len(factors))
    ea_true = ea0 * factors[groups]
    levels, u = [], None
    for lam in load_factors:
        u, _, ok = gl.newton(nodes, el, loads, fixed, ea_true, 2, lam=lam, u0=u, tol=1e-12)
        assert ok
        levels.append((float(lam), idx.copy(), u[idx].copy()))
    return Case(nodes, el, loads, fixed, tip, float(ea0), groups, factors, levels)


def recover(case, q0=None, **kw):
    """torch.optim.LBFGS (strong Wolfe) on the log-factors from q0 (zeros: all factors 1).
    Returns (factors, misfit evaluations, J at the last evaluation)."""
    import torch
    q = torch.zeros(case.n_groups, dtype=torch.float64) if q0 is None else torch.as_tensor(q0, dtype=torch.float64).clone()
    q.requires_grad_(True)
    opt = torch.optim.LBFGS([q], **LBFGS)
    seen = []

    def closure():
        opt.zero_grad()
        J, g = case.objective(q.detach().numpy(), **kw)
        q.grad = torch.from_numpy(g.copy())
        seen.append(J)
        return torch.tensor(J, dtype=torch.float64)
    opt.step(closure)
    return np.exp(q.detach().numpy()), len(seen), seen[-1]


@functools.lru_cache(maxsize=None)
def reference_recovery(n_panels):
    """(case, factors, evaluations) of recover() on warren_case(n_panels) from all factors 1: computed once, shared by
    the tests that hold the device optimisation to the reference's evaluation count."""
    case = warren_case(n_panels)
    factors, evaluations, _ = recover(case)
    return case, factors, evaluations
