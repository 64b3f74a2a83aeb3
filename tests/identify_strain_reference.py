"""Identification of E*A factors from strain-gauge data in numpy / scipy float64, on top of tests/gl_reference.py,
tests/identify_reference.py and tests/identify_gn_reference.py: the strain residuals, the derivative B = d e / d u of the
Green-Lagrange strains applied to vectors and its transpose applied to per-element coefficients (with the magnitude sums
the round-off bounds of the GPU tests are stated in), the misfit with its adjoint gradient, the weighted residuals with
their Jacobian, and the Levenberg-Marquardt loop, all with levels that carry gauges.  Sparse direct solves by default; it
shares no code with the kernels or with pinn_fem_amd/fem/identify.py.

  e_e = (2 d0.du + du.du) / (2 l0^2),  d = d0 + du            d e_e / d u_j = +d / l0^2,  d e_e / d u_i = -d / l0^2
  J   = sum_k [ mean_m (u_k[m] - ubar_k[m])^2 + L_k^2 mean_i (e_k[elem_i] - ebar_ki)^2 ]
  rho = per level (u_k[m_k] - ubar_k) / sqrt|m_k|, then L_k (e - ebar) / sqrt p_k;   J = rho.rho
  g_k = 2 r_k / |m_k| at m_k  +  B^T c,  c_e = 2 L_k^2 (e_e - ebar_e) / p_k on the gauges;   K_t a_k = g_k
  A   = per level s_kg[m_k] / sqrt|m_k|, then (L_k / sqrt p_k) B s_kg at the gauges
"""
import functools
from dataclasses import dataclass, field

import numpy as np
import scipy.sparse.linalg as spla

import gl_reference as gl
import identify_gn_reference as gn
import identify_reference as ir

STRAIN_SCALE = 8.0                   # the span of warren_case(8)


# ---- B = d e / d u ---------------------------------------------------------------------------------------------------
def strains(nodes, el, u, dim):
    return gl.element_state(nodes, el, u, 1.0, dim)[0]


def _abs_d(nodes, el, u, dim):
    """|d0_c| + |u_j,c| + |u_i,c| per element and component: the magnitude d = d0 + (u_j - u_i) is summed from."""
    t = gl.element_state(nodes, el, u, 1.0, dim)[3]
    U = np.abs(np.asarray(u, dtype=np.float64).reshape(-1, dim))
    el = np.asarray(el, dtype=np.int64)
    return np.abs(t["d0"]) + U[el[:, 1]] + U[el[:, 0]], t


def bt_c(nodes, el, u, c, dim):
    """B^T c [n_dofs]: +(c_e / l0^2) d_e at the element's second node, - at its first, every row (fixed dofs included)."""
    t = gl.element_state(nodes, el, u, 1.0, dim)[3]
    el = np.asarray(el, dtype=np.int64)
    term = (np.asarray(c, dtype=np.float64) / t["l02"])[:, None] * t["d"]
    out = np.zeros((len(np.asarray(nodes, dtype=float).reshape(-1, dim)), dim))
    np.add.at(out, el[:, 1], term)
    np.add.at(out, el[:, 0], -term)
    return out.reshape(-1)


def bt_c_scale(nodes, el, u, c, dim):
    """Per dof, the sum over the node's elements of (|c_e| / l0^2) (|d0_c| + |u_j,c| + |u_i,c|): the magnitude of the terms
    bt_c is summed from, in front of any cancellation (in d as well)."""
    mag_d, t = _abs_d(nodes, el, u, dim)
    el = np.asarray(el, dtype=np.int64)
    term = (np.abs(np.asarray(c, dtype=np.float64)) / t["l02"])[:, None] * mag_d
    out = np.zeros((len(np.asarray(nodes, dtype=float).reshape(-1, dim)), dim))
    np.add.at(out, el[:, 1], term)
    np.add.at(out, el[:, 0], term)
    return out.reshape(-1)


def b_v(nodes, el, u, elements, v, dim):
    """(B v)[i] = (d_e / l0^2).(v_j - v_i) for e = elements[i]."""
    t = gl.element_state(nodes, el, u, 1.0, dim)[3]
    V = np.asarray(v, dtype=np.float64).reshape(-1, dim)
    el = np.asarray(el, dtype=np.int64)[np.asarray(elements, dtype=int)]
    pick = np.asarray(elements, dtype=int)
    return np.sum(t["d"][pick] * (V[el[:, 1]] - V[el[:, 0]]), axis=1) / t["l02"][pick]


def b_v_scale(nodes, el, u, elements, v, dim):
    """sum_c (|d0_c| + |u_j,c| + |u_i,c|) (|v_j,c| + |v_i,c|) / l0^2 per gauge: b_v's terms in front of any cancellation."""
    mag_d, t = _abs_d(nodes, el, u, dim)
    V = np.abs(np.asarray(v, dtype=np.float64).reshape(-1, dim))
    pick = np.asarray(elements, dtype=int)
    el = np.asarray(el, dtype=np.int64)[pick]
    return np.sum(mag_d[pick] * (V[el[:, 1]] + V[el[:, 0]]), axis=1) / t["l02"][pick]


# ---- misfit, adjoint gradient, residuals, Jacobian -----------------------------------------------------------------------
def strain_residuals(nodes, el, u, gauge, dim):
    """(e[elements] - ebar, L, p) of one level's gauges (elements, values, scale)."""
    elements, values, scale = gauge
    elements = np.asarray(elements, dtype=int)
    return strains(nodes, el, u, dim)[elements] - np.asarray(values, dtype=np.float64), float(scale), len(elements)


def misfit_and_gradient(nodes, el, loads, fixed, ea, dim, levels, gauges, tol=1e-10, linear_solve=spla.spsolve):
    """levels: [(load factor, dofs, values)] in ascending load factor (dofs may be empty); gauges: per level None or
    (elements, strains, scale).  Returns (J, dJ/d ea [ne], displacements per level, Newton iterations per level)."""
    assert all(a[0] <= b[0] for a, b in zip(levels, levels[1:]))
    n = len(np.asarray(nodes, dtype=float).reshape(-1, dim)) * dim
    free = gl.free_mask(n, fixed)
    idx = np.flatnonzero(free)
    J, grad, us, its, u = 0.0, np.zeros(len(el)), [], [], None
    for (lam, dofs, ubar), gauge in zip(levels, gauges):
        u, it, ok = gl.newton(nodes, el, loads, fixed, ea, dim, lam=lam, u0=u, tol=tol, linear_solve=linear_solve)
        assert ok, f"reference Newton did not converge at load factor {lam}"
        dofs, ubar = np.asarray(dofs, dtype=int), np.asarray(ubar, dtype=np.float64)
        g = np.zeros(n)
        if len(dofs):
            r = u[dofs] - ubar
            J += float(np.mean(r * r))
            np.add.at(g, dofs, 2.0 * r / len(dofs))
        if gauge is not None:
            r_e, scale, p = strain_residuals(nodes, el, u, gauge, dim)
            J += scale * scale * float(np.mean(r_e * r_e))
            c = np.zeros(len(el))
            c[np.asarray(gauge[0], dtype=int)] = 2.0 * scale * scale * r_e / p
            g += np.where(free, bt_c(nodes, el, u, c, dim), 0.0)
        a = np.zeros(n)
        a[idx] = linear_solve(gl.restrict(gl.k_t(nodes, el, u, ea, dim), free), g[idx])
        grad += ir.element_sensitivity(nodes, el, u, a, dim)
        us.append(u)
        its.append(it)
    return J, grad, us, its


@dataclass
class StrainCase(ir.Case):
    """identify_reference.Case whose levels (ascending load factor) carry gauges: gauges[k] = (elements, strains, scale) or
    None beside levels[k] = (load factor, dofs, values), dofs possibly empty."""
    gauges: list = field(default_factory=list)

    def objective(self, q, **kw):
        """(J, dJ/dq) at the log-factors q."""
        ea = self.ea(q)
        J, g_ea, _, _ = misfit_and_gradient(self.nodes, self.el, self.loads, self.fixed, ea, 2, self.levels, self.gauges, **kw)
        return J, ir.group_reduce(g_ea, ea, self.groups, self.n_groups)

    def dict_levels(self):
        """The levels as identify_nr takes them."""
        out = []
        for (lam, dofs, ubar), gauge in zip(self.levels, self.gauges):
            lv = {"load_factor": lam, "dofs": np.asarray(dofs, dtype=np.int64), "u": np.asarray(ubar, dtype=np.float64)}
            if gauge is not None:
                lv.update(strain_elements=np.asarray(gauge[0], dtype=np.int64), strains=np.asarray(gauge[1]),
                          strain_scale=gauge[2])
            out.append(lv)
        return out

    @property
    def n_rows(self):
        return sum(len(lv[1]) for lv in self.levels) + sum(len(g[0]) for g in self.gauges if g is not None)


def residuals_and_jacobian(case, q, states=None, jacobian=True, tol=1e-10, linear_solve=spla.spsolve):
    """identify_gn_reference.residuals_and_jacobian with the gauges' rows behind every level's displacement rows:
    (rho [M], A [M, G] or None, displacements per level, Newton iterations per level)."""
    nodes, el, dim = case.nodes, case.el, 2
    ea = case.ea(q)
    n = len(case.loads)
    free = gl.free_mask(n, case.fixed)
    idx = np.flatnonzero(free)
    rho, rows, us, its, u = [], [], [], [], None
    for k, ((lam, dofs, ubar), gauge) in enumerate(zip(case.levels, case.gauges)):
        if states is None:
            u, it, ok = gl.newton(nodes, el, case.loads, case.fixed, ea, dim, lam=lam, u0=u, tol=tol, linear_solve=linear_solve)
            assert ok, f"reference Newton did not converge at load factor {lam}"
            its.append(it)
        else:
            u = np.asarray(states[k], dtype=np.float64)
        dofs, ubar = np.asarray(dofs, dtype=int), np.asarray(ubar, dtype=np.float64)
        if len(dofs):
            rho.append((u[dofs] - ubar) / np.sqrt(len(dofs)))
        if gauge is not None:
            r_e, scale, p = strain_residuals(nodes, el, u, gauge, dim)
            rho.append(scale * r_e / np.sqrt(p))
        if jacobian:
            Kff = gl.restrict(gl.k_t(nodes, el, u, ea, dim), free)
            B = gn.group_rhs(nodes, el, u, ea, dim, case.groups, case.n_groups, case.fixed)
            S = np.zeros_like(B)
            for g in range(case.n_groups):
                S[g, idx] = linear_solve(Kff, B[g, idx])
            if len(dofs):
                rows.append(S[:, dofs].T / np.sqrt(len(dofs)))
            if gauge is not None:
                rows.append(np.stack([b_v(nodes, el, u, gauge[0], S[g], dim) for g in range(case.n_groups)], axis=1)
                            * (scale / np.sqrt(p)))
        us.append(u)
    return np.concatenate(rho), (np.concatenate(rows, axis=0) if jacobian else None), us, its


def levenberg_marquardt(case, q0=None, max_evaluations=200, gtol=1e-12, misfit_tolerance=0.0, damping=1e-3,
                        step_tolerance=1e-12, **kw):
    """The loop of identify_nr(method="gauss-newton") on this module's residuals_and_jacobian.  Returns a dict: q, factors,
    misfit, rho, jacobian, states, evaluations, stop, history ([{misfit, accepted, damping}] per evaluation)."""
    q = np.zeros(case.n_groups) if q0 is None else np.asarray(q0, dtype=np.float64).copy()
    rho, A, states, _ = residuals_and_jacobian(case, q, **kw)
    J, mu, evaluations = float(rho @ rho), float(damping), 1
    history = [dict(misfit=J, accepted=True, damping=mu)]
    while True:
        if J <= misfit_tolerance:
            stop = "misfit"
            break
        if np.max(np.abs(2.0 * A.T @ rho)) <= gtol:
            stop = "gradient"
            break
        if evaluations >= max_evaluations:
            stop = "cap"
            break
        H = A.T @ A
        delta = np.linalg.solve(H + mu * np.diag(np.diag(H)), -(A.T @ rho))
        if np.max(np.abs(delta)) <= step_tolerance:
            stop = "step"
            break
        rho_t, _, states_t, _ = residuals_and_jacobian(case, q + delta, jacobian=False, **kw)
        evaluations += 1
        J_t = float(rho_t @ rho_t)
        history.append(dict(misfit=J_t, accepted=J_t < J, damping=mu))
        if J_t < J:
            q, rho, J, states = q + delta, rho_t, J_t, states_t
            A = residuals_and_jacobian(case, q, states=states, **kw)[1]
            mu = max(mu / 10.0, 1e-12)
        else:
            mu *= 10.0
            if mu > 1e12:
                stop = "damping"
                break
    return dict(q=q, factors=np.exp(q), misfit=J, rho=rho, jacobian=A, states=states, evaluations=evaluations, stop=stop,
                history=history)


# ---- cases -------------------------------------------------------------------------------------------------------------
def gauge_elements(groups, n_groups, per_group=1):
    """The per_group lowest-numbered elements of every group, in group order."""
    groups = np.asarray(groups, dtype=int)
    return np.concatenate([np.flatnonzero(groups == g)[:per_group] for g in range(n_groups)])


@functools.lru_cache(maxsize=None)
def strain_case(n_groups, gauges_per_group=1, tip=False):
    """case_with_groups(n_groups) measured by strain gauges: at every load level the Green-Lagrange strains of the
    gauges_per_group lowest-numbered elements of every span group, on the structure with the true factors (its states are the
    base case's measurements of every free dof), with strain scale 8.0 (the span); tip: the tip dof as the one displacement
    row of every level, otherwise no displacement data."""
    base = gn.case_with_groups(n_groups)
    elements = gauge_elements(base.groups, base.n_groups, gauges_per_group)
    levels, gauges = [], []
    for lam, dofs, ubar in sorted(base.levels, key=lambda lv: lv[0]):
        u = np.zeros(len(base.loads))
        u[dofs] = ubar
        e = strains(base.nodes, base.el, u, 2)
        m = np.array([base.tip]) if tip else np.zeros(0, dtype=int)
        levels.append((lam, m, u[m].copy()))
        gauges.append((elements.copy(), e[elements].copy(), STRAIN_SCALE))
    return StrainCase(base.nodes, base.el, base.loads, base.fixed, base.tip, base.ea0, base.groups, base.factors, levels,
                      gauges)


@functools.lru_cache(maxsize=None)
def reference_run(n_groups, tip=False):
    """(case, levenberg_marquardt(case, misfit_tolerance=1e-15)) from all factors 1: computed once and shared."""
    case = strain_case(n_groups, tip=tip)
    return case, levenberg_marquardt(case, misfit_tolerance=1e-15)


@functools.lru_cache(maxsize=None)
def reference_recovery(tip=False):
    """(case, factors, evaluations) of identify_reference.recover on strain_case(4, tip=tip) from all factors 1."""
    case = strain_case(4, tip=tip)
    factors, evaluations, _ = ir.recover(case)
    return case, factors, evaluations


# ---- the two-bar closed form ---------------------------------------------------------------------------------------------
def two_bar_closed_form(tb, p, w, e_bar, scale):
    """dJ/d(ea) of J = L^2 (e(w) - e_bar)^2 (both bars carry e(w) = (w^2 - 2 h w) / (2 l0^2)) at fixed load P with both
    bars at ea: de/dw = (w - h) / l0^2 and dw/d(ea) = -P / (ea * tangent(w))."""
    return 2.0 * scale * scale * (tb.strain(w) - e_bar) * ((w - tb.h) / tb.l0 ** 2) * (-p / (tb.ea * tb.tangent(w)))


def two_bar_bound(tb, w, e_bar, tol):
    """identify_reference.two_bar_bound's reasoning for the strain misfit: the Newton loop stops at |du| <= tol |u|, so w is
    off by at most tol * w, which enters (e(w) - e_bar) through de/dw, de/dw = (w - h) / l0^2 itself, and tangent(w):
    tol w (|de/dw| / |e - e_bar| + 1 / |w - h| + |tangent'| / |tangent|), as much again for the adjoint gradient, which is
    formed at the same iterate; plus 1e-12 for the round-off of both."""
    d_tangent = tb.ea * (6.0 * w - 6.0 * tb.h) / tb.l0 ** 3
    de_dw = (w - tb.h) / tb.l0 ** 2
    return 2.0 * tol * w * (abs(de_dw) / abs(tb.strain(w) - e_bar) + 1.0 / abs(w - tb.h)
                            + abs(d_tangent / tb.tangent(w))) + 1e-12
