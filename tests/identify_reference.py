"""Identification through the Green-Lagrange Newton solve in numpy / scipy float64, on top of tests/gl_reference.py: the
one evaluation core and the one loop that every kind of identification uses, laid out as pinn_fem_amd/fem/identify.py lays
out the device's.  The misfit over several load levels (displacements, strain gauges, an initial strain in the model) with
its gradient with respect to every element's E*A by one adjoint solve per level, the group reduction and the L-BFGS loop
on log-factors; the weighted residuals with their Jacobian with respect to one log-factor per stiffness group and one
additive initial strain per prestress group, by one sensitivity solve per level and column; the Levenberg-Marquardt loop
with its named entry points.  The feature modules (gl_e0_reference, identify_strain_reference,
identify_prestress_reference) hold their cases and closed forms.  Sparse direct solves by default; it shares no code with
the kernels or with pinn_fem_amd.

  J = sum_k [ mean_{m in m_k} (u_k[m] - ubar_k[m])^2 + L_k^2 mean_i (e_k[elem_i] - ebar_ki)^2 ],   f_int(u_k; ea, e0) = lam_k f
  K_t(u_k) a_k = g_k,   g_k = 2 r_k / |m_k| at m_k  +  B^T c,  c_e = 2 L_k^2 (e_e - ebar_e) / p_k on the gauges
  dJ/d ea_e = - sum_k ((e - e0) / l0) d.(a_j - a_i),   ea_e = ea0 exp(q_group(e)),   dJ/dq_g = sum_{e in g} ea_e dJ/d ea_e
  rho = per level (u_k[m_k] - ubar_k) / sqrt|m_k|, then L_k (e - ebar) / sqrt p_k;   J = rho.rho,   dJ/dx = 2 A^T rho
  K_t(u_k) s_kg = -f_int(u_k; ea restricted to group g),   K_t(u_k) s_kh = -d f_int / d t_h
  A = per level s[m_k] / sqrt|m_k|, then (L_k / sqrt p_k) B s at the gauges;   columns [A_q | A_t]
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


class Refused(RuntimeError):
    """A point the restatement has no misfit at: a slack start, an indefinite tangent or no Newton convergence."""


def _spd_solve(solve):
    def checked(K, b):
        x = solve(K, b)
        if not np.all(np.isfinite(x)) or (np.any(b != 0.0) and not float(b @ x) > 0.0):
            raise Refused("the tangent is not positive definite")
        return x
    return checked


def _ascending(levels, gauges):
    """[(load factor, dofs, values, gauge or None)] in ascending load factor, every gauge beside its level."""
    gauges = [None] * len(levels) if gauges is None else gauges
    both = sorted(zip(levels, gauges), key=lambda lg: lg[0][0])
    return [(lam, np.asarray(dofs, dtype=int), np.asarray(ubar, dtype=np.float64), gauge) for (lam, dofs, ubar), gauge in both]


def _strain_residuals(nodes, el, u, gauge, dim):
    """(e[elements] - ebar, L, p) of one level's gauges (elements, values, scale)."""
    elements, values, scale = gauge
    elements = np.asarray(elements, dtype=int)
    return gl.strains(nodes, el, u, dim)[elements] - np.asarray(values, dtype=np.float64), float(scale), len(elements)


def misfit_and_gradient(nodes, el, loads, fixed, ea, dim, levels, gauges=None, e0=None, tol=1e-10, linear_solve=spla.spsolve):
    """levels: [(load factor, measured dofs, measured values)] (dofs may be empty), taken in ascending order of load factor,
    each Newton solve started from the last; gauges: per level None or (elements, strains, scale); e0: the initial strain.
    Returns (J, dJ/d ea [ne], displacements per level in that order, Newton iterations)."""
    n = len(np.asarray(nodes, dtype=float).reshape(-1, dim)) * dim
    free = gl.free_mask(n, fixed)
    idx = np.flatnonzero(free)
    J, grad, us, its, u = 0.0, np.zeros(len(el)), [], [], None
    for lam, dofs, ubar, gauge in _ascending(levels, gauges):
        u, it, ok = gl.newton(nodes, el, loads, fixed, ea, dim, lam=lam, u0=u, tol=tol, linear_solve=linear_solve, e0=e0)
        assert ok, f"reference Newton did not converge at load factor {lam}"
        g = np.zeros(n)
        if len(dofs):
            r = u[dofs] - ubar
            J += float(np.mean(r * r))
            np.add.at(g, dofs, 2.0 * r / len(dofs))
        if gauge is not None:
            r_e, scale, p = _strain_residuals(nodes, el, u, gauge, dim)
            J += scale * scale * float(np.mean(r_e * r_e))
            c = np.zeros(len(el))
            c[np.asarray(gauge[0], dtype=int)] = 2.0 * scale * scale * r_e / p
            g += np.where(free, gl.bt_c(nodes, el, u, c, dim), 0.0)
        a = np.zeros(n)
        a[idx] = linear_solve(gl.restrict(gl.k_t(nodes, el, u, ea, dim, e0=e0), free), g[idx])
        grad += gl.element_sensitivity(nodes, el, u, a, dim, e0=e0)
        us.append(u)
        its.append(it)
    return J, grad, us, its


def residuals_and_jacobian(nodes, el, loads, fixed, dim, levels, ea, e0=None, gauges=None, groups=None, prestress=None,
                           states=None, jacobian=True, tol=1e-10, linear_solve=spla.spsolve, refuse=False):
    """(rho [M], A [M, G + H] or None, displacements per level in ascending load factor, Newton iterations per level) of
    the structure with ea [ne] and the initial strain e0.  groups, prestress: None or (group of every element, count): the
    columns A_q of one log-factor per stiffness group, then A_t of one additive initial strain per prestress group (-1 in
    its map: none).  A level's gauge rows follow its displacement rows.  states given: those are the u_k, no Newton solves.
    refuse: every solve is held to rhs.x > 0 (the rule the device holds its CG solves to), a diagonal of the starting
    tangent that is not positive on a free dof and a Newton loop that does not converge raise Refused."""
    n = len(np.asarray(loads).reshape(-1))
    free = gl.free_mask(n, fixed)
    idx = np.flatnonzero(free)
    solve = _spd_solve(linear_solve) if refuse else linear_solve
    if refuse and not np.all(gl.k_t(nodes, el, np.zeros(n), ea, dim, e0=e0).diagonal()[idx] > 0.0):
        raise Refused("the tangent at the starting state has a diagonal that is not positive (a slack mechanism)")
    rho, rows, us, its, u = [], [], [], [], None
    for k, (lam, dofs, ubar, gauge) in enumerate(_ascending(levels, gauges)):
        if states is None:
            u, it, ok = gl.newton(nodes, el, loads, fixed, ea, dim, lam=lam, u0=u, tol=tol, linear_solve=solve, e0=e0)
            if refuse and not ok:
                raise Refused(f"Newton did not converge at load factor {lam}")
            assert ok, f"reference Newton did not converge at load factor {lam}"
            its.append(it)
        else:
            u = np.asarray(states[k], dtype=np.float64)
        w = 1.0 / np.sqrt(len(dofs)) if len(dofs) else 0.0
        rho.append((u[dofs] - ubar) * w)
        if gauge is not None:
            r_e, scale, p = _strain_residuals(nodes, el, u, gauge, dim)
            w_e = scale / np.sqrt(p)
            rho.append(r_e * w_e)
        if jacobian:
            B = [gl.group_rhs(nodes, el, u, ea, dim, *groups, fixed, e0=e0)] if groups is not None else []
            if prestress is not None:
                B.append(gl.prestress_rhs(nodes, el, u, ea, *prestress, dim))
            B = np.concatenate(B, axis=0)
            B[:, np.asarray(fixed, dtype=int)] = 0.0
            Kff = gl.restrict(gl.k_t(nodes, el, u, ea, dim, e0=e0), free)
            S = np.zeros_like(B)
            for g in range(len(B)):
                S[g, idx] = solve(Kff, B[g, idx])
            rows.append(S[:, dofs].T * w)
            if gauge is not None:
                rows.append(np.stack([gl.b_v(nodes, el, u, gauge[0], s, dim) for s in S], axis=1) * w_e)
        us.append(u)
    return np.concatenate(rho), (np.concatenate(rows, axis=0) if jacobian else None), us, its


def levenberg_marquardt(evaluate, x0, max_evaluations=200, gtol=1e-12, misfit_tolerance=0.0, damping=1e-3,
                        step_tolerance=1e-12, reject=()):
    """The loop of identify_nr(method="gauss-newton") and identify_prestress, restated.  evaluate(x, states=None,
    jacobian=True) returns (rho, A or None, states).  A trial point whose evaluation raises one of `reject` is a rejected
    step (mu <- 10 mu) that counts as an evaluation; its history entry has misfit None and the message under "error".
    Returns a dict: x, misfit, rho, jacobian, states, evaluations, stop, history ([{misfit, accepted, damping}] per
    evaluation)."""
    x = np.asarray(x0, dtype=np.float64).copy()
    rho, A, states = evaluate(x)
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
        evaluations += 1
        try:
            rho_t, _, states_t = evaluate(x + delta, jacobian=False)
            J_t = float(rho_t @ rho_t)
            history.append(dict(misfit=J_t, accepted=J_t < J, damping=mu))
        except reject as exc:
            J_t = float("inf")
            history.append(dict(misfit=None, accepted=False, damping=mu, error=str(exc)))
        if J_t < J:
            x, rho, J, states = x + delta, rho_t, J_t, states_t
            A = evaluate(x, states=states)[1]
            mu = max(mu / 10.0, 1e-12)
        else:
            mu *= 10.0
            if mu > 1e12:
                stop = "damping"
                break
    return dict(x=x, misfit=J, rho=rho, jacobian=A, states=states, evaluations=evaluations, stop=stop, history=history)


def case_residuals(case, q, e0=None, t=None, **kw):
    """residuals_and_jacobian of a case at the log-factors q: of a Case with the initial strain e0 in the model and the
    case's gauges, if it has any, or (t given) of a PrestressCase at the offsets t, with the refusals."""
    structure = (case.nodes, case.el, case.loads, case.fixed, 2, case.levels, case.ea(q))
    if t is None:
        return residuals_and_jacobian(*structure, e0=e0, gauges=case.gauges, groups=(case.groups, case.n_groups), **kw)
    return residuals_and_jacobian(*structure, e0=case.e0(t), groups=None if case.groups is None else (case.groups, case.n_q),
                                  prestress=(case.pgroups, case.n_t), refuse=True, **kw)


def identify_factors(case, q0=None, e0=None, tol=1e-10, linear_solve=spla.spsolve, **loop):
    """levenberg_marquardt on the log-factors of a Case from q0 (None: all factors 1), with the initial strain e0 in the
    model (None or 0.0: left out) and the case's gauges.  Returns the loop's dict with q and factors in place of x."""
    run = levenberg_marquardt(lambda q, **kw: case_residuals(case, q, e0, tol=tol, linear_solve=linear_solve, **kw)[:3],
                              np.zeros(case.n_groups) if q0 is None else q0, **loop)
    q = run.pop("x")
    return dict(run, q=q, factors=np.exp(q))


def identify_prestress(case, q0=None, t0=None, scale=1e-3, max_evaluations=50, tol=1e-10, linear_solve=spla.spsolve, **loop):
    """levenberg_marquardt on x = (q, t / scale) of a PrestressCase from (q0, t0) (None: all factors 1, the case's start),
    a Refused trial rejected.  Returns the loop's dict with q, t and factors in place of x, the Jacobian in the parameters'
    own units."""
    n_q = case.n_q
    cols = np.concatenate([np.ones(n_q), np.full(case.n_t, scale)])

    def evaluate(x, **kw):
        rho, A, states, _ = case_residuals(case, x[:n_q], t=x[n_q:] * scale, tol=tol, linear_solve=linear_solve, **kw)
        return rho, (None if A is None else A * cols), states

    x0 = np.concatenate([np.zeros(n_q) if q0 is None else q0, (case.t0 if t0 is None else np.asarray(t0)) / scale])
    run = levenberg_marquardt(evaluate, x0, max_evaluations=max_evaluations, reject=(Refused,), **loop)
    x = run.pop("x")
    return dict(run, q=x[:n_q], t=x[n_q:] * scale, factors=np.exp(x[:n_q]), jacobian=run["jacobian"] / cols)


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
    levels: list               # [(load factor, dofs, measured values)], dofs possibly empty
    gauges: list = None        # beside levels: (elements, strains, scale) or None per level
    e0: np.ndarray = None      # [ne] the initial strain the measurements were generated with

    @property
    def n_groups(self):
        return len(self.factors)

    def ea(self, q):
        return self.ea0 * np.exp(np.asarray(q, dtype=np.float64))[self.groups]

    def objective(self, q, e0=None, **kw):
        """(J, dJ/dq) at the log-factors q, with the case's gauges and its initial strain (or the e0 given: 0.0 leaves it
        out)."""
        ea = self.ea(q)
        J, g_ea, _, _ = misfit_and_gradient(self.nodes, self.el, self.loads, self.fixed, ea, 2, self.levels, self.gauges,
                                            self.e0 if e0 is None else e0, **kw)
        return J, group_reduce(g_ea, ea, self.groups, self.n_groups)


def span_groups(nodes, el, n_groups):
    """Group of every element by the part of the span its centre x lies in (equal parts)."""
    X = np.asarray(nodes, dtype=float).reshape(-1, 2)
    xc = 0.5 * (X[el[:, 0], 0] + X[el[:, 1], 0])
    span = X[:, 0].max() - X[:, 0].min()
    return np.minimum((n_groups * (xc - X[:, 0].min()) / span).astype(int), n_groups - 1)


def measure(nodes, el, loads, fixed, ea, load_factors, dofs, e0=None):
    """Synthetic measurements from the restatement's own Newton solve (to 1e-12): [(load factor, dofs, u[dofs])]."""
    levels, u = [], None
    for lam in load_factors:
        u, _, ok = gl.newton(nodes, el, loads, fixed, ea, 2, lam=lam, u0=u, tol=1e-12, e0=e0)
        assert ok
        levels.append((float(lam), dofs.copy(), u[dofs].copy()))
    return levels


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
    levels = measure(nodes, el, loads, fixed, ea0 * factors[groups], load_factors, idx)
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


# ---- the Gauss-Newton cases ------------------------------------------------------------------------------------------
EIGHT_FACTORS = (1.0, 0.7, 1.3, 0.85, 1.1, 0.9, 1.2, 0.8)
NOISE_SIGMA = 1e-4


def covariance(A, J):
    """J / (M - G) (A^T A)^-1: the covariance of the log-factors of the weighted fit."""
    M, G = A.shape
    return J / (M - G) * np.linalg.inv(A.T @ A)


def case_with_groups(n_groups):
    """warren_case(8) with 4 (TRUE_FACTORS) or 8 (EIGHT_FACTORS) span groups."""
    return warren_case(8) if n_groups == 4 else warren_case(8, factors=EIGHT_FACTORS)


@functools.lru_cache(maxsize=None)
def reference_run(n_groups):
    """(case, identify_factors(case, misfit_tolerance=1e-15)) from all factors 1: computed once, shared by the tests
    that hold the device loop to the restatement's evaluation count."""
    case = case_with_groups(n_groups)
    return case, identify_factors(case, misfit_tolerance=1e-15)


@functools.lru_cache(maxsize=None)
def noisy_case(seed=0, sigma=NOISE_SIGMA):
    """warren_case(8) with Gaussian noise of standard deviation sigma on every measured value (numpy default_rng(seed),
    drawn level by level in ascending load factor)."""
    case = warren_case(8)
    rng = np.random.default_rng(seed)
    case.levels = [(lam, dofs, ubar + sigma * rng.standard_normal(len(ubar))) for lam, dofs, ubar in case.levels]
    return case
