"""Gauss-Newton identification of E*A factors in numpy / scipy float64, on top of tests/gl_reference.py and
tests/identify_reference.py: the weighted residuals over the load levels, their Jacobian with respect to one log-factor per
group by one sensitivity solve per level and group, and the Levenberg-Marquardt loop of identify_nr(method="gauss-newton").
Sparse direct solves by default; it shares no code with the kernels or with pinn_fem_amd/fem/identify.py.

  rho = (u_k[m_k] - ubar_k) / sqrt|m_k| stacked over the levels,   J = rho.rho
  f_int(u_k; ea) = lam_k f,  ea_e = ea0 exp(q_group(e))   =>   K_t(u_k) s_kg = -f_int(u_k; ea restricted to group g)
  A = d rho / d q: the rows of s_kg at m_k over sqrt|m_k|,   dJ/dq = 2 A^T rho
"""
import functools

import numpy as np
import scipy.sparse.linalg as spla

import gl_reference as gl
import identify_reference as ir

EIGHT_FACTORS = (1.0, 0.7, 1.3, 0.85, 1.1, 0.9, 1.2, 0.8)
NOISE_SIGMA = 1e-4


def group_rhs(nodes, el, u, ea, dim, groups, n_groups, fixed):
    """[G, n_dofs]: minus the internal force of the elements of every group alone, zero on the fixed dofs."""
    ea = np.broadcast_to(np.asarray(ea, dtype=np.float64), (len(el),))
    groups = np.asarray(groups, dtype=int)
    out = np.stack([-gl.f_int(nodes, el, u, np.where(groups == g, ea, 0.0), dim) for g in range(n_groups)])
    out[:, np.asarray(fixed, dtype=int)] = 0.0
    return out


def residuals_and_jacobian(case, q, states=None, jacobian=True, tol=1e-10, linear_solve=spla.spsolve):
    """(rho [M], A [M, G] or None, displacements per level in ascending load factor, Newton iterations per level) at the
    log-factors q.  states given: those are the u_k, no Newton solves."""
    nodes, el, dim = case.nodes, case.el, 2
    ea = case.ea(q)
    n = len(case.loads)
    free = gl.free_mask(n, case.fixed)
    idx = np.flatnonzero(free)
    rho, rows, us, its, u = [], [], [], [], None
    for k, (lam, dofs, ubar) in enumerate(sorted(case.levels, key=lambda lv: lv[0])):
        if states is None:
            u, it, ok = gl.newton(nodes, el, case.loads, case.fixed, ea, dim, lam=lam, u0=u, tol=tol, linear_solve=linear_solve)
            assert ok, f"reference Newton did not converge at load factor {lam}"
            its.append(it)
        else:
            u = np.asarray(states[k], dtype=np.float64)
        dofs, ubar = np.asarray(dofs, dtype=int), np.asarray(ubar, dtype=np.float64)
        w = 1.0 / np.sqrt(len(dofs))
        rho.append((u[dofs] - ubar) * w)
        if jacobian:
            Kff = gl.restrict(gl.k_t(nodes, el, u, ea, dim), free)
            B = group_rhs(nodes, el, u, ea, dim, case.groups, case.n_groups, case.fixed)
            S = np.zeros_like(B)
            for g in range(case.n_groups):
                S[g, idx] = linear_solve(Kff, B[g, idx])
            rows.append(S[:, dofs].T * w)
        us.append(u)
    return np.concatenate(rho), (np.concatenate(rows, axis=0) if jacobian else None), us, its


def levenberg_marquardt(case, q0=None, max_evaluations=200, gtol=1e-12, misfit_tolerance=0.0, damping=1e-3,
                        step_tolerance=1e-12, **kw):
    """The loop of identify_nr(method="gauss-newton"), restated.  Returns a dict: q, factors, misfit, rho, jacobian, states,
    evaluations, stop, history ([{misfit, accepted, damping}] per evaluation)."""
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


def covariance(A, J):
    """J / (M - G) (A^T A)^-1: the covariance of the log-factors of the weighted fit."""
    M, G = A.shape
    return J / (M - G) * np.linalg.inv(A.T @ A)


def case_with_groups(n_groups):
    """warren_case(8) with 4 (identify_reference.TRUE_FACTORS) or 8 (EIGHT_FACTORS) span groups."""
    return ir.warren_case(8) if n_groups == 4 else ir.warren_case(8, factors=EIGHT_FACTORS)


@functools.lru_cache(maxsize=None)
def reference_run(n_groups):
    """(case, levenberg_marquardt(case, misfit_tolerance=1e-15)) from all factors 1: computed once, shared by the tests
    that hold the device loop to the restatement's evaluation count."""
    case = case_with_groups(n_groups)
    return case, levenberg_marquardt(case, misfit_tolerance=1e-15)


@functools.lru_cache(maxsize=None)
def noisy_case(seed=0, sigma=NOISE_SIGMA):
    """warren_case(8) with Gaussian noise of standard deviation sigma on every measured value (numpy default_rng(seed),
    drawn level by level in ascending load factor)."""
    case = ir.warren_case(8)
    rng = np.random.default_rng(seed)
    case.levels = [(lam, dofs, ubar + sigma * rng.standard_normal(len(ubar))) for lam, dofs, ubar in case.levels]
    return case
