"""Identification of a prestress (one additive initial strain t_h per group of elements), alone or with the E*A factors,
restated in numpy / scipy float64 on top of tests/gl_e0_reference.py: the right-hand side of the sensitivity solve with
respect to t_h (with the magnitude sums the round-off bound of the GPU test is stated in), the weighted residuals with
the joint Jacobian A = [A_q | A_t], the Levenberg-Marquardt loop on x = (q, t / scale) with the rejected-trial rule, and the
three cases the tests share.  Sparse direct solves by default; it shares no code with the kernels or with pinn_fem_amd.

  e0_e = e0_base_e + t_h(e),   N = ea (e - e0),   fe = (N / l0) d           d fe / d e0 = -(ea / l0) d
  K_t(u_k) s_kh = -d f_int / d t_h = sum_{e in h} +-(ea_e / l0_e) d_e        + at the second node, - at the first
  A_t rows: s_kh[m_k] / sqrt|m_k|;   A_q rows as gl_e0_reference.residuals_and_jacobian forms them
"""
import functools
from dataclasses import dataclass

import numpy as np
import scipy.sparse.linalg as spla

import gl_e0_reference as e0r
import gl_reference as gl
import identify_reference as ir

TRUE_OFFSETS = (-1e-3, 5e-4, -2e-4, 8e-4)


def prestress_rhs(nodes, el, u, ea, pgroups, n_t, dim):
    """[n_t, n_dofs], every row (fixed dofs included): row h = sum over the elements of group h of +-(ea_e / l0_e) d_e."""
    t = gl.element_state(nodes, el, u, 1.0, dim)[3]
    el = np.asarray(el, dtype=np.int64)
    term = (np.broadcast_to(np.asarray(ea, dtype=np.float64), (len(el),)) / t["l0"])[:, None] * t["d"]
    n_nodes = len(gl._as2d(nodes, dim))
    out = np.zeros((n_t, n_nodes, dim))
    for h in range(n_t):
        pick = np.flatnonzero(np.asarray(pgroups) == h)
        np.add.at(out[h], el[pick, 1], term[pick])
        np.add.at(out[h], el[pick, 0], -term[pick])
    return out.reshape(n_t, -1)


def prestress_rhs_scale(nodes, el, u, ea, pgroups, n_t, dim):
    """Per row and dof, the sum over the node's elements of group h of (|ea_e| / l0_e) (|d0_c| + |u_j,c| + |u_i,c|): the
    magnitude of the terms prestress_rhs is summed from, in front of any cancellation (in d as well)."""
    t = gl.element_state(nodes, el, u, 1.0, dim)[3]
    U = np.abs(np.asarray(u, dtype=np.float64).reshape(-1, dim))
    el = np.asarray(el, dtype=np.int64)
    mag = (np.abs(np.broadcast_to(np.asarray(ea, dtype=np.float64), (len(el),))) / t["l0"])[:, None] \
        * (np.abs(t["d0"]) + U[el[:, 1]] + U[el[:, 0]])
    out = np.zeros((n_t, len(U), dim))
    for h in range(n_t):
        pick = np.flatnonzero(np.asarray(pgroups) == h)
        np.add.at(out[h], el[pick, 1], mag[pick])
        np.add.at(out[h], el[pick, 0], mag[pick])
    return out.reshape(n_t, -1)


@dataclass
class PrestressCase:
    nodes: np.ndarray
    el: np.ndarray
    loads: np.ndarray          # at load factor 1
    fixed: np.ndarray
    ea0: float
    groups: object             # [ne] stiffness group of every element, or None: E*A is known (ea0 everywhere)
    factors: object            # the true factor of every stiffness group, or None
    pgroups: np.ndarray        # [ne] prestress group of every element (-1: given)
    offsets: np.ndarray        # the true t [H]
    e0_base: np.ndarray        # [ne] the known base initial strain
    levels: list               # [(load factor, dofs, measured values)]
    t0: np.ndarray             # the start

    @property
    def n_q(self):
        return 0 if self.groups is None else len(self.factors)

    @property
    def n_t(self):
        return len(self.offsets)

    @property
    def n_rows(self):
        return sum(len(dofs) for _, dofs, _ in self.levels)

    def ea(self, q):
        if self.groups is None:
            return np.full(len(self.el), self.ea0)
        return self.ea0 * np.exp(np.asarray(q, dtype=np.float64))[self.groups]

    def e0(self, t):
        pg = np.asarray(self.pgroups)
        return self.e0_base + np.where(pg >= 0, np.asarray(t, dtype=np.float64)[np.maximum(pg, 0)], 0.0)


class Refused(RuntimeError):
    """A point the restatement has no misfit at: a slack start, an indefinite tangent or no Newton convergence."""


def _spd_solve(solve):
    def checked(K, b):
        x = solve(K, b)
        if not np.all(np.isfinite(x)) or (np.any(b != 0.0) and not float(b @ x) > 0.0):
            raise Refused("the tangent is not positive definite")
        return x
    return checked


def residuals_and_jacobian(case, q, t, states=None, jacobian=True, tol=1e-10, linear_solve=spla.spsolve):
    """(rho [M], A = [A_q | A_t] [M, G + H] or None, displacements per level, Newton iterations per level) at the
    log-factors q [G] and the offsets t [H].  Every solve is held to rhs.x > 0 (the rule the device holds its CG solves to)
    and a diagonal of the starting tangent that is not positive on a free dof is refused, as is a Newton loop that does
    not converge: Refused."""
    nodes, el, dim = case.nodes, case.el, 2
    ea, e0 = case.ea(q), case.e0(t)
    n = len(case.loads)
    free = gl.free_mask(n, case.fixed)
    idx = np.flatnonzero(free)
    solve = _spd_solve(linear_solve)
    if not np.all(e0r.k_t(nodes, el, np.zeros(n), ea, e0, dim).diagonal()[idx] > 0.0):
        raise Refused("the tangent at the starting state has a diagonal that is not positive (a slack mechanism)")
    rho, rows, us, its, u = [], [], [], [], None
    for k, (lam, dofs, ubar) in enumerate(sorted(case.levels, key=lambda lv: lv[0])):
        if states is None:
            u, it, ok = e0r.newton(nodes, el, case.loads, case.fixed, ea, e0, dim, lam=lam, u0=u, tol=tol, linear_solve=solve)
            if not ok:
                raise Refused(f"Newton did not converge at load factor {lam}")
            its.append(it)
        else:
            u = np.asarray(states[k], dtype=np.float64)
        dofs, ubar = np.asarray(dofs, dtype=int), np.asarray(ubar, dtype=np.float64)
        w = 1.0 / np.sqrt(len(dofs))
        rho.append((u[dofs] - ubar) * w)
        if jacobian:
            Kff = gl.restrict(e0r.k_t(nodes, el, u, ea, e0, dim), free)
            B = prestress_rhs(nodes, el, u, ea, case.pgroups, case.n_t, dim)
            if case.n_q:
                Bq = np.stack([-e0r.f_int(nodes, el, u, np.where(case.groups == g, ea, 0.0), e0, dim) for g in range(case.n_q)])
                B = np.concatenate([Bq, B], axis=0)
            B[:, np.asarray(case.fixed, dtype=int)] = 0.0
            S = np.zeros_like(B)
            for g in range(len(B)):
                S[g, idx] = solve(Kff, B[g, idx])
            rows.append(S[:, dofs].T * w)
        us.append(u)
    return np.concatenate(rho), (np.concatenate(rows, axis=0) if jacobian else None), us, its


def levenberg_marquardt(case, q0=None, t0=None, scale=1e-3, max_evaluations=50, gtol=1e-12, misfit_tolerance=0.0,
                        damping=1e-3, step_tolerance=1e-12, **kw):
    """The loop of gl_e0_reference.levenberg_marquardt on x = (q, t / scale), with one more rule: a trial point that is
    Refused is a rejected step (mu <- 10 mu) and counts as an evaluation."""
    n_q = case.n_q
    q = np.zeros(n_q) if q0 is None else np.asarray(q0, dtype=np.float64)
    t = case.t0 if t0 is None else np.asarray(t0, dtype=np.float64)
    cols = np.concatenate([np.ones(n_q), np.full(case.n_t, scale)])

    def evaluate(x, **more):
        rho, A, states, _ = residuals_and_jacobian(case, x[:n_q], x[n_q:] * scale, **more, **kw)
        return rho, (None if A is None else A * cols), states

    x = np.concatenate([q, t / scale])
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
        except Refused as exc:
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
    return dict(q=x[:n_q], t=x[n_q:] * scale, factors=np.exp(x[:n_q]), misfit=J, rho=rho, jacobian=A / cols, states=states,
                evaluations=evaluations, stop=stop, history=history)


# ---- the cases -------------------------------------------------------------------------------------------------------
def _measure(nodes, el, loads, fixed, ea, e0, load_factors, dofs):
    levels, u = [], None
    for lam in load_factors:
        u, _, ok = e0r.newton(nodes, el, loads, fixed, ea, e0, 2, lam=lam, u0=u, tol=1e-12)
        assert ok
        levels.append((float(lam), dofs.copy(), u[dofs].copy()))
    return levels


@functools.lru_cache(maxsize=None)
def warren_case(joint=True, with_base=True):
    """ir.warren_case(8) (geometry, loads, span groups) with a prestress offset per span group (TRUE_OFFSETS) on top of a
    known random base e0 in +-1e-3 (with_base; else zero), every free dof measured at its three levels on the structure
    with the true parameters.  joint: the four true E*A factors of ir.warren_case are unknowns as well (start q = 0);
    otherwise E*A is known and uniform.  The start is t = 0."""
    base = ir.warren_case(8)
    ne = len(base.el)
    e0_base = np.random.default_rng(0).uniform(-e0r.E0_AMPLITUDE, e0r.E0_AMPLITUDE, ne) if with_base else np.zeros(ne)
    offsets = np.asarray(TRUE_OFFSETS)
    idx = np.flatnonzero(gl.free_mask(len(base.loads), base.fixed))
    ea_true = base.ea0 * base.factors[base.groups] if joint else np.full(ne, base.ea0)
    levels = _measure(base.nodes, base.el, base.loads, base.fixed, ea_true, e0_base + offsets[base.groups],
                      [lv[0] for lv in base.levels], idx)
    return PrestressCase(base.nodes, base.el, base.loads, base.fixed, base.ea0, base.groups if joint else None,
                         base.factors if joint else None, base.groups.copy(), offsets, e0_base, levels, np.zeros(4))


@functools.lru_cache(maxsize=None)
def cable_case():
    """e0r.cable_chain(16) (E*A 1000, pretension e0 = -1e-2; the middle sags by 0.29 at load factor 1): the vertical dofs of
    the inner nodes measured at load factors 0.5 and 1, one offset for the whole cable, the start t = -5e-3 (taut: at t = 0
    the cable has no stiffness across)."""
    n = 16
    nodes, el, loads, fixed = e0r.cable_chain(n, ea=1000.0, e0=-1e-2)
    dofs = np.arange(3, 2 * n, 2)
    levels = _measure(nodes, el, loads, fixed, np.full(n, 1000.0), np.full(n, -1e-2), [0.5, 1.0], dofs)
    return PrestressCase(nodes, el, loads, fixed, 1000.0, None, None, np.zeros(n, dtype=int), np.array([-1e-2]), np.zeros(n),
                         levels, np.array([-5e-3]))


NOISE_SIGMA = 1e-4


@functools.lru_cache(maxsize=None)
def noisy_case(seed=0):
    """warren_case(True, True) with Gaussian noise of NOISE_SIGMA on every measurement."""
    case = warren_case(True, True)
    rng = np.random.default_rng(seed)
    levels = [(lam, dofs, u + NOISE_SIGMA * rng.standard_normal(len(u))) for lam, dofs, u in case.levels]
    return PrestressCase(case.nodes, case.el, case.loads, case.fixed, case.ea0, case.groups, case.factors, case.pgroups,
                         case.offsets, case.e0_base, levels, case.t0)


def covariance(A, J):
    """J / (M - P) (A^T A)^-1 of (q, t), formed with unit columns and scaled back (the columns differ by 1e3 in size)."""
    M, P = A.shape
    norms = np.linalg.norm(A, axis=0)
    An = A / norms
    return J / (M - P) * np.linalg.inv(An.T @ An) / np.outer(norms, norms)


CASES = {"warren-prestress": lambda: warren_case(False, True), "warren-prestress-no-base": lambda: warren_case(False, False),
         "warren-joint": lambda: warren_case(True, True), "warren-joint-no-base": lambda: warren_case(True, False),
         "cable": cable_case}


@functools.lru_cache(maxsize=None)
def reference_run(name):
    """(case, levenberg_marquardt(case, misfit_tolerance=1e-15)) of CASES[name]: computed once, shared by the tests."""
    case = CASES[name]()
    return case, levenberg_marquardt(case, misfit_tolerance=1e-15)
