"""Initial (eigen-) strains in the Green-Lagrange truss element, restated in numpy / scipy float64 on top of
tests/gl_reference.py: element state, internal force, tangent, the Newton loop with a sparse direct solve, the adjoint
gradient and the Gauss-Newton identification of E*A factors on a prestressed structure, and the closed forms the tests pin
them to.  It shares no code with the kernels or with pinn_fem_amd/fem.  tests/test_gl_e0_host.py checks it against finite
differences and closed forms.

  W(u) = sum_e  E A l0 (e - e0)^2 / 2,   e = (|d|^2 - |d0|^2) / (2 l0^2),  d = d0 + du
  N = E A (e - e0),   fe = (N / l0) d,   B = (E A / l0^3) d d^T + (N / l0) I
e0 < 0 is a pretension (T = -E A e0), thermal loading is e0 = alpha dT, lack of fit e0 = (L_natural - l0) / l0.  e0 acts
in full at every load factor.
"""
import functools
from dataclasses import dataclass

import numpy as np
import scipy.sparse.linalg as spla

import gl_reference as gl
import identify_reference as ir


def _e0(e0, ne):
    return np.broadcast_to(np.asarray(e0, dtype=np.float64), (ne,))


def element_state(nodes, el, u, ea, e0, dim):
    """(strain [ne] (the total strain e), fe [ne, dim], B [ne, dim, dim], terms); `terms` is gl.element_state's with n the
    axial force E A (e - e0), e0 and e_abs = (2 |d0|.|du| + |du|.|du|) / (2 l0^2)."""
    strain, _, _, t = gl.element_state(nodes, el, u, ea, dim)
    e0 = _e0(e0, len(strain))
    n = t["ea"] * (strain - e0)
    n_l0 = n / t["l0"]
    fe = n_l0[:, None] * t["d"]
    B = (t["ea"] / (t["l02"] * t["l0"]))[:, None, None] * (t["d"][:, :, None] * t["d"][:, None, :]) \
        + n_l0[:, None, None] * np.eye(dim)
    e_abs = (2.0 * np.sum(np.abs(t["d0"]) * np.abs(t["du"]), axis=1) + np.sum(t["du"] ** 2, axis=1)) / (2.0 * t["l02"])
    return strain, fe, B, dict(t, n=n, e0=e0, e_abs=e_abs)


def axial_forces(nodes, el, u, ea, e0, dim):
    return element_state(nodes, el, u, ea, e0, dim)[3]["n"]


def f_int(nodes, el, u, ea, e0, dim):
    X, el = gl._as2d(nodes, dim), np.asarray(el, dtype=np.int64)
    fe = element_state(nodes, el, u, ea, e0, dim)[1]
    out = np.zeros((len(X), dim))
    np.add.at(out, el[:, 1], fe)
    np.add.at(out, el[:, 0], -fe)
    return out.reshape(-1)


def f_int_scale(nodes, el, u, ea, e0, dim):
    """gl.f_int_scale with (e_abs + |e0|) in place of e_abs: per dof the magnitude of the terms f_int is summed from, in
    front of the cancellation of e - e0 and of the sum over the node's elements."""
    X, el = gl._as2d(nodes, dim), np.asarray(el, dtype=np.int64)
    t = element_state(nodes, el, u, ea, e0, dim)[3]
    mag = (np.abs(t["ea"]) * (t["e_abs"] + np.abs(t["e0"])) / t["l0"])[:, None] * np.abs(t["d"])
    out = np.zeros((len(X), dim))
    np.add.at(out, el[:, 1], mag)
    np.add.at(out, el[:, 0], mag)
    return out.reshape(-1)


def k_t(nodes, el, u, ea, e0, dim):
    return gl.blocks_csr(element_state(nodes, el, u, ea, e0, dim)[2], el, len(gl._as2d(nodes, dim)), dim)


def energy(nodes, el, u, ea, e0, dim):
    strain, _, _, t = element_state(nodes, el, u, ea, e0, dim)
    return float(np.sum(t["ea"] * t["l0"] * (strain - t["e0"]) ** 2) / 2.0)


def newton(nodes, el, loads, fixed, ea, e0, dim, lam=1.0, u0=None, tol=1e-10, max_iter=50, min_den=1e-10, on_iterate=None,
           linear_solve=spla.spsolve):
    """gl.newton with the initial strain: the load factor scales the loads only.  Returns (u, iterations, converged)."""
    n = len(gl._as2d(nodes, dim)) * dim
    free = gl.free_mask(n, fixed)
    f = lam * np.asarray(loads, dtype=np.float64).reshape(-1)
    u = np.zeros(n) if u0 is None else np.where(free, np.asarray(u0, dtype=np.float64).reshape(-1), 0.0)
    for it in range(max_iter):
        K = k_t(nodes, el, u, ea, e0, dim)
        rhs = f - f_int(nodes, el, u, ea, e0, dim)
        if on_iterate is not None:
            on_iterate(u, K, free, rhs)
        du = np.zeros(n)
        du[free] = linear_solve(gl.restrict(K, free), rhs[free])
        u = u + du
        if np.linalg.norm(du) / max(np.linalg.norm(u), min_den) <= tol:
            return u, it + 1, True
    return u, max_iter, False


# ---- closed forms and meshes -----------------------------------------------------------------------------------------
class TautString:
    """Two collinear bars between supports at (-a, 0) and (a, 0), both with E*A = ea and the initial strain e0, load P
    across at the middle node.  With the middle's deflection w:  e = w^2 / (2 a^2),  N = ea (e - e0),
    P(w) = 2 N w / a."""

    def __init__(self, a=1.0, ea=1000.0, e0=-1e-3):
        self.a, self.ea, self.e0 = float(a), float(ea), float(e0)
        self.nodes = np.array([[-a, 0.0], [0.0, 0.0], [a, 0.0]])
        self.el = np.array([[0, 1], [1, 2]])
        self.fixed = np.array([0, 1, 4, 5])

    def strain(self, w):
        return w * w / (2.0 * self.a ** 2)

    def force(self, w):
        return self.ea * (self.strain(w) - self.e0)

    def load(self, w):
        return 2.0 * self.force(w) * w / self.a

    def loads(self, p):
        out = np.zeros(6)
        out[3] = p
        return out


class PrestressedTwoBar(gl.TwoBar):
    """gl.TwoBar with the initial strain e0 in both bars.  With the apex drop w:  e = (w^2 - 2 h w) / (2 l0^2),
    P(w) = E A ((w^2 - 2 h w) / (2 l0^2) - e0) (w - h) 2 / l0,  dP/dw = (2 E A / l0) ((3 (w - h)^2 - h^2) / (2 l0^2) - e0):
    the limit point is at w = h - sqrt((h^2 + 2 l0^2 e0) / 3) (a pretension beyond e0 = -h^2 / (2 l0^2) removes it), and
    the unloaded apex already sits at P(w) = 0 below w = 0 for e0 < 0."""

    def __init__(self, a=10.0, h=1.0, ea=1000.0, e0=-1e-3):
        self.e0 = float(e0)
        super().__init__(a, h, ea)
        self.w_lim = self.h - np.sqrt((self.h ** 2 + 2.0 * self.l0 ** 2 * self.e0) / 3.0)
        self.p_lim = self.load(self.w_lim)

    def tangent(self, w):
        return 2.0 * self.ea / self.l0 * ((3.0 * (w - self.h) ** 2 - self.h ** 2) / (2.0 * self.l0 ** 2) - self.e0)

    def load(self, w):
        return self.ea * (self.strain(w) - self.e0) * (w - self.h) * 2.0 / self.l0 ** 3 * self.l0 ** 2


def cable_chain(n, ea=1000.0, e0=-1e-2, sag=0.02):
    """n collinear unit elements between two supports with the pretension -ea e0 and equal loads across at every inner node:
    the load of a parabolic cable with a sag of `sag` of the span under that pretension, p = 8 T sag / n.
    Returns (nodes, el, loads, fixed)."""
    nodes = np.zeros((n + 1, 2))
    nodes[:, 0] = np.arange(n + 1)
    e = np.arange(n)
    el = np.stack([e, e + 1], axis=1)
    loads = np.zeros(2 * (n + 1))
    loads[3:2 * n:2] = -8.0 * (-ea * e0) * sag / n
    return nodes, el, loads, np.array([0, 1, 2 * n, 2 * n + 1])


def heated_bar(n, h=0.75):
    """1-D chain of n equal elements between two supports.  Returns (x, el, fixed)."""
    x = h * np.arange(n + 1)
    e = np.arange(n)
    return x, np.stack([e, e + 1], axis=1), np.array([0, n])


# ---- identification --------------------------------------------------------------------------------------------------
def element_sensitivity(nodes, el, u, a, e0, dim):
    """-((e - e0) / l0) d.(a_j - a_i) per element."""
    strain, _, _, t = element_state(nodes, el, u, 1.0, e0, dim)
    A = np.asarray(a, dtype=np.float64).reshape(-1, dim)
    el = np.asarray(el, dtype=np.int64)
    return -((strain - t["e0"]) / t["l0"]) * np.sum(t["d"] * (A[el[:, 1]] - A[el[:, 0]]), axis=1)


def sensitivity_scale(nodes, el, u, a, e0, dim):
    """ir.sensitivity_scale with (e_abs + |e0|) in place of e_abs: the magnitude in front of the cancellation of e - e0."""
    t = element_state(nodes, el, u, 1.0, e0, dim)[3]
    A = np.abs(np.asarray(a, dtype=np.float64).reshape(-1, dim))
    el = np.asarray(el, dtype=np.int64)
    return ((t["e_abs"] + np.abs(t["e0"])) / t["l0"]) * np.sum(np.abs(t["d"]) * (A[el[:, 1]] + A[el[:, 0]]), axis=1)


def misfit_and_gradient(nodes, el, loads, fixed, ea, e0, dim, levels, tol=1e-10, linear_solve=spla.spsolve):
    """ir.misfit_and_gradient with the initial strain.  Returns (J, dJ/d ea [ne], displacements per level, iterations)."""
    n = len(gl._as2d(nodes, dim)) * dim
    free = gl.free_mask(n, fixed)
    idx = np.flatnonzero(free)
    J, grad, us, its, u = 0.0, np.zeros(len(el)), [], [], None
    for lam, dofs, ubar in sorted(levels, key=lambda lv: lv[0]):
        u, it, ok = newton(nodes, el, loads, fixed, ea, e0, dim, lam=lam, u0=u, tol=tol, linear_solve=linear_solve)
        assert ok, f"reference Newton did not converge at load factor {lam}"
        dofs, ubar = np.asarray(dofs, dtype=int), np.asarray(ubar, dtype=np.float64)
        r = u[dofs] - ubar
        J += float(np.mean(r * r))
        g = np.zeros(n)
        np.add.at(g, dofs, 2.0 * r / len(dofs))
        a = np.zeros(n)
        a[idx] = linear_solve(gl.restrict(k_t(nodes, el, u, ea, e0, dim), free), g[idx])
        grad += element_sensitivity(nodes, el, u, a, e0, dim)
        us.append(u)
        its.append(it)
    return J, grad, us, its


@dataclass
class Case(ir.Case):
    e0: np.ndarray = None      # [ne] the initial strain the measurements were generated with

    def objective(self, q, e0=None, **kw):
        """(J, dJ/dq) at the log-factors q, with the case's initial strain (or the e0 given: 0.0 leaves it out)."""
        ea = self.ea(q)
        J, g_ea, _, _ = misfit_and_gradient(self.nodes, self.el, self.loads, self.fixed, ea, self.e0 if e0 is None else e0, 2,
                                            self.levels, **kw)
        return J, ir.group_reduce(g_ea, ea, self.groups, self.n_groups)


E0_AMPLITUDE = 1e-3


@functools.lru_cache(maxsize=None)
def warren_case(n_panels=8, amplitude=E0_AMPLITUDE, seed=0):
    """ir.warren_case(n_panels) (geometry, loads, groups and true factors) with a random initial strain in +-amplitude in
    every element and the measurements generated WITH it: every free dof at every load level from this file's Newton."""
    base = ir.warren_case(n_panels)
    e0 = np.random.default_rng(seed).uniform(-amplitude, amplitude, len(base.el))
    idx = np.flatnonzero(gl.free_mask(len(base.loads), base.fixed))
    ea_true = base.ea0 * base.factors[base.groups]
    levels, u = [], None
    for lam, _, _ in base.levels:
        u, _, ok = newton(base.nodes, base.el, base.loads, base.fixed, ea_true, e0, 2, lam=lam, u0=u, tol=1e-12)
        assert ok
        levels.append((float(lam), idx.copy(), u[idx].copy()))
    return Case(base.nodes, base.el, base.loads, base.fixed, base.tip, base.ea0, base.groups, base.factors, levels, e0)


def residuals_and_jacobian(case, q, e0, states=None, jacobian=True, tol=1e-10, linear_solve=spla.spsolve):
    """gn.residuals_and_jacobian with the initial strain e0 in the Newton solves, the tangent and the group forces."""
    nodes, el, dim = case.nodes, case.el, 2
    ea = case.ea(q)
    free = gl.free_mask(len(case.loads), case.fixed)
    idx = np.flatnonzero(free)
    rho, rows, us, its, u = [], [], [], [], None
    for k, (lam, dofs, ubar) in enumerate(sorted(case.levels, key=lambda lv: lv[0])):
        if states is None:
            u, it, ok = newton(nodes, el, case.loads, case.fixed, ea, e0, dim, lam=lam, u0=u, tol=tol, linear_solve=linear_solve)
            assert ok, f"reference Newton did not converge at load factor {lam}"
            its.append(it)
        else:
            u = np.asarray(states[k], dtype=np.float64)
        dofs, ubar = np.asarray(dofs, dtype=int), np.asarray(ubar, dtype=np.float64)
        w = 1.0 / np.sqrt(len(dofs))
        rho.append((u[dofs] - ubar) * w)
        if jacobian:
            Kff = gl.restrict(k_t(nodes, el, u, ea, e0, dim), free)
            B = np.stack([-f_int(nodes, el, u, np.where(case.groups == g, ea, 0.0), e0, dim) for g in range(case.n_groups)])
            B[:, np.asarray(case.fixed, dtype=int)] = 0.0
            S = np.zeros_like(B)
            for g in range(case.n_groups):
                S[g, idx] = linear_solve(Kff, B[g, idx])
            rows.append(S[:, dofs].T * w)
        us.append(u)
    return np.concatenate(rho), (np.concatenate(rows, axis=0) if jacobian else None), us, its


def levenberg_marquardt(case, e0, q0=None, max_evaluations=200, gtol=1e-12, misfit_tolerance=0.0, damping=1e-3,
                        step_tolerance=1e-12, **kw):
    """gn.levenberg_marquardt on this file's residuals: the loop of identify_nr(method="gauss-newton") with the initial
    strain e0 in the model (0.0: the identification that leaves the prestress out)."""
    q = np.zeros(case.n_groups) if q0 is None else np.asarray(q0, dtype=np.float64).copy()
    rho, A, states, _ = residuals_and_jacobian(case, q, e0, **kw)
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
        rho_t, _, states_t, _ = residuals_and_jacobian(case, q + delta, e0, jacobian=False, **kw)
        evaluations += 1
        J_t = float(rho_t @ rho_t)
        history.append(dict(misfit=J_t, accepted=J_t < J, damping=mu))
        if J_t < J:
            q, rho, J, states = q + delta, rho_t, J_t, states_t
            A = residuals_and_jacobian(case, q, e0, states=states, **kw)[1]
            mu = max(mu / 10.0, 1e-12)
        else:
            mu *= 10.0
            if mu > 1e12:
                stop = "damping"
                break
    return dict(q=q, factors=np.exp(q), misfit=J, rho=rho, jacobian=A, states=states, evaluations=evaluations, stop=stop,
                history=history)


@functools.lru_cache(maxsize=None)
def reference_run(with_prestress=True):
    """(case, levenberg_marquardt(case, misfit_tolerance=1e-15)) on warren_case() from all factors 1, with the case's
    initial strain in the model or (with_prestress False) left out of it: computed once, shared by the tests."""
    case = warren_case()
    return case, levenberg_marquardt(case, case.e0 if with_prestress else 0.0, misfit_tolerance=1e-15)
