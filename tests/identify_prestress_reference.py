"""Identification of a prestress (one additive initial strain t_h per group of elements), alone or with the E*A factors:
the cases the tests pin tests/identify_reference.py's residuals with the joint Jacobian A = [A_q | A_t] and its loop on
x = (q, t / scale) with the rejected-trial rule (identify_prestress) to, and the covariance of (q, t).  The right-hand side
of the sensitivity solve with respect to t_h is gl_reference.prestress_rhs.  It shares no code with the kernels or with
pinn_fem_amd.

  e0_e = e0_base_e + t_h(e),   N = ea (e - e0),   fe = (N / l0) d           d fe / d e0 = -(ea / l0) d
  K_t(u_k) s_kh = -d f_int / d t_h = sum_{e in h} +-(ea_e / l0_e) d_e        + at the second node, - at the first
  A_t rows: s_kh[m_k] / sqrt|m_k|, behind the A_q rows of the factors
"""
import functools
from dataclasses import dataclass

import numpy as np

import gl_e0_reference as e0r
import gl_reference as gl
import identify_reference as ir

TRUE_OFFSETS = (-1e-3, 5e-4, -2e-4, 8e-4)


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


# ---- the cases -------------------------------------------------------------------------------------------------------
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
    levels = ir.measure(base.nodes, base.el, base.loads, base.fixed, ea_true, [lv[0] for lv in base.levels], idx,
                        e0=e0_base + offsets[base.groups])
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
    levels = ir.measure(nodes, el, loads, fixed, np.full(n, 1000.0), [0.5, 1.0], dofs, e0=np.full(n, -1e-2))
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
    """(case, ir.identify_prestress(case, misfit_tolerance=1e-15)) of CASES[name]: computed once, shared by the tests."""
    case = CASES[name]()
    return case, ir.identify_prestress(case, misfit_tolerance=1e-15)
