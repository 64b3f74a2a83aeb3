"""Identification of a prestress (an additive initial strain per group of elements), alone or together with the E*A factors
of fem/identify.py, from displacements and strains measured through the Green-Lagrange Newton solve.

The parameters: prestress_groups [n_elems] holds ids 0..H-1 (-1: the element's e0 is given, not identified) and one
strain t_h per group is ADDED to the base initial strain, e0_e = e0_base_e + t_h(e), with e0_base config.initial_strain or
zero; optionally, alongside, the log-factors q_g of identify_nr on a stiffness group map, ea_e = ea0 exp(q_g(e)).

f_int is affine in e0: N = ea (e - e0), fe = (N / l0) d, so d fe / d e0 = -(ea / l0) d and, differentiating the equilibrium
f_int(u_k; ea, e0) = lam_k f with respect to t_h,

  K_t(u_k) s_kh = - d f_int / d t_h = sum_{e in h} +-(ea_e / l0_e) d_e        + at the element's second node, - at its first,
                                                                             zero on fixed dofs        (pf_gl_prestress_rhs)

on the tangent the Newton loop has just converged on.  All H right-hand sides of a level are one launch; they are stacked
under the G right-hand sides of the factors (pf_gl_group_rhs) and solved by one pcg_solve_many behind one preconditioner
setup.  identify._residuals forms these rows as it forms the factors': s at the measured dofs over
sqrt|m_k|, and (L / sqrt p) B s at the gauges (pf_gl_strain_jvp).  The measured strain is the TOTAL strain e: it depends on
t only through u.  The joint Jacobian is A = [A_q | A_t].

The loop is the Levenberg-Marquardt loop of identify_nr(method="gauss-newton") on x = (q, t / prestress_scale); its step
(H + mu diag H) delta = -A^T rho is invariant to the scale of a column, so the gap between log-factors (order 1) and
strains (order 1e-3) does not enter it.

Limits: those of fem/identify.py (a positive definite tangent at every state, load control, a scalar base material, no
regularisation, no bounds), and an additive prestress only.  A structure that has no stiffness at u = 0 without its
prestress (a cable) needs a taut start t0: the refusal of the slack starting state says so.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np
import torch

from . import solver as _solver
from .identify import (_GN_COUNTERS, _add_counters, _base_ea, _check_ea, _checked, _levenberg_marquardt, _newton_level,
                       check_gauss_newton)
from .identify import _residuals as _factor_residuals
from .model import FEMModel
from .solver import SolverConfig


@dataclass
class PrestressResult:
    prestress: np.ndarray                # t [H]: the strain added to the base initial strain of every prestress group
    initial_strain: np.ndarray           # [n_elems] e0_base + t[prestress_groups]
    factors: Optional[np.ndarray]        # exp(q) [G]; None when groups is None
    ea: np.ndarray                       # [n_elems] identified E*A (the base E*A when groups is None)
    misfit: float                        # J = rho.rho at the returned point
    evaluations: int                     # misfit evaluations (Newton solves of every level), rejected trials included
    converged: bool                      # stopped on a tolerance ("misfit", "gradient" or "step")
    stop: str                            # "misfit" | "gradient" | "step" | "cap" | "damping"
    history: List[Dict] = field(default_factory=list)     # one {misfit, gradient_norm, factors, prestress, accepted, damping}
                                                          # per evaluation; a trial that raised: misfit None and "error"
    displacements: List[np.ndarray] = field(default_factory=list)   # per level, ascending load factor
    strains: List[np.ndarray] = field(default_factory=list)         # per level, every element's total strain
    reactions: Optional[np.ndarray] = None                          # of the last level
    axial_forces: Optional[np.ndarray] = None                       # N = ea (e - e0) of every element at the last level
    counters: Dict[str, int] = field(default_factory=dict)          # identify_nr's Gauss-Newton counters, all evaluations
    jacobian: Optional[np.ndarray] = None          # A = [A_q | A_t] [M, G + H], in the parameters' own units
    singular_values: Optional[np.ndarray] = None   # of A with every column scaled to unit length, descending
    covariance: Optional[np.ndarray] = None        # J / (M - P) (A^T A)^-1 of (q, t), own units (None when M <= P)
    prestress_std: Optional[np.ndarray] = None     # sqrt(diag covariance) of t
    factor_std: Optional[np.ndarray] = None        # factors * sqrt(diag covariance) of q (None when groups is None)


def check_prestress(model: FEMModel, config: SolverConfig, levels, prestress_groups, t0=None, groups=None, q0=None):
    """What the identification of a prestress needs, checked before an engine is built; every violation is a ValueError:
    everything check_identify and check_strains refuse (linear kinematics, displacement control, NN materials, a sharded
    run, bad levels, a bad stiffness group map or q0), a prestress group map of the wrong length, with non-integer ids or
    ids below -1, an id in 0..H-1 without an element, no element identified at all, a t0 of the wrong length or not
    finite, and more parameters H + G than measurement rows.
    Returns ([_Level] in ascending order of load factor, prestress_groups int64 [n_elems], t0 float64 [H], groups int64
    [n_elems] or None, q0 float64 [G] (empty when groups is None), M the number of measurement rows)."""
    levels, groups, q = _checked(model, config, levels, groups, q0 if groups is not None else None)
    if groups is None:
        q = np.zeros(0)
    pg = np.asarray(prestress_groups).reshape(-1)
    if pg.size != model.nelm:
        raise ValueError(f"the prestress group map has the wrong length: {pg.size} entries for {model.nelm} elements.")
    if pg.dtype.kind not in "iu":
        raise ValueError("the prestress group map must hold integer group ids (-1: the element's e0 is given).")
    if pg.size and pg.min() < -1:
        raise ValueError("the prestress group map holds ids below -1 (-1: the element's e0 is given).")
    pg = pg.astype(np.int64)
    n_t = int(pg.max()) + 1 if pg.size else 0
    if n_t < 1:
        raise ValueError("the prestress group map identifies no element: every id is -1.")
    empty = np.flatnonzero(np.bincount(pg[pg >= 0], minlength=n_t) == 0)
    if empty.size:
        raise ValueError(f"prestress groups {empty.tolist()} have no element: their strains are not determined.")
    t = np.zeros(n_t) if t0 is None else np.asarray(t0, dtype=np.float64).reshape(-1)
    if t.size != n_t:
        raise ValueError(f"t0 has {t.size} entries for {n_t} prestress groups.")
    if not np.all(np.isfinite(t)):
        raise ValueError("t0 holds non-finite strains.")
    n_rows = sum(len(lv.dofs) + (len(lv.gauges[0]) if lv.gauges is not None else 0) for lv in levels)
    if n_t + q.size > n_rows:
        raise ValueError(f"{n_t} prestress groups and {q.size} stiffness groups for {n_rows} measurement rows: the "
                         "least-squares problem is underdetermined.")
    return levels, pg, t.copy(), groups, q, n_rows


def _base_e0(s, model) -> np.ndarray:
    return np.zeros(model.nelm) if s.e0_np is None else s.e0_np


def _initial_strain(s, model, pg, t) -> np.ndarray:
    """e0_base + t[prestress_groups] of one evaluation; an entry that is no eigenstrain (not finite, or 0.5 and above in
    magnitude: check_initial_strain's rule) is a RuntimeError, so that a trial point there is a rejected step."""
    e0 = _base_e0(s, model) + np.where(pg >= 0, np.asarray(t, dtype=np.float64)[np.maximum(pg, 0)], 0.0)
    if not np.all(np.isfinite(e0)) or (e0.size and float(np.max(np.abs(e0))) >= 0.5):
        raise RuntimeError("the initial strain of this point is not finite or not smaller than 0.5 in magnitude: no misfit "
                           "at this point")
    return np.ascontiguousarray(e0)


def _ea_of(model, groups, q) -> np.ndarray:
    ea0 = _base_ea(model)
    return np.full(model.nelm, ea0) if groups is None else ea0 * np.exp(np.asarray(q, dtype=np.float64))[groups]


def residuals_and_jacobian_prestress(model: FEMModel, config: SolverConfig, levels, prestress_groups, t, groups=None,
                                     q=None, states=None, jacobian: bool = True):
    """The weighted residuals rho [M] of identify.residuals_and_jacobian at the prestress strains t [H] (and the log-factors
    q [G] on the stiffness group map `groups`; None: the model's E*A), and their Jacobian A = [A_q | A_t] [M, G + H].

    Per level, in ascending load factor, the Newton loop of an identification evaluation with e0 = e0_base +
    t[prestress_groups] in every gl_state call, started from the previous level's state (states given: no Newton solves);
    with jacobian, the element state at u_k, the G right-hand sides of gl_group_rhs (G > 0), the H of gl_prestress_rhs,
    ONE pcg_solve_many on the stacked G + H rows, each solve held to solve_nr's rule, and the rows at the measured dofs
    and at the gauges (gl_strain_jvp) exactly as residuals_and_jacobian forms them.  A parameter that moves no measured
    dof and no gauge (a zero column) is a RuntimeError naming it.
    Returns (rho, A or None, displacements per level on the device, residuals_and_jacobian's counters)."""
    config = config or SolverConfig()
    levels, pg, t, groups, q, _ = check_prestress(model, config, levels, prestress_groups, t, groups, q)
    s = _solver._newton_setup(model, _solver.check_initial_strain(config, model))
    if states is not None and len(states) != len(levels):
        raise ValueError(f"states has {len(states)} entries for {len(levels)} levels")
    return _residuals(s, model, config, levels, pg, t, groups, q, states, jacobian)


def _residuals(s, model, config, levels, pg, t, groups, q, states=None, jacobian=True):
    """residuals_and_jacobian_prestress on checked input: s the solver's _newton_setup with the BASE initial strain, the
    rest check_prestress's.  This point's e0 and ea, then identify._residuals with the prestress map."""
    e0_np = _initial_strain(s, model, pg, t)
    s = s._replace(e0_np=e0_np, e0=torch.from_numpy(e0_np).to(s.eng.device))
    ea_t = torch.from_numpy(_check_ea(model, _ea_of(model, groups, q))).to(s.eng.device)
    return _factor_residuals(s, model, config, levels, ea_t, groups, states, jacobian, prestress=pg)


def identify_prestress(model: FEMModel, config: Optional[SolverConfig], levels, prestress_groups, groups=None, t0=None,
                       q0=None, prestress_scale: float = 1e-3, max_evaluations: int = 50, gtol: float = 1e-12,
                       misfit_tolerance: float = 0.0, damping: float = 1e-3,
                       step_tolerance: float = 1e-12) -> PrestressResult:
    """The strains t_h, one per prestress group, that added to the base initial strain (config.initial_strain, or zero)
    make the Green-Lagrange Newton solve match the measurements of `levels` (identify_nr's levels, strain-gauge keys
    included); with `groups`, the factors on E*A of identify_nr are identified alongside.  prestress_groups: [n_elems]
    ids 0..H-1, -1 for an element whose e0 is given.  From t0 (None: zeros) and q0 (None: zeros, every factor 1).

    The Levenberg-Marquardt loop of identify_nr(method="gauss-newton"), with the same stops ("misfit", "gradient", "cap",
    "step", "damping") and the same mu rule, on x = (q, t / prestress_scale) with the Jacobian of
    residuals_and_jacobian_prestress; gtol and step_tolerance are in the units of x.  One difference: a trial point whose
    evaluation raises RuntimeError (a slack or non-positive-definite state, no Newton convergence) is a REJECTED step: mu
    becomes 10 mu and the history entry carries the message under "error"; it counts as an evaluation.  The first
    evaluation's error propagates: a structure with no stiffness at u = 0 without its prestress (a cable) needs a taut
    t0, and the refusal of the slack starting state says so.

    The result carries the covariance of (q, t) = J / (M - P) (A^T A)^-1 in the parameters' own units (the weighted
    fit's, as identify_nr's), prestress_std and factor_std from it, and the state of every level at the returned point."""
    config = config or SolverConfig()
    levels, pg, t_start, groups, q_start, n_rows = check_prestress(model, config, levels, prestress_groups, t0, groups, q0)
    if int(max_evaluations) < 1:
        raise ValueError("max_evaluations must be at least 1")
    scale = float(prestress_scale)
    if not (np.isfinite(scale) and scale > 0.0):
        raise ValueError("prestress_scale must be positive and finite.")
    n_q, n_t = len(q_start), len(t_start)
    if groups is not None:
        check_gauss_newton([lv[:3] for lv in levels], groups, damping, [lv.gauges for lv in levels])
    damping = float(damping)
    if not (np.isfinite(damping) and damping > 0.0):
        raise ValueError("damping must be positive and finite.")
    s = _solver._newton_setup(model, _solver.check_initial_strain(config, model))
    eng = s.eng
    counters = dict.fromkeys(_GN_COUNTERS, 0)
    col_scale = np.concatenate([np.ones(n_q), np.full(n_t, scale)])

    def evaluate(x, **kw):
        rho, A, states, c = _residuals(s, model, config, levels, pg, x[n_q:] * scale, groups, x[:n_q], **kw)
        _add_counters(counters, c)
        return rho, (None if A is None else A * col_scale), states

    def describe(x):
        return {"factors": np.exp(x[:n_q]) if groups is not None else None, "prestress": x[n_q:] * scale}

    x, rho, A_x, states, history, stop, evaluations = _levenberg_marquardt(
        evaluate, np.concatenate([q_start, t_start / scale]), describe, max_evaluations, gtol, misfit_tolerance, damping,
        step_tolerance)
    q, t = x[:n_q], x[n_q:] * scale
    J = float(rho @ rho)
    A = A_x / col_scale
    norms = np.linalg.norm(A, axis=0)
    covariance = prestress_std = factor_std = None
    if n_rows > n_q + n_t:
        covariance = J / (n_rows - n_q - n_t) * np.linalg.inv(A_x.T @ A_x) * np.outer(col_scale, col_scale)
        std = np.sqrt(np.diag(covariance))
        prestress_std = std[n_q:]
        factor_std = np.exp(q) * std[:n_q] if groups is not None else None
    e0_np = _initial_strain(s, model, pg, t)
    e0_t = torch.from_numpy(e0_np).to(eng.device)
    ea_np = _ea_of(model, groups, q)
    ea_t = torch.from_numpy(ea_np).to(eng.device)
    strains = [eng.gl_state(u, ea_t, e0_t).cpu().numpy() for u in states]          # the last call: the last level's state
    reactions = eng.gl_fint().cpu().numpy() - levels[-1].load_factor * np.asarray(model.loads, dtype=float).reshape(-1)
    reactions[s.free] = 0.0
    return PrestressResult(
        prestress=t, initial_strain=e0_np, factors=np.exp(q) if groups is not None else None, ea=ea_np, misfit=J,
        evaluations=evaluations, converged=stop in ("misfit", "gradient", "step"), stop=stop, history=history,
        displacements=[u.cpu().numpy() for u in states], strains=strains, reactions=reactions,
        axial_forces=ea_np * (strains[-1] - e0_np), counters=counters, jacobian=A,
        singular_values=np.linalg.svd(A / norms, compute_uv=False), covariance=covariance, prestress_std=prestress_std,
        factor_std=factor_std)
