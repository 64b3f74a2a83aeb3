"""Identification of element stiffness E*A from measured displacements through the Green-Lagrange Newton solve
(DESIGN.md §7).

The data are load levels k: a load factor lam_k, measured dofs m_k and values ubar_k.  The state u_k solves
f_int(u_k; ea) = lam_k f on the free dofs.  With solve_gd's loss_data summed over the levels,

  J = sum_k mean_{m in m_k} (u_k[m] - ubar_k[m])^2
  K_t(u_k) a_k = g_k,   g_k[m] = 2 (u_k[m] - ubar_k[m]) / |m_k|         one adjoint solve per level, on the tangent the
                                                                         Newton loop has just converged on
  dJ/d ea_e = - sum_k (e / l0) d.(a_j - a_i)                             pf_gl_sens, accumulated in level order

and, with an element -> group map and one log-factor per group, ea_e = ea0 exp(q_group(e)) and
dJ/dq_g = sum_{e in g} ea_e dJ/d ea_e (pf_group_sum_f64).  No finite differences, no dense matrix.

Gauss-Newton (identify_nr(method="gauss-newton")): the problem is a small nonlinear least-squares problem,
J = rho.rho with rho the residuals r_k / sqrt|m_k| stacked over the levels, and its Jacobian is cheap.  Differentiating the
equilibrium with respect to the log-factor q_g of a group,

  K_t(u_k) s_kg = - d f_int / d q_g = - f_int of the elements of group g alone     (f_int is linear in E*A)

the right-hand side is the node gather of the fe records gl_state has just written, with a group filter
(pf_gl_group_rhs), the operator is the tangent the Newton loop has just converged on, and the batched tangent CG carries
two such right-hand sides per solve (pcg_solve_many: one coarse-space refresh per level).  The rows of s_kg at m_k over
sqrt|m_k| are the Jacobian A [M, G]; 2 A^T rho is the adjoint gradient.  Levenberg-Marquardt on A needs a handful of
evaluations where L-BFGS needs fifty, and A gives the covariance of the factors.

Strain gauges: a level may carry, beside or in place of its measured dofs, the Green-Lagrange strains ebar of p_k elements
("strain_elements", "strains") and a length L_k ("strain_scale", default 1) that makes them commensurable with
displacements.  This is the strain pf_gl_state writes, e = (l^2 - l0^2) / (2 l0^2); an engineering strain eps converts as
e = eps + eps^2 / 2 (there is no conversion option).  With B = d e / d u,  d e_e / d u_j = +d_e / l0^2 = -d e_e / d u_i
(e is quadratic in u, so this is exact; it does not contain E*A, so no other term of the derivations changes),

  J   += sum_k L_k^2 mean_{i < p_k} (e_k[elem_i] - ebar_ki)^2
  g_k += B^T c,   c_e = 2 L_k^2 (e_e - ebar_e) / p_k on the measured elements, 0 elsewhere      (pf_gl_strain_rhs)
  rho:  per level the displacement rows, then L_k (e - ebar) / sqrt p_k;   A: (L_k / sqrt p_k) B s_kg at the gauges
                                                                                                  (pf_gl_strain_jvp)

Initial strains: config.initial_strain (solver.check_initial_strain) gives every element an eigenstrain e0,
N = ea (e - e0).  It goes into every gl_state call (the Newton loops, the states the adjoint and the sensitivity solves are
taken at, the reactions) and into the sensitivity, dJ/d ea_e = - sum_k ((e - e0) / l0) d.(a_j - a_i) (pf_gl_sens_e0).
f_int stays linear in E*A and the group's own fe records already hold the prestress, so pf_gl_group_rhs needs nothing; the
strains, measured and computed, stay the total strains e.  A measured structure carries its prestress: fitted without it,
the error goes into the factors.

Limits: states with a positive definite tangent only (the CG solves), load control only, a scalar base material, no
regularisation term, no bounds on the factors and no weight per sensor but strain_scale; what a set of gauges
determines is what the singular values of A say, not more.  The initial strain is given here; fem/prestress.py identifies it.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, NamedTuple, Optional

import numpy as np
import torch

from . import solver as _solver
from .model import FEMModel
from .solver import SolverConfig


@dataclass
class IdentifyResult:
    factors: np.ndarray                  # exp(q): one per group (groups=None: one per element)
    ea: np.ndarray                       # [n_elems] identified E*A
    misfit: float                        # J at `factors`
    gradient: np.ndarray                 # dJ/dq at `factors`
    evaluations: int                     # misfit evaluations (Newton solves of every level plus the adjoint solves)
    converged: bool                      # stopped on a tolerance (False: the evaluation cap ended it)
    history: List[Dict] = field(default_factory=list)     # one {misfit, gradient_norm, factors} per evaluation
    displacements: List[np.ndarray] = field(default_factory=list)   # per level, ascending load factor, at `factors`
    counters: Dict[str, int] = field(default_factory=dict)          # Newton, CG and adjoint CG iterations, all evaluations
    reactions: Optional[np.ndarray] = None                          # of the last level, at `factors`
    strains: Optional[List[np.ndarray]] = None     # per level, every element's Green-Lagrange strain at `factors` (None
                                                   # unless some level carries strain data)
    # method "gauss-newton" only, at `factors` (None under L-BFGS)
    jacobian: Optional[np.ndarray] = None          # A [M, G]: d rho / d q, rho the stacked r_k / sqrt|m_k|
    singular_values: Optional[np.ndarray] = None   # of A, descending
    covariance: Optional[np.ndarray] = None        # J / (M - G) (A^T A)^-1 of the log-factors (None when M <= G)
    factor_std: Optional[np.ndarray] = None        # factors * sqrt(diag(covariance))
    stop: Optional[str] = None                     # "misfit" | "gradient" | "step" | "cap" | "damping"


def check_identify(model: FEMModel, config: SolverConfig, levels, groups=None, q0=None):
    """What identification needs, checked before an engine is built; every violation is a ValueError.
    Returns (levels as [(load factor, dofs int64 [m], values float64 [m])] in ascending order of load factor,
    groups int64 [n_elems] or None, q0 float64 [n_parameters])."""
    if _solver.check_kinematics(config.kinematics, config.nr_preconditioner) != "green-lagrange":
        raise ValueError("identification needs kinematics 'green-lagrange': the linear operator has no per-element "
                         "E*A override (its stiffness is the model's own); solve_gd identifies on the linear element.")
    if _solver.check_control(config, model) == "displacement":
        raise ValueError("identification runs under load control only: nr_control 'displacement' is not supported.")
    if _solver.cable_mask(model, getattr(config, "cable_elements", None)) is not None:
        raise ValueError("identification does not support cable_elements: the sensitivities treat every element as a bar.")
    if getattr(config, "yield_strain", None) is not None:
        raise ValueError("identification does not support yield_strain: its Newton solves and sensitivities are elastic "
                         "and would silently answer for the structure that never yields.")
    if model.material.has_trainable_params():
        raise ValueError("identification needs scalar materials (no NN parameters): the base E*A is the model's scalar one.")
    if _solver._world_size() > 1:
        raise ValueError("identification does not support a sharded (multi-GPU) run.")
    levels = list(levels) if levels is not None else []
    if not levels:
        raise ValueError("identification needs at least one load level: levels is empty.")
    free = _solver._free_mask(model)
    out = []
    for k, level in enumerate(levels):
        lam, dofs, u = (level["load_factor"], level["dofs"], level["u"]) if isinstance(level, dict) else level
        lam = float(lam)
        dofs = np.asarray(dofs).reshape(-1)
        u = np.asarray(u, dtype=np.float64).reshape(-1)
        if not np.isfinite(lam):
            raise ValueError(f"level {k}: the load factor is not finite.")
        gauges = isinstance(level, dict) and ("strain_elements" in level or "strains" in level)
        if dofs.size == 0 and not gauges:
            raise ValueError(f"level {k}: no measured dofs (an empty level).")
        if dofs.size != u.size:
            raise ValueError(f"level {k}: mismatched lengths: {dofs.size} measured dofs, {u.size} measured values.")
        if dofs.size and dofs.dtype.kind not in "iu":
            raise ValueError(f"level {k}: measured dofs must be integers.")
        dofs = dofs.astype(np.int64)
        if dofs.size and (dofs.min() < 0 or dofs.max() >= model.ndof):
            raise ValueError(f"level {k}: measured dofs out of range 0..{model.ndof - 1}.")
        if not free[dofs].all():
            raise ValueError(f"level {k}: measured dofs {dofs[~free[dofs]].tolist()} are fixed dofs.")
        if not np.all(np.isfinite(u)):
            raise ValueError(f"level {k}: measured values are not all finite.")
        out.append((lam, dofs, u))
    out.sort(key=lambda lv: lv[0])
    n_params = model.nelm
    if groups is not None:
        g = np.asarray(groups).reshape(-1)
        if g.size != model.nelm:
            raise ValueError(f"the group map has the wrong length: {g.size} entries for {model.nelm} elements.")
        if g.dtype.kind not in "iu":
            raise ValueError("the group map must hold integer group ids.")
        if g.size and g.min() < 0:
            raise ValueError("the group map holds negative group ids.")
        groups = g.astype(np.int64)
        n_params = int(groups.max()) + 1 if groups.size else 0
    q = np.zeros(n_params) if q0 is None else np.asarray(q0, dtype=np.float64).reshape(-1)
    if q.size != n_params:
        raise ValueError(f"q0 has {q.size} entries for {n_params} parameters.")
    if not np.all(np.isfinite(q)):
        raise ValueError("q0 holds non-finite log-factors.")
    return out, groups, q.copy()


def check_strains(model: FEMModel, levels):
    """The strain-gauge data of the levels, checked before an engine is built; every violation is a ValueError.
    A dict level may carry "strain_elements" (element ids [p]), "strains" (the measured Green-Lagrange strains [p],
    e = (l^2 - l0^2) / (2 l0^2); an engineering strain eps is e = eps + eps^2 / 2) and optionally "strain_scale" (a
    length L > 0, default 1.0).  Returns, in check_identify's order (the same stable sort on the load factor), one
    (elements int64 [p], values float64 [p], scale) per level, or None for a level without strain data."""
    out = []
    for k, level in enumerate(list(levels) if levels is not None else []):
        if not isinstance(level, dict):
            if len(level) != 3:
                raise ValueError(f"level {k}: a tuple level is (load factor, dofs, u); only the dict form carries strains.")
            out.append((float(level[0]), None))
            continue
        lam = float(level["load_factor"])
        has_e, has_v = "strain_elements" in level, "strains" in level
        if has_e != has_v:
            raise ValueError(f"level {k}: 'strain_elements' and 'strains' go together: one is given without the other.")
        if not has_e:
            if "strain_scale" in level:
                raise ValueError(f"level {k}: 'strain_scale' without 'strain_elements' and 'strains'.")
            out.append((lam, None))
            continue
        elems = np.asarray(level["strain_elements"]).reshape(-1)
        values = np.asarray(level["strains"], dtype=np.float64).reshape(-1)
        if elems.size != values.size:
            raise ValueError(f"level {k}: mismatched lengths: {elems.size} strain elements, {values.size} strains.")
        if elems.size == 0:
            raise ValueError(f"level {k}: no strain elements (leave both keys out for a level without gauges).")
        if elems.dtype.kind not in "iu":
            raise ValueError(f"level {k}: strain elements must be integers.")
        elems = elems.astype(np.int64)
        if elems.min() < 0 or elems.max() >= model.nelm:
            raise ValueError(f"level {k}: strain elements out of range 0..{model.nelm - 1}.")
        if np.unique(elems).size != elems.size:
            raise ValueError(f"level {k}: a strain element is listed twice.")
        if not np.all(np.isfinite(values)):
            raise ValueError(f"level {k}: strains are not all finite.")
        if np.any(values <= -0.5):
            raise ValueError(f"level {k}: a strain <= -0.5 is no Green-Lagrange strain (e = (l^2 - l0^2) / (2 l0^2) > -1/2).")
        scale = float(level.get("strain_scale", 1.0))
        if not (np.isfinite(scale) and scale > 0.0):
            raise ValueError(f"level {k}: strain_scale must be positive and finite.")
        out.append((lam, (elems, values, scale)))
    out.sort(key=lambda lv: lv[0])
    return [data for _, data in out]


class _Level(NamedTuple):
    """One load level as check_identify and check_strains pass it."""
    load_factor: float
    dofs: np.ndarray                     # int64 [m]
    values: np.ndarray                   # float64 [m]
    gauges: Optional[tuple]              # check_strains' (elements int64 [p], strains float64 [p], scale), or None


def _checked(model, config, levels, groups=None, q0=None):
    """check_identify and check_strains on the levels as they were given.
    Returns ([_Level] in ascending order of load factor, groups, q0)."""
    raw = list(levels) if levels is not None else []
    levels, groups, q = check_identify(model, config, raw, groups, q0)
    return [_Level(*lv, st) for lv, st in zip(levels, check_strains(model, raw))], groups, q


def _check_ea(model, ea) -> np.ndarray:
    """One evaluation's ea as float64 [n_elems] on the host; a wrong length or an entry not finite and positive: ValueError."""
    ea_np = ea.detach().cpu().numpy() if isinstance(ea, torch.Tensor) else np.asarray(ea)
    ea_np = np.ascontiguousarray(ea_np, dtype=np.float64).reshape(-1)
    if ea_np.size != model.nelm:
        raise ValueError(f"ea has {ea_np.size} entries, the model has {model.nelm} elements")
    if not (np.all(np.isfinite(ea_np)) and np.all(ea_np > 0.0)):
        raise ValueError("ea must be finite and positive in every element")
    return ea_np


_COUNTERS = ("newton_iterations", "cg_iterations", "adjoint_cg_iterations")
_GN_COUNTERS = _COUNTERS + ("sensitivity_cg_iterations", "jacobians")


def _add_counters(total, part):
    for key in total:
        total[key] += part[key]


def _strain_residual(eng, e, gauges):
    """(ids on the device, e[ids] - ebar on the device, L, p) of one level's gauges from the element strains e."""
    elems, values, scale = gauges
    ids = torch.from_numpy(elems).to(eng.device)
    return ids, e[ids] - torch.from_numpy(values).to(eng.device), scale, len(elems)


def _base_ea(model) -> float:
    return float(model.material.young.value()) * float(model.material.area.value())


def _newton_level(s, model, config, lam, u, ea_t, counters):
    """One level's Newton loop from u, as an evaluation runs it; no convergence is a RuntimeError."""
    u, ok, residual, _, ite, cg = _solver._newton_loop(s, model, config, lam * s.loads, u, True, ea=ea_t)
    counters["newton_iterations"] += ite + 1
    counters["cg_iterations"] += cg
    if not ok:
        raise RuntimeError(f"Newton-Raphson did not converge at load factor {lam} in {config.max_iterations} "
                           f"iterations (|du|/|u| = {residual:.3e}): no misfit at this point")
    return u


def misfit_and_gradient(model: FEMModel, config: SolverConfig, levels, ea):
    """J and dJ/d ea at the element stiffnesses ea [n_elems] (float64; host or device).

    Per level, in ascending order of load factor, the Green-Lagrange Newton loop of solve_nr with ea in place of the
    model's E*A, started from the previous level's state; then the element state at the converged u, ONE tangent CG
    solve for the adjoint (config.nr_preconditioner / nr_aggregates) and the element sensitivities, accumulated on the
    device.  The adjoint solve is held to solve_nr's rule: g.a > 0, else the same RuntimeError.  A Newton loop that does
    not converge in config.max_iterations is a RuntimeError too.  A level with strain data (check_strains) adds
    L^2 mean (e - ebar)^2 to J and B^T c to the adjoint right-hand side (gl_strain_rhs) before that one solve; the
    sensitivity kernel is the same.
    Returns (J, dJ/d ea [n_elems] on the device, displacements per level [n_dofs] on the device in that order,
    {"newton_iterations", "cg_iterations", "adjoint_cg_iterations"})."""
    config = config or SolverConfig()
    levels, _, _ = _checked(model, config, levels)
    ea_np = _check_ea(model, ea)
    s = _solver._newton_setup(model, _solver.check_initial_strain(config, model))
    return _misfit(s, model, config, levels, torch.from_numpy(ea_np).to(s.eng.device))


def _misfit(s, model, config, levels, ea_t):
    """misfit_and_gradient on checked input: s the solver's _newton_setup, levels [_Level], ea_t _check_ea's on the device."""
    eng, dev, ndof = s.eng, s.eng.device, model.ndof
    _solver._pre_check(s, ea_t)             # solve_nr's rule at the starting state u = 0, with this evaluation's ea
    u = s.u
    J, grad, states = 0.0, None, []
    counters = dict.fromkeys(_COUNTERS, 0)
    for lam, dofs, ubar, gauges in levels:
        u = _newton_level(s, model, config, lam, u, ea_t, counters)
        e = eng.gl_state(u, ea_t, s.e0)
        g = torch.zeros(ndof, dtype=torch.float64, device=dev)
        if len(dofs):
            dofs_t = torch.from_numpy(dofs).to(dev)
            r = u[dofs_t] - torch.from_numpy(ubar).to(dev)
            J += float(torch.mean(r * r))
            g.index_add_(0, dofs_t, r * (2.0 / len(dofs)))
        if gauges is not None:
            ids, r_e, scale, p = _strain_residual(eng, e, gauges)
            J += scale * scale * float(torch.mean(r_e * r_e))
            coef = torch.zeros(model.nelm, dtype=torch.float64, device=dev)
            coef[ids] = r_e * (2.0 * scale * scale / p)
            eng.gl_strain_rhs(u, coef, out=g)
        a, it_a, ok_a, rr, bb = eng.pcg_solve(g, tangent=True, preconditioner=config.nr_preconditioner,
                                              n_aggregates=config.nr_aggregates, u=u)
        _solver._check_cg_step(True, g, a, ok_a, rr, bb, s.free_t)
        counters["adjoint_cg_iterations"] += int(it_a)
        grad = eng.gl_sensitivity(u, a, out=grad, e0=s.e0)
        states.append(u)
    return J, grad, states, counters


def check_gauss_newton(levels, groups, damping, strains=None):
    """What method "gauss-newton" needs on top of check_identify (whose levels and groups these are); every violation
    is a ValueError.  strains: check_strains' list, whose gauges count as measurement rows (None: no strain data).
    Returns (G, M): groups and measurement rows."""
    if groups is None:
        raise ValueError("method 'gauss-newton' needs an element -> group map (groups=None, one factor and so one "
                         "sensitivity solve per element, is not supported); use method 'lbfgs'.")
    n_groups = int(groups.max()) + 1 if groups.size else 0
    empty = np.flatnonzero(np.bincount(groups, minlength=n_groups) == 0)
    if empty.size:
        raise ValueError(f"groups {empty.tolist()} have no element: their factors are not determined.")
    n_rows = sum(len(dofs) for _, dofs, _ in levels)
    if strains is not None:
        n_rows += sum(len(st[0]) for st in strains if st is not None)
    if n_groups > n_rows:
        raise ValueError(f"{n_groups} groups for {n_rows} measurement rows: the least-squares problem is underdetermined.")
    damping = float(damping)
    if not (np.isfinite(damping) and damping > 0.0):
        raise ValueError("damping must be positive and finite.")
    return n_groups, n_rows


def residuals_and_jacobian(model: FEMModel, config: SolverConfig, levels, ea, groups, states=None, jacobian: bool = True):
    """The weighted residuals rho [M] (r_k / sqrt|m_k| stacked over the levels in ascending load factor, so rho.rho is
    misfit_and_gradient's J) at the element stiffnesses ea [n_elems], and their Jacobian A [M, G] with respect to one
    log-factor per group (groups [n_elems]).

    Per level the Newton loop of misfit_and_gradient, started from the previous level's state; states (per level
    [n_dofs], in that order) given: no Newton solves, those are the u_k.  With jacobian, per level: the element state
    at u_k, the G right-hand sides -f_int of every group alone (gl_group_rhs) and their tangent CG solves behind one
    preconditioner setup (pcg_solve_many), each held to solve_nr's rule as the adjoint solve is; the solutions' rows at
    m_k over sqrt|m_k| are the level's rows of A.  A level with strain data (check_strains) appends L (e - ebar) / sqrt p to
    its part of rho and (L / sqrt p) B s_g at its gauges (gl_strain_jvp) to its rows of A.  A group that moves no
    measured dof and no gauge (a zero column) is a RuntimeError.
    Returns (rho, A or None, displacements per level on the device, misfit_and_gradient's counters plus
    "sensitivity_cg_iterations" and "jacobians")."""
    config = config or SolverConfig()
    levels, groups, _ = _checked(model, config, levels, groups)
    if groups is None:
        raise ValueError("residuals_and_jacobian needs an element -> group map")
    ea_np = _check_ea(model, ea)
    s = _solver._newton_setup(model, _solver.check_initial_strain(config, model))
    if states is not None and len(states) != len(levels):
        raise ValueError(f"states has {len(states)} entries for {len(levels)} levels")
    return _residuals(s, model, config, levels, torch.from_numpy(ea_np).to(s.eng.device), groups, states, jacobian)


def _residuals(s, model, config, levels, ea_t, groups, states=None, jacobian=True, prestress=None):
    """residuals_and_jacobian on checked input: s, levels and ea_t as _misfit takes them (s.e0 this evaluation's initial
    strain), groups check_identify's, states None or one per level.  prestress: a prestress group map (fem/prestress.py)
    whose gl_prestress_rhs rows are stacked under the factors' rows, so A = [A_q | A_t]; groups may then be None."""
    eng, dev = s.eng, s.eng.device
    _solver._pre_check(s, ea_t)             # solve_nr's rule at the starting state u = 0, with this evaluation's ea and e0
    counters = dict(dict.fromkeys(_GN_COUNTERS, 0), jacobians=int(bool(jacobian)))
    u = s.u
    rho, rows, out_states = [], [], []
    for k, (lam, dofs, ubar, gauges) in enumerate(levels):
        if states is None:
            u = _newton_level(s, model, config, lam, u, ea_t, counters)
        else:
            u = states[k].to(device=dev, dtype=torch.float64).reshape(-1)
        dofs_t = torch.from_numpy(dofs).to(dev)
        w = 1.0 / np.sqrt(len(dofs)) if len(dofs) else 0.0
        rho.append((u[dofs_t] - torch.from_numpy(ubar).to(dev)).cpu().numpy() * w)
        if jacobian or gauges is not None:
            e = eng.gl_state(u, ea_t, s.e0)
        if gauges is not None:
            _, r_e, scale, p = _strain_residual(eng, e, gauges)
            w_e = scale / np.sqrt(p)
            rho.append(r_e.cpu().numpy() * w_e)
        if jacobian:
            B = None if prestress is None else eng.gl_prestress_rhs(u, ea_t, prestress)
            if groups is not None:
                B = eng.gl_group_rhs(groups) if B is None else torch.cat([eng.gl_group_rhs(groups), B], dim=0)
            S, reports = eng.pcg_solve_many(B, preconditioner=config.nr_preconditioner, n_aggregates=config.nr_aggregates, u=u)
            for g, (it_s, ok_s, rr, bb) in enumerate(reports):
                _solver._check_cg_step(True, B[g], S[g], ok_s, rr, bb, s.free_t)
                counters["sensitivity_cg_iterations"] += int(it_s)
            rows.append(S[:, dofs_t].t().cpu().numpy() * w)
            if gauges is not None:
                rows.append(eng.gl_strain_jvp(u, gauges[0], S).t().cpu().numpy() * w_e)
        out_states.append(u)
    A = None
    if jacobian:
        A = np.concatenate(rows, axis=0)
        dead = np.flatnonzero(~np.any(A != 0.0, axis=0))
        if dead.size:
            c, n_q = int(dead[0]), 0 if groups is None else int(groups.max()) + 1
            name = f"group {c}" if prestress is None else f"stiffness group {c}" if c < n_q else f"prestress group {c - n_q}"
            raise RuntimeError(f"{name} moves no measured dof and no gauge (a zero column of the Jacobian): its "
                               f"{'factor' if prestress is None else 'parameter'} is not determined by these measurements")
    return np.concatenate(rho), A, out_states, counters


def _levenberg_marquardt(evaluate, x_start, describe, max_evaluations, gtol, misfit_tolerance, damping, step_tolerance,
                         reject_errors=True):
    """The Levenberg-Marquardt loop of identify_nr(method="gauss-newton") and identify_prestress, whose docstrings state its
    stops and its mu rule.  evaluate(x, states=None, jacobian=True) returns (rho, A or None, states); describe(x) the
    history's view of x.  reject_errors: a trial point whose evaluation raises RuntimeError is a rejected step (mu <- 10 mu,
    the history entry carries the message under "error" and misfit None); otherwise the error propagates.
    Returns (x, rho, A, states, history, stop, evaluations) of the last accepted point."""
    x = x_start
    rho, A, states = evaluate(x)            # the first evaluation's error propagates
    J, mu, evaluations = float(rho @ rho), float(damping), 1
    history = [{"misfit": J, "gradient_norm": float(np.linalg.norm(2.0 * A.T @ rho)), **describe(x), "accepted": True,
                "damping": mu}]
    while True:
        if J <= misfit_tolerance:
            stop = "misfit"
            break
        if np.max(np.abs(2.0 * A.T @ rho)) <= gtol:
            stop = "gradient"
            break
        if evaluations >= int(max_evaluations):
            stop = "cap"
            break
        H = A.T @ A
        delta = np.linalg.solve(H + mu * np.diag(np.diag(H)), -(A.T @ rho))
        if np.max(np.abs(delta)) <= step_tolerance:
            stop = "step"
            break
        entry = {"misfit": None, "gradient_norm": None, **describe(x + delta), "accepted": False, "damping": mu}
        history.append(entry)
        evaluations += 1
        try:
            rho_t, _, states_t = evaluate(x + delta, jacobian=False)
            J_t = entry["misfit"] = float(rho_t @ rho_t)
        except RuntimeError as exc:
            if not reject_errors:
                raise
            J_t = float("inf")
            entry["error"] = str(exc)
        if J_t < J:
            x, rho, J, states = x + delta, rho_t, J_t, states_t
            _, A, _ = evaluate(x, states=states)                # the Jacobian at the trial's own states: no Newton solves
            entry["accepted"] = True
            entry["gradient_norm"] = float(np.linalg.norm(2.0 * A.T @ rho))
            mu = max(mu / 10.0, 1e-12)
        else:
            mu *= 10.0
            if mu > 1e12:
                stop = "damping"
                break
    return x, rho, A, states, history, stop, evaluations


def _gauss_newton(s, model, config, levels, groups, q_start, ea_of, max_evaluations, gtol, misfit_tolerance, damping,
                  step_tolerance):
    """_levenberg_marquardt on the log-factors (identify_nr, method "gauss-newton"); s, levels, groups as _residuals' are.  A
    trial's error propagates.  Returns (q, rho, A, states, history, counters, stop, evaluations)."""
    counters = dict.fromkeys(_GN_COUNTERS, 0)

    def evaluate(q_np, **kw):
        ea_t = torch.from_numpy(_check_ea(model, ea_of(q_np))).to(s.eng.device)
        out = _residuals(s, model, config, levels, ea_t, groups, **kw)
        _add_counters(counters, out[3])
        return out[:3]

    q, rho, A, states, history, stop, evaluations = _levenberg_marquardt(
        evaluate, q_start, lambda q: {"factors": np.exp(q)}, max_evaluations, gtol, misfit_tolerance, damping, step_tolerance,
        reject_errors=False)
    return q, rho, A, states, history, counters, stop, evaluations


class _Stop(Exception):
    pass


def _reactions(s, model, lam, u, ea_t):
    """Reactions of a level at its state: f_int(u; ea, e0) - lam f on the fixed dofs."""
    s.eng.gl_state(u, ea_t, s.e0)
    reactions = s.eng.gl_fint().cpu().numpy() - lam * np.asarray(model.loads, dtype=float).reshape(-1)
    reactions[s.free] = 0.0
    return reactions


def identify_nr(model: FEMModel, config: Optional[SolverConfig], levels, groups=None, q0=None, max_evaluations: int = 200,
                gtol: float = 1e-12, misfit_tolerance: float = 0.0, history_size: int = 10,
                tolerance_change: float = 1e-18, method: str = "lbfgs", damping: float = 1e-3,
                step_tolerance: float = 1e-12) -> IdentifyResult:
    """Factors on the model's scalar E*A, one per group of elements, that make the Green-Lagrange Newton solve match
    the measured displacements of `levels` ([{"load_factor", "dofs", "u"}] or tuples in that order).  A dict level may
    also carry strain-gauge data: "strain_elements" (element ids), "strains" (the measured GREEN-LAGRANGE strains
    e = (l^2 - l0^2) / (2 l0^2), what pf_gl_state writes; an engineering strain eps converts as e = eps + eps^2 / 2) and
    "strain_scale" (a length L > 0, default 1.0; the level adds L^2 mean (e - ebar)^2 to the misfit).  Such a level may
    have empty "dofs".  Both methods take strain data; the result then carries `strains`, every element's strain per level.

    torch.optim.LBFGS with the strong-Wolfe line search on float64 log-factors q on the host, from q0 (None: zeros, every
    factor 1); each evaluation is one misfit_and_gradient and one group_sum.  groups: the group id of every element
    [n_elems]; None: one parameter per element (the gradient is then dJ/d ea * ea and the group kernel is skipped).
    It stops when max |dJ/dq| <= gtol, when J <= misfit_tolerance, when L-BFGS can no longer change q
    (tolerance_change) or after max_evaluations evaluations (converged False), and returns the evaluated point with the
    smallest misfit.  A trial point whose Newton solve raises (a limit point, no convergence) propagates the error.

    method "gauss-newton": Levenberg-Marquardt on the same log-factors with the Jacobian A of residuals_and_jacobian
    (groups is required, every group needs an element and there must be at least as many measurement rows M as groups
    G).  From q0 with mu = damping, repeat: stop "misfit" if J <= misfit_tolerance, "gradient" if max |2 A^T rho| <= gtol,
    "cap" at max_evaluations; delta solves (H + mu diag H) delta = -A^T rho with H = A^T A; stop "step" if max |delta| <=
    step_tolerance; evaluate rho at q + delta without a Jacobian (one evaluation); if that lowers J accept it, form A
    at the trial's own states (no Newton solves, not an evaluation) and mu <- max(mu / 10, 1e-12); otherwise mu <- 10 mu
    and stop "damping" once mu > 1e12.  converged is True for "misfit", "gradient" and "step"; the returned point is the
    last accepted one.  The result then carries jacobian, singular_values, covariance = J / (M - G) (A^T A)^-1 of the
    log-factors, factor_std = factors * sqrt(diag covariance) and stop; history entries carry "accepted" and "damping"
    (a trial that was not accepted has gradient_norm None).  The covariance is that of the WEIGHTED fit (every level's
    residuals over sqrt|m_k|): it is the covariance of the log-factors for equal noise on all measurements and equal
    level sizes, and first-order otherwise."""
    if method not in ("lbfgs", "gauss-newton"):
        raise ValueError(f"unknown identification method {method!r}: 'lbfgs' or 'gauss-newton'.")
    config = config or SolverConfig()
    levels, groups, q_start = _checked(model, config, levels, groups, q0)
    if int(max_evaluations) < 1:
        raise ValueError("max_evaluations must be at least 1")
    if method == "gauss-newton":
        n_groups, n_rows = check_gauss_newton([lv[:3] for lv in levels], groups, damping, [lv.gauges for lv in levels])
    have_gauges = any(lv.gauges is not None for lv in levels)
    lam_last = levels[-1].load_factor
    ea0 = _base_ea(model)
    s = _solver._newton_setup(model, _solver.check_initial_strain(config, model))
    eng = s.eng

    def ea_of(q_np):
        f = np.exp(q_np)
        return ea0 * (f if groups is None else f[groups])

    def strains_at(states, ea_t):
        """Every element's strain per level at the returned point (None without strain data)."""
        return [eng.gl_state(u, ea_t, s.e0).cpu().numpy() for u in states] if have_gauges else None
    if method == "gauss-newton":
        q, rho, A, states, history, counters, stop, evaluations = _gauss_newton(
            s, model, config, levels, groups, q_start, ea_of, max_evaluations, gtol, misfit_tolerance, damping,
            step_tolerance)
        J = float(rho @ rho)
        covariance = J / (n_rows - n_groups) * np.linalg.inv(A.T @ A) if n_rows > n_groups else None
        ea_t = torch.from_numpy(ea_of(q)).to(eng.device)
        return IdentifyResult(
            factors=np.exp(q), ea=ea_of(q), misfit=J, gradient=2.0 * A.T @ rho, evaluations=evaluations,
            converged=stop in ("misfit", "gradient", "step"), history=history,
            displacements=[u.cpu().numpy() for u in states], counters=counters, strains=strains_at(states, ea_t),
            reactions=_reactions(s, model, lam_last, states[-1], ea_t), jacobian=A,
            singular_values=np.linalg.svd(A, compute_uv=False), covariance=covariance,
            factor_std=None if covariance is None else np.exp(q) * np.sqrt(np.diag(covariance)), stop=stop)
    counters = dict.fromkeys(_COUNTERS, 0)
    history, best = [], {}
    q = torch.from_numpy(q_start).requires_grad_(True)
    opt = torch.optim.LBFGS([q], lr=1, max_iter=int(max_evaluations), max_eval=int(max_evaluations),
                            history_size=int(history_size), line_search_fn="strong_wolfe", tolerance_grad=float(gtol),
                            tolerance_change=float(tolerance_change))

    def closure():
        if len(history) >= int(max_evaluations):
            raise _Stop
        opt.zero_grad()
        q_np = q.detach().numpy().copy()
        ea_t = torch.from_numpy(_check_ea(model, ea_of(q_np))).to(eng.device)
        J, g_ea, states, c = _misfit(s, model, config, levels, ea_t)
        gq = (g_ea * ea_t) if groups is None else eng.group_sum(g_ea, ea_t, groups)
        gq = gq.cpu()
        _add_counters(counters, c)
        history.append({"misfit": J, "gradient_norm": float(torch.linalg.norm(gq)), "factors": np.exp(q_np)})
        if not best or J < best["J"]:
            best.update(J=J, q=q_np, g=gq.numpy().copy(), states=states, ea=ea_t)
        q.grad = gq
        if J <= misfit_tolerance:
            raise _Stop
        return torch.tensor(J, dtype=torch.float64)

    try:
        opt.step(closure)
    except _Stop:
        pass
    met = bool(np.max(np.abs(best["g"]), initial=0.0) <= gtol or best["J"] <= misfit_tolerance)
    converged = met or len(history) < int(max_evaluations)          # False: the evaluation cap ended it
    reactions = _reactions(s, model, lam_last, best["states"][-1], best["ea"])
    return IdentifyResult(factors=np.exp(best["q"]), ea=ea_of(best["q"]), misfit=float(best["J"]), gradient=best["g"],
                          evaluations=len(history), converged=converged, history=history,
                          displacements=[u.cpu().numpy() for u in best["states"]], counters=counters, reactions=reactions,
                          strains=strains_at(best["states"], best["ea"]))
