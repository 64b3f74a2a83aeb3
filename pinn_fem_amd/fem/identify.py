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

Limits: states with a positive definite tangent only (the CG solves), load control only, a scalar base material, no
regularisation term and no bounds on the factors.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional

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


def _level_parts(level):
    if isinstance(level, dict):
        return level["load_factor"], level["dofs"], level["u"]
    lam, dofs, u = level
    return lam, dofs, u


def check_identify(model: FEMModel, config: SolverConfig, levels, groups=None, q0=None):
    """What identification needs, checked before an engine is built; every violation is a ValueError.
    Returns (levels as [(load factor, dofs int64 [m], values float64 [m])] in ascending order of load factor,
    groups int64 [n_elems] or None, q0 float64 [n_parameters])."""
    if _solver.check_kinematics(config.kinematics, config.nr_preconditioner) != "green-lagrange":
        raise ValueError("identification needs kinematics 'green-lagrange': the linear operator has no per-element "
                         "E*A override (its stiffness is the model's own); solve_gd identifies on the linear element.")
    if _solver.check_control(config, model) == "displacement":
        raise ValueError("identification runs under load control only: nr_control 'displacement' is not supported.")
    if model.material.has_trainable_params():
        raise ValueError("identification needs scalar materials (no NN parameters): the base E*A is the model's scalar one.")
    if _solver._world_size() > 1:
        raise ValueError("identification does not support a sharded (multi-GPU) run.")
    levels = list(levels) if levels is not None else []
    if not levels:
        raise ValueError("identification needs at least one load level: levels is empty.")
    free = np.ones(model.ndof, dtype=bool)
    free[np.asarray(model.fixed_dofs, dtype=int)] = False
    out = []
    for k, level in enumerate(levels):
        lam, dofs, u = _level_parts(level)
        lam = float(lam)
        dofs = np.asarray(dofs).reshape(-1)
        u = np.asarray(u, dtype=np.float64).reshape(-1)
        if not np.isfinite(lam):
            raise ValueError(f"level {k}: the load factor is not finite.")
        if dofs.size == 0:
            raise ValueError(f"level {k}: no measured dofs (an empty level).")
        if dofs.size != u.size:
            raise ValueError(f"level {k}: mismatched lengths: {dofs.size} measured dofs, {u.size} measured values.")
        if dofs.dtype.kind not in "iu":
            raise ValueError(f"level {k}: measured dofs must be integers.")
        dofs = dofs.astype(np.int64)
        if dofs.min() < 0 or dofs.max() >= model.ndof:
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


def _base_ea(model) -> float:
    return float(model.material.young.value()) * float(model.material.area.value())


def misfit_and_gradient(model: FEMModel, config: SolverConfig, levels, ea):
    """J and dJ/d ea at the element stiffnesses ea [n_elems] (float64; host or device).

    Per level, in ascending order of load factor, the Green-Lagrange Newton loop of solve_nr with ea in place of the
    model's E*A, started from the previous level's state; then the element state at the converged u, ONE tangent CG
    solve for the adjoint (config.nr_preconditioner / nr_aggregates) and the element sensitivities, accumulated on the
    device.  The adjoint solve is held to solve_nr's rule: g.a > 0, else the same RuntimeError.  A Newton loop that does
    not converge in config.max_iterations is a RuntimeError too.
    Returns (J, dJ/d ea [n_elems] on the device, displacements per level [n_dofs] on the device in that order,
    {"newton_iterations", "cg_iterations", "adjoint_cg_iterations"})."""
    config = config or SolverConfig()
    levels, _, _ = check_identify(model, config, levels)
    ea_np = ea.detach().cpu().numpy() if isinstance(ea, torch.Tensor) else np.asarray(ea)
    ea_np = np.asarray(ea_np, dtype=np.float64).reshape(-1)
    if ea_np.size != model.nelm:
        raise ValueError(f"ea has {ea_np.size} entries, the model has {model.nelm} elements")
    if not (np.all(np.isfinite(ea_np)) and np.all(ea_np > 0.0)):
        raise ValueError("ea must be finite and positive in every element")
    eng = _solver._engine_for(model, None, None)
    dev, ndof = eng.device, model.ndof
    ea_t = ea.to(device=dev, dtype=torch.float64).reshape(-1) if isinstance(ea, torch.Tensor) else torch.from_numpy(ea_np).to(dev)
    free = np.ones(ndof, dtype=bool)
    free[np.asarray(model.fixed_dofs, dtype=int)] = False
    if bool((eng.diag_k().cpu().numpy()[free] == 0.0).any()):
        raise RuntimeError("Tangent stiffness became singular during solve")
    free_t = torch.from_numpy(free).to(dev)
    loads = torch.from_numpy(np.ascontiguousarray(np.asarray(model.loads, dtype=float).reshape(-1))).to(dev)
    u = torch.zeros(ndof, dtype=torch.float64, device=dev)
    J, grad, states = 0.0, None, []
    counters = {"newton_iterations": 0, "cg_iterations": 0, "adjoint_cg_iterations": 0}
    for lam, dofs, ubar in levels:
        u, ok, residual, _, ite, cg = _solver._newton_loop(eng, model, config, lam * loads, u, free_t, True, ea=ea_t)
        counters["newton_iterations"] += ite + 1
        counters["cg_iterations"] += cg
        if not ok:
            raise RuntimeError(f"Newton-Raphson did not converge at load factor {lam} in {config.max_iterations} "
                               f"iterations (|du|/|u| = {residual:.3e}): no misfit at this point")
        eng.gl_state(u, ea_t)
        dofs_t = torch.from_numpy(dofs).to(dev)
        r = u[dofs_t] - torch.from_numpy(ubar).to(dev)
        J += float(torch.mean(r * r))
        g = torch.zeros(ndof, dtype=torch.float64, device=dev)
        g.index_add_(0, dofs_t, r * (2.0 / len(dofs)))
        a, it_a, ok_a, rr, bb = eng.pcg_solve(g, tangent=True, preconditioner=config.nr_preconditioner,
                                              n_aggregates=config.nr_aggregates, u=u)
        _solver._check_cg_step(True, g, a, ok_a, rr, bb, free_t)
        counters["adjoint_cg_iterations"] += int(it_a)
        grad = eng.gl_sensitivity(u, a, out=grad)
        states.append(u)
    return J, grad, states, counters


class _Stop(Exception):
    pass


def identify_nr(model: FEMModel, config: Optional[SolverConfig], levels, groups=None, q0=None, max_evaluations: int = 200,
                gtol: float = 1e-12, misfit_tolerance: float = 0.0, history_size: int = 10,
                tolerance_change: float = 1e-18) -> IdentifyResult:
    """Factors on the model's scalar E*A, one per group of elements, that make the Green-Lagrange Newton solve match
    the measured displacements of `levels` ([{"load_factor", "dofs", "u"}] or tuples in that order).

    torch.optim.LBFGS with the strong-Wolfe line search on float64 log-factors q on the host, from q0 (None: zeros, every
    factor 1); each evaluation is one misfit_and_gradient and one group_sum.  groups: the group id of every element
    [n_elems]; None: one parameter per element (the gradient is then dJ/d ea * ea and the group kernel is skipped).
    It stops when max |dJ/dq| <= gtol, when J <= misfit_tolerance, when L-BFGS can no longer change q
    (tolerance_change) or after max_evaluations evaluations (converged False), and returns the evaluated point with the
    smallest misfit.  A trial point whose Newton solve raises (a limit point, no convergence) propagates the error."""
    config = config or SolverConfig()
    levels, groups, q_start = check_identify(model, config, levels, groups, q0)
    if int(max_evaluations) < 1:
        raise ValueError("max_evaluations must be at least 1")
    ea0 = _base_ea(model)
    eng = _solver._engine_for(model, None, None)
    counters = {"newton_iterations": 0, "cg_iterations": 0, "adjoint_cg_iterations": 0}
    history, best = [], {}

    def ea_of(q_np):
        f = np.exp(q_np)
        return ea0 * (f if groups is None else f[groups])

    q = torch.from_numpy(q_start).requires_grad_(True)
    opt = torch.optim.LBFGS([q], lr=1, max_iter=int(max_evaluations), max_eval=int(max_evaluations),
                            history_size=int(history_size), line_search_fn="strong_wolfe", tolerance_grad=float(gtol),
                            tolerance_change=float(tolerance_change))

    def closure():
        if len(history) >= int(max_evaluations):
            raise _Stop
        opt.zero_grad()
        q_np = q.detach().numpy().copy()
        ea_t = torch.from_numpy(ea_of(q_np)).to(eng.device)
        J, g_ea, states, c = misfit_and_gradient(model, config, levels, ea_t)
        gq = (g_ea * ea_t) if groups is None else eng.group_sum(g_ea, ea_t, groups)
        gq = gq.cpu()
        for key in counters:
            counters[key] += c[key]
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
    # reactions of the last level at the returned point: f_int(u; ea) - lam f on the fixed dofs
    lam_last = levels[-1][0]
    eng.gl_state(best["states"][-1], best["ea"])
    reactions = eng.gl_fint().cpu().numpy() - lam_last * np.asarray(model.loads, dtype=float).reshape(-1)
    free = np.ones(model.ndof, dtype=bool)
    free[np.asarray(model.fixed_dofs, dtype=int)] = False
    reactions[free] = 0.0
    return IdentifyResult(factors=np.exp(best["q"]), ea=ea_of(best["q"]), misfit=float(best["J"]), gradient=best["g"],
                          evaluations=len(history), converged=converged, history=history,
                          displacements=[s.cpu().numpy() for s in best["states"]], counters=counters, reactions=reactions)
