"""Unified solver — drop-in for the GD path of the reference's FEM/python/fem/solver.py.

Same names, signatures, dataclass fields, history keys and control flow:
  SolverConfig (:35-62), SolverResult (:65-75), solve_gd (:83-400), solve_hybrid (:520-692),
  solve (:1045-1167).
What changed is the body of the GD iteration (:254-355): instead of a Python loop over elements with
batch-1 MLP calls, 20 indexed `+=` per element into a dense K, autograd and two torch.optim.Adam
steps, each iteration is a fixed sequence of HIP kernels (pf_gd_iterations) working on device-
resident state; the stop test runs on the device, so the host only polls a 64-byte state record
every `check_every` iterations and the final state equals the reference's `break`.

solve_nr (:408-512, classical Newton-Raphson for scalar materials) runs on the
device too: matrix-free float64 K v and a Jacobi-preconditioned CG solve replace the dense
np.linalg.solve, which also gives the scalar branch of solve_hybrid its real GD -> NR switch (:653-692).
Out of scope: solve_full_nr (:753-1037, non-functional in the reference); calling it
raises NotImplementedError.
"""
from __future__ import annotations

import copy
import os
import warnings
from dataclasses import dataclass, field
from typing import Dict, List, NamedTuple, Optional

import numpy as np
import torch

from .boundary import free_and_fixed_dofs
from .model import FEMModel
from ..engine import HipEngine


@dataclass
class SolverConfig:
    """Unified configuration for all solvers (solver.py:35-62)."""
    max_iterations: int = 1000
    tolerance: float = 1e-6
    print_every: int = 10
    n_increments: int = 10
    load_factor_initial: float = 0.0
    load_factor_final: float = 1.0
    min_denominator: float = 1e-10
    learning_rate_u: float = 1e-7
    learning_rate_theta: float = 1e-4
    alpha_physics: float = 1.0
    alpha_data: float = 100.0
    method: str = "auto"
    preconditioning: bool = False
    # preconditioner of the CG solve inside solve_nr: "jacobi" (diag(K_ff)), "two-level" (Jacobi plus a coarse space
    # of per-aggregate rigid-body modes, pinn_fem_amd/coarse.py; linear kinematics) or "two-level-updated" (the same on the
    # Green-Lagrange tangent, rebuilt on the current configuration at every Newton iteration); nr_aggregates: number of
    # aggregates (None: default)
    nr_preconditioner: str = "jacobi"
    nr_aggregates: Optional[int] = None
    # kinematics of solve_nr: "linear" (small displacements, the reference's element) or "green-lagrange" (total-Lagrangian
    # truss element for large displacements: the tangent depends on u and the Newton loop really iterates)
    kinematics: str = "linear"
    # what solve_nr prescribes: "load" (the load factor; the default) or "displacement" (Green-Lagrange only: the global
    # dof nr_control_dof is held at factor * nr_control_displacement and the load factor is solved for, which carries the
    # solve through a limit point of the load)
    nr_control: str = "load"
    nr_control_dof: Optional[int] = None
    nr_control_displacement: float = 0.0
    # initial (eigen-) strain of the Green-Lagrange elements of solve_nr: None, one value for every element or n_elems
    # values, a Green-Lagrange strain e0 with N = E*A (e - e0).  e0 < 0 is a pretension (T = -E*A e0), thermal loading is
    # e0 = alpha dT, lack of fit e0 = (L_natural - l0) / l0.  It acts in full at every load factor
    initial_strain: Optional[object] = None
    # the tension-only (cable) elements of the Green-Lagrange solve_nr: None, "all" or a list of element ids (cable_mask).
    # A flagged element with e - e0 < 0 is slack and carries nothing; the Newton loop iterates on the slack set
    # (_newton_loop).  solve_dynamic takes its cables from here when DynamicsConfig.cable_elements is not given
    cable_elements: Optional[object] = None
    # elastoplastic elements of the Green-Lagrange solve_nr (check_plasticity): yield_strain is sigma_y / E,
    # None (elastic, the default), one number or n_elems of them, inf = that element never yields; hardening_ratio is
    # H / E >= 0 (linear isotropic hardening), a number or n_elems of them
    yield_strain: Optional[object] = None
    hardening_ratio: object = 0.0
    # the load factors solve() walks with method "nr", one Newton solve each, in place of the linear ramp of n_increments
    # steps: a load program that may unload, reverse and reload.  None: the ramp
    load_factors: Optional[object] = None


KINEMATICS = ("linear", "green-lagrange")
NR_CONTROLS = ("load", "displacement")


def check_kinematics(name, nr_preconditioner: str = "jacobi") -> str:
    """The kinematics name, checked, and its combination with the CG preconditioner of solve_nr."""
    from ..coarse import check_preconditioner
    if name not in KINEMATICS:
        raise ValueError(f"unknown kinematics {name!r}: accepted values are 'linear' and 'green-lagrange'")
    pre = check_preconditioner(nr_preconditioner)
    if name == "green-lagrange" and pre == "two-level":
        raise ValueError("kinematics 'green-lagrange' supports nr_preconditioner 'jacobi' and 'two-level-updated': "
                         "'two-level' keeps the coarse space of the reference configuration, which is not the tangent's.")
    if name == "linear" and pre == "two-level-updated":
        raise ValueError("nr_preconditioner 'two-level-updated' belongs to kinematics 'green-lagrange': the linear "
                         "stiffness does not change, so there is nothing to update; use 'two-level'.")
    return name


def check_control(config, model=None, method: str = "nr") -> str:
    """The control name of solve_nr, checked.  Displacement control needs the Green-Lagrange kinematics, the Newton solve
    and, when a model is given, scalar materials, one GPU, a free control dof, a non-zero control displacement and loads
    that are not all zero on the free dofs: every violation is a ValueError before an engine is built."""
    name = getattr(config, "nr_control", "load")
    if name not in NR_CONTROLS:
        raise ValueError(f"unknown nr_control {name!r}: accepted values are 'load' and 'displacement'")
    if name == "load":
        return name
    if method != "nr":
        raise ValueError(f"nr_control 'displacement' belongs to the Newton-Raphson solve (solve_nr, method 'nr'): "
                         f"method {method!r} does not support it.")
    if config.kinematics != "green-lagrange":
        raise ValueError("nr_control 'displacement' needs kinematics 'green-lagrange': the linear solve has no limit "
                         "point to pass.")
    if model is None:
        return name
    if model.material.has_trainable_params():
        raise ValueError("nr_control 'displacement' needs scalar materials (no NN parameters).")
    if _world_size() > 1:
        raise ValueError("nr_control 'displacement' does not support a sharded (multi-GPU) run.")
    c = config.nr_control_dof
    if c is None or isinstance(c, bool) or int(c) != c or not 0 <= int(c) < model.ndof:
        raise ValueError(f"nr_control 'displacement' needs nr_control_dof, a global dof in 0..{model.ndof - 1}: got {c!r}")
    free = _free_mask(model)
    if not free[int(c)]:
        raise ValueError(f"nr_control_dof {int(c)} is a fixed dof: the control dof must be free.")
    d = float(config.nr_control_displacement)
    if not np.isfinite(d) or d == 0.0:
        raise ValueError("nr_control 'displacement' needs a non-zero nr_control_displacement (the control dof's value at "
                         "factor 1).")
    if not np.any(np.asarray(model.loads, dtype=float).reshape(-1)[free] != 0.0):
        raise ValueError("nr_control 'displacement' needs loads that are not all zero on the free dofs: the load factor "
                         "is the unknown.")
    return name


def check_initial_strain(config, model):
    """config.initial_strain as a float64 array [n_elems], or None when it is not given.  It belongs to the Green-Lagrange
    Newton solve: linear kinematics, a wrong length, a non-finite value or one of magnitude >= 0.5 (no eigenstrain; 1 + 2 e
    must stay positive) is a ValueError before an engine is built."""
    e0 = getattr(config, "initial_strain", None)
    if e0 is None:
        return None
    if config.kinematics != "green-lagrange":
        raise ValueError("initial_strain needs kinematics 'green-lagrange': solve_gd and the linear solve_nr are untouched "
                         "by it and would silently solve the unstrained structure.")
    try:
        arr = np.asarray(e0, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"initial_strain must be a number or {model.nelm} numbers (one for each element)") from None
    if arr.ndim == 0:
        arr = np.full(model.nelm, float(arr))
    arr = np.ascontiguousarray(arr.reshape(-1))
    if arr.size != model.nelm:
        raise ValueError(f"initial_strain has {arr.size} entries, the model has {model.nelm} elements")
    if not np.all(np.isfinite(arr)):
        raise ValueError("initial_strain holds non-finite values")
    if arr.size and float(np.max(np.abs(arr))) >= 0.5:
        raise ValueError("initial_strain must be smaller than 0.5 in magnitude: it is a small Green-Lagrange eigenstrain, "
                         f"got max |e0| = {float(np.max(np.abs(arr))):g}")
    return arr


def cable_mask(model, cable_elements) -> Optional[np.ndarray]:
    """SolverConfig.cable_elements / DynamicsConfig.cable_elements as a bool [n_elems], or None where nothing is flagged
    (None, an empty list).  Anything else than "all" or a list of distinct element ids is a ValueError."""
    ne = int(model.nelm)
    if cable_elements is None:
        return None
    if isinstance(cable_elements, str):
        if cable_elements != "all":
            raise ValueError(f'cable_elements must be "all" or a list of element ids, got {cable_elements!r}')
        return np.ones(ne, dtype=bool) if ne else None
    try:
        ids = np.asarray(cable_elements)
    except (TypeError, ValueError):
        raise ValueError('cable_elements must be "all" or a list of element ids') from None
    if ids.ndim != 1 or (ids.size and (ids.dtype.kind not in "iu")):
        raise ValueError(f"cable_elements must be a list of integer element ids in 0..{ne - 1}")
    if ids.size == 0:
        return None
    if ids.min() < 0 or ids.max() >= ne:
        raise ValueError(f"cable_elements must be element ids in 0..{ne - 1}, got {int(ids.min())}..{int(ids.max())}")
    if np.unique(ids).size != ids.size:
        raise ValueError("cable_elements names an element twice")
    mask = np.zeros(ne, dtype=bool)
    mask[ids.astype(np.int64)] = True
    return mask


def check_cables(config, model, method: str = "nr"):
    """config.cable_elements as cable_mask's bool [n_elems], or None when nothing is flagged.  Cables belong to the
    Green-Lagrange Newton solve under load control, with scalar materials on one GPU: everything else is a ValueError
    before an engine is built."""
    cable = cable_mask(model, getattr(config, "cable_elements", None))
    if cable is None:
        return None
    if config.kinematics != "green-lagrange":
        raise ValueError("cable_elements needs kinematics 'green-lagrange': solve_gd and the linear solve_nr know no "
                         "tension-only element and would silently solve the structure of bars.")
    if method not in ("nr", "hybrid"):
        raise ValueError(f"cable_elements belongs to the Green-Lagrange Newton solve (solve_nr): method {method!r} is "
                         "untouched by it.")
    if getattr(config, "nr_control", "load") == "displacement":
        raise ValueError("cable_elements does not support nr_control 'displacement': there is no displacement control "
                         "with cables; use load control (solve()'s increments) or solve_dynamic.")
    if model.material.has_trainable_params():
        raise ValueError("cable_elements needs scalar materials (no NN parameters).")
    if _world_size() > 1:
        raise ValueError("cable_elements does not support a sharded (multi-GPU) run.")
    return cable


def _per_element(value, ne, name):
    """A number or ne numbers as a float64 array [ne]; anything else is a ValueError."""
    try:
        arr = np.asarray(value, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a number or {ne} numbers (one for each element)") from None
    if arr.ndim == 0:
        arr = np.full(ne, float(arr))
    arr = np.ascontiguousarray(arr.reshape(-1))
    if arr.size != ne:
        raise ValueError(f"{name} has {arr.size} entries, the model has {ne} elements")
    return arr


def check_plasticity(config, model, method: str = "nr"):
    """(yield strain, hardening ratio) as float64 arrays [n_elems] each, or None where config.yield_strain is None.
    Plasticity belongs to the Green-Lagrange Newton solve under load control, on bars, with scalar materials on one GPU:
    linear kinematics, another method than 'nr' / 'hybrid', nr_control 'displacement', cable_elements, NN materials, a
    sharded run, a wrong length, a yield strain that is not > 0 (inf is the elastic element) and a hardening ratio that is
    negative or not finite are each a ValueError before an engine is built.  initial_strain is supported."""
    if getattr(config, "yield_strain", None) is None:
        return None
    if config.kinematics != "green-lagrange":
        raise ValueError("yield_strain needs kinematics 'green-lagrange': solve_gd and the linear solve_nr know no "
                         "plasticity and would silently solve the elastic structure.")
    if method not in ("nr", "hybrid"):
        raise ValueError(f"yield_strain belongs to the Green-Lagrange Newton solve (solve_nr): method {method!r} is "
                         "untouched by it.")
    if getattr(config, "nr_control", "load") == "displacement":
        raise ValueError("yield_strain does not support nr_control 'displacement': there is no displacement control "
                         "with plasticity; use load control (solve()'s increments or load_factors).")
    if cable_mask(model, getattr(config, "cable_elements", None)) is not None:
        raise ValueError("yield_strain does not support cable_elements: an element is elastoplastic or tension-only, "
                         "not both.")
    if model.material.has_trainable_params():
        raise ValueError("yield_strain needs scalar materials (no NN parameters).")
    if _world_size() > 1:
        raise ValueError("yield_strain does not support a sharded (multi-GPU) run.")
    ey = _per_element(config.yield_strain, model.nelm, "yield_strain")
    kappa = _per_element(getattr(config, "hardening_ratio", 0.0), model.nelm, "hardening_ratio")
    if not np.all(ey > 0.0):                                # (NaN fails the comparison too)
        raise ValueError("yield_strain must be positive (sigma_y / E; inf: the element never yields)")
    if not np.all(np.isfinite(kappa) & (kappa >= 0.0)):
        raise ValueError("hardening_ratio must be finite and not negative (H / E; 0: perfect plasticity)")
    return ey, kappa


def check_plastic_state(plastic_state, ne):
    """solve_nr's plastic_state as (ep, alpha), float64 [ne] each: a pair of the right length, finite, alpha >= 0."""
    try:
        ep, alpha = plastic_state
        ep, alpha = (np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1)) for v in (ep, alpha))
    except (TypeError, ValueError):
        raise ValueError("plastic_state must be a pair (ep, alpha) of arrays, one value for each element") from None
    if ep.size != ne or alpha.size != ne:
        raise ValueError(f"plastic_state has {ep.size} and {alpha.size} entries, the model has {ne} elements")
    if not (np.all(np.isfinite(ep)) and np.all(np.isfinite(alpha))):
        raise ValueError("plastic_state holds non-finite values")
    if np.any(alpha < 0.0):
        raise ValueError("plastic_state: the accumulated plastic strain alpha must not be negative")
    return ep, alpha


def check_load_factors(config, method: str = "nr"):
    """config.load_factors as a list of floats, or None when it is not given.  It belongs to solve() with method 'nr'
    under load control; an empty or non-finite sequence is a ValueError."""
    lf = getattr(config, "load_factors", None)
    if lf is None:
        return None
    if method != "nr":
        raise ValueError(f"load_factors belongs to solve() with method 'nr': method {method!r} walks the linear ramp.")
    if getattr(config, "nr_control", "load") == "displacement":
        raise ValueError("load_factors does not support nr_control 'displacement': the factors are load factors.")
    try:
        arr = np.asarray(lf, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("load_factors must be a sequence of numbers") from None
    if arr.ndim != 1 or arr.size == 0 or not np.all(np.isfinite(arr)):
        raise ValueError("load_factors must be a non-empty sequence of finite numbers")
    return [float(v) for v in arr]


def _axial_forces(model, strain, e0):
    """N = E*A (e - e0) of every element on the host, from the strains a gl_state returned; E*A is the model's scalar one
    as the device forms it (each factor rounded to float32 first)."""
    ea = float(np.float32(model.material.young.value())) * float(np.float32(model.material.area.value()))
    return ea * (strain.cpu().numpy() - e0)


def _free_mask(model) -> np.ndarray:
    """True on the free dofs of the model, False on model.fixed_dofs (bool [n_dofs], host)."""
    mask = np.zeros(model.ndof, dtype=bool)
    mask[free_and_fixed_dofs(model.ndof, model.fixed_dofs)[0]] = True
    return mask


@dataclass
class SolverResult:
    """Unified result from any solver (solver.py:65-75)."""
    displacements: np.ndarray
    reactions: np.ndarray
    converged: bool
    history: List[Dict[str, float]] = field(default_factory=list)
    nn_parameters: Optional[Dict[str, np.ndarray]] = None
    # displacement control (solve() with nr_control = "displacement"): one {control_displacement, load_factor,
    # iterations} per increment, the equilibrium path; None otherwise
    path: Optional[list] = None
    # Green-Lagrange solve_nr with config.cable_elements: bool [n_elems], the slack elements at the final state; None
    # without cables
    slack: Optional[np.ndarray] = None
    # Green-Lagrange solve_nr with config.yield_strain: the committed plastic strain and accumulated plastic strain of
    # every element at the final state (the pair the next increment takes as plastic_state), the elements that yielded in
    # this increment (bool); None without plasticity
    plastic_strain: Optional[np.ndarray] = None
    accumulated_plastic_strain: Optional[np.ndarray] = None
    yielding: Optional[np.ndarray] = None
    # solve() with config.load_factors or config.yield_strain: one {load_factor, iterations, yielding_elements} per
    # increment (yielding_elements is 0.0 without plasticity); None otherwise
    load_path: Optional[list] = None
    # Green-Lagrange solve_nr with config.initial_strain or config.cable_elements: N = E*A (e - e0) of every element at
    # the final state, 0.0 in a slack cable; with config.yield_strain N = E*A (e - e0 - ep); None otherwise
    axial_forces: Optional[np.ndarray] = None


# host polls the device state every CHECK_EVERY iterations (launches after the stop are no-ops)
CHECK_EVERY = int(os.environ.get("PINNFEM_CHECK_EVERY", 50))
VERBOSE = os.environ.get("PINNFEM_QUIET", "0") != "1"


def _say(msg: str = ""):
    if VERBOSE:
        print(msg)


def _engine_for(model: FEMModel, measured_disp, measured_dofs) -> HipEngine:
    """One engine (mesh plan + device buffers) per model and measurement set, reused across load
    increments and phases like the reference reuses the nn.Modules."""
    key = _engine_key_terms(model, measured_disp, measured_dofs) + (getattr(model, "_pf_mlp_dtype", None),
                                                                    getattr(model, "_pf_fe_mode", None))
    cache = getattr(model, "_pf_engine_cache", None)
    if cache is not None and cache[0] == key and (not cache[1].n_theta or cache[1].theta.still_bound()):
        return cache[1]
    eng = HipEngine(model, measured_disp, measured_dofs, fe_mode=getattr(model, "_pf_fe_mode", None))
    model._pf_engine_cache = (key, eng)
    return eng


def _material_signature(model: FEMModel):
    """What of the material an engine bakes in: which properties are networks (and which module), and the
    value of every scalar one (the reference re-reads material.*.value() on every assembly)."""
    sig = []
    for prop in (model.material.young, model.material.area, model.material.density):
        if prop.is_trainable():
            sig.append(("nn", id(prop.net), bool(prop.enforce_positive), float(prop.scale)))
        else:
            sig.append(("scalar", float(prop.value())))
    return tuple(sig)


def _engine_key_terms(model: FEMModel, measured_disp, measured_dofs) -> tuple:
    """What the cache key of the single-GPU engine and the one of the sharded backend share: the measurement set, the
    mesh, the loads, the supports and the material."""
    return (None if measured_disp is None else np.asarray(measured_disp, dtype=float).tobytes(),
            None if measured_dofs is None else np.asarray(measured_dofs, dtype=int).tobytes(),
            model.nodes.tobytes(), model.elements.tobytes(), model.loads.tobytes(),
            model.fixed_dofs.tobytes(), _material_signature(model))


def _shifted_history(first, second):
    """The history of two phases run one after the other: first's entries, then copies of second's with their iteration
    numbers continuing from first's last."""
    shift = first[-1].get("iteration", 0) if first else 0
    return list(first) + [dict(entry, iteration=entry.get("iteration", 0) + shift) for entry in second]


def _result(model, u, reactions, free, converged, history, theta_list=(), **more) -> SolverResult:
    """The tail of every solver: u and reactions (host, [n_dofs]) in the nodal shape, the reactions zeroed on the free
    dofs (a mask or indices), the NN parameters when there are any."""
    shape = (-1, 1) if model.dimension == 1 else (model.nnode, model.dimension)
    reactions[free] = 0.0
    nn_params = {f"param_{i}": p.detach().cpu().numpy() for i, p in enumerate(theta_list)} if theta_list else None
    return SolverResult(displacements=u.reshape(shape), reactions=reactions.reshape(shape), converged=converged,
                        history=history, nn_parameters=nn_params, **more)


def solve_gd(
    model: FEMModel,
    config: Optional[SolverConfig] = None,
    measured_disp: Optional[np.ndarray] = None,
    measured_dofs: Optional[List[int]] = None,
    target_load_factor: float = 1.0,
    u_initial: Optional[torch.Tensor] = None,
    skip_preconditioning: bool = False,
) -> SolverResult:
    """Gradient Descent solver for FEM/PINN problems (solver.py:83-400)."""
    config = config or SolverConfig()
    check_control(config, method="gd")
    if check_kinematics(config.kinematics) == "green-lagrange":
        # the GD path assembles the small-displacement element only (solve_hybrid runs it as phase 1 of a
        # Green-Lagrange Newton solve, which then starts from this linear answer)
        warnings.warn("kinematics 'green-lagrange' applies to the Newton-Raphson solve only: solve_gd uses the linear "
                      "element", RuntimeWarning, stacklevel=2)

    # ---- two-phase "preconditioning" schedule (solver.py:113-198) --------------------------------
    if config.preconditioning and not skip_preconditioning:
        _say("GD Preconditioning phase...")
        precon_config = copy.deepcopy(config)
        precon_config.max_iterations = min(300, config.max_iterations // 3)
        precon_config.tolerance = max(1e-4, config.tolerance * 10)
        precon_config.preconditioning = False
        try:
            precon_result = solve_gd(model, precon_config, measured_disp, measured_dofs,
                                     target_load_factor, u_initial, skip_preconditioning=True)
            _say(f"  Preconditioning: {precon_result.history[-1]['iteration']} iterations")
            if (precon_result.converged
                    and precon_result.history[-1].get("residual_norm", 1.0) < config.tolerance):
                _say("  Preconditioning achieved final convergence")
                return precon_result
            u_initial = torch.tensor(precon_result.displacements.flatten(), dtype=torch.float32)
            _say("Main GD phase (tight tolerance)...")
            main_config = copy.deepcopy(config)
            main_config.max_iterations = config.max_iterations - precon_config.max_iterations
            main_config.preconditioning = False
            main_result = solve_gd(model, main_config, measured_disp, measured_dofs,
                                   target_load_factor, u_initial, skip_preconditioning=True)
            main_result.history = _shifted_history(precon_result.history, main_result.history)
            total_iterations = (main_result.history[-1].get("iteration", 0)
                                if main_result.history else 0)
            _say(f"  Total GD (with preconditioning): {total_iterations} iterations")
            return main_result
        except NotImplementedError:
            raise
        except Exception as e:  # solver.py:197-198 swallows and falls through to plain GD
            _say(f"  Preconditioning failed: {e}, proceeding with standard GD")

    has_nn = model.material.has_trainable_params()
    theta_list = model.material.get_all_torch_params() if has_nn else []
    has_measurements = measured_disp is not None and measured_dofs is not None
    eng = _engine_for(model, measured_disp, measured_dofs) if _world_size() == 1 else None
    if u_initial is not None:
        _say("  🔥 Using warm start from previous increment")
    else:
        _say("  ❄️  Cold start from zeros")
    if has_measurements and config.alpha_data == 0.0:
        _say("⚠️  Warning: measured_dofs provided but alpha_data=0.0")

    header = (f"{'Iter':>6} | {'Loss Total':>12} | {'Loss Physics':>12} | {'||R||':>12} | "
              f"{'Loss Data':>12} | {'||u||':>10}")
    if has_nn:
        header += f" | {'NN Params':>10}"
    _say(header)
    _say("-" * (82 + (12 if has_nn else 0)))

    if _world_size() > 1:
        return _solve_gd_sharded(model, config, measured_disp, measured_dofs, target_load_factor,
                                 u_initial, has_nn, theta_list, has_measurements)

    # ---- the hot loop (solver.py:252-355) on the device --------------------------------------------
    eng.begin(u_initial, target_load_factor, config)
    n_launched = 0
    st = None
    k = max(int(eng.GRAPH_ITERS), 1)
    poll = max(k, (CHECK_EVERY // k) * k)      # whole graph replays per poll (large meshes replay 20 iterations at a time)
    while n_launched < config.max_iterations:
        chunk = min(poll, config.max_iterations - n_launched)
        # chained replays: a replay leaves the updates and the bookkeeping of its last iteration to the next replay's first
        # iteration (HipEngine.iterate, defer_tail), so the state read here lags by that one iteration — the stop flag is all
        # the loop needs; launches behind a stop are no-ops
        eng.iterate(chunk, defer_tail=True)
        n_launched += chunk
        st = eng.state()                       # one small D2H copy + sync per chunk
        if st.done:
            break
    eng.flush()                                # the pending tail (no-ops after a stop)
    st = eng.state()
    n_iter = st.iter if st is not None else 0
    converged = bool(st.converged) if st is not None else False
    history = _history_from_rows(eng.history(n_iter), n_iter, has_measurements, theta_list)
    for it, entry in enumerate(history):
        if VERBOSE and ((it + 1) % config.print_every == 0 or it == 0):
            msg = (f"{it+1:6d} | {entry['loss_total']:12.3e} | {entry['loss_physics']:12.3e} | "
                   f"{entry['residual_norm']:12.3e} | {entry['loss_data']:12.3e} | {entry['u_norm']:10.3e}")
            if has_nn:
                msg += f" | {entry['theta_norm']:10.3e}"
            print(msg)
    if converged:
        last = history[-1]
        if last["residual_norm"] < config.tolerance:
            _say(f"\n[CONVERGED] Reached equilibrium in {n_iter} iterations "
                 f"(residual={last['residual_norm']:.2e} < tol={config.tolerance:.1e})")
        else:
            _say(f"\n[CONVERGED] Loss minimized in {n_iter} iterations "
                 f"(loss={last['loss_total']:.2e} < tol={config.tolerance:.1e})")
    else:
        _say(f"\n[WARNING] Did not converge in {config.max_iterations} iterations.")
        if history:
            _say(f"          Final loss: {history[-1]['loss_total']:.3e}")

    # ---- result (solver.py:365-400) -----------------------------------------------------------------
    u_final = eng.u.detach().cpu().numpy().copy()
    f_int_final = eng.internal_force(lam=target_load_factor)           # no-grad re-assembly :374-377
    reactions_t = f_int_final - float(np.float32(target_load_factor)) * eng.f_ext
    return _result(model, u_final, reactions_t.cpu().numpy(), eng.plan.free_dofs, converged, history, theta_list)  # :379


def _world_size() -> int:
    import torch.distributed as dist
    return dist.get_world_size() if (dist.is_available() and dist.is_initialized()) else 1


def _history_from_rows(rows, n_iter, has_measurements, theta_list):
    history = []
    for it in range(n_iter):
        r = rows[it]
        entry = {"iteration": float(it + 1), "loss_total": float(r[0]), "loss_physics": float(r[1]),
                 "loss_data": float(r[2]) if has_measurements else 0.0, "u_norm": float(r[3]),
                 "residual_norm": float(r[4])}
        if theta_list:
            entry["theta_norm"] = float(r[5])
        history.append(entry)
    return history


def _solve_gd_sharded(model, config, measured_disp, measured_dofs, lam, u_initial, has_nn, theta_list,
                      has_measurements) -> SolverResult:
    """solve_gd body when torch.distributed runs with world_size > 1: elements sharded over the
    ranks (pinn_fem_amd.dist); every rank returns the same global SolverResult."""
    import torch.distributed as dist
    from .. import dist as pfd
    key = ("shard", dist.get_rank(), dist.get_world_size()) + _engine_key_terms(model, measured_disp, measured_dofs)
    cache = getattr(model, "_pf_shard_cache", None)
    if cache is not None and cache[0] == key and (not cache[1].eng.n_theta or cache[1].eng.theta.still_bound()):
        be = cache[1]
    else:
        be = pfd.build_shard_backend(model, measured_disp, measured_dofs, dist.get_rank(),
                                     dist.get_world_size())
        model._pf_shard_cache = (key, be)
    u0 = None
    if u_initial is not None:
        ug = u_initial.detach().cpu().numpy() if isinstance(u_initial, torch.Tensor) else np.asarray(u_initial)
        u0 = torch.from_numpy(np.ascontiguousarray(ug.reshape(-1)[be.dofs_global], dtype=np.float32))
    be.begin(u0, lam, config)
    bufs = be.bufs
    n_done, st = 0, None
    while n_done < config.max_iterations:
        chunk = min(CHECK_EVERY, config.max_iterations - n_done)
        pfd.run_iterations(be, chunk, bufs=bufs)
        st = be.state()
        n_done = st.iter
        if st.done:
            break
    n_iter = st.iter if st is not None else 0
    converged = bool(st.converged) if st is not None else False
    history = _history_from_rows(be.history(n_iter), n_iter, has_measurements, theta_list)
    u_glob = pfd.gather_global_vector(be.eng.u, be, model.ndof)
    f_loc = pfd.assembled_f_int(be, lam)
    r_loc = f_loc - float(np.float32(lam)) * be.eng.f_ext
    r_glob = pfd.gather_global_vector(r_loc, be, model.ndof)
    return _result(model, u_glob, r_glob, _free_mask(model), converged, history, theta_list)


class _NewtonSetup(NamedTuple):
    """What a Newton solve and an identification evaluation hold before their first iteration (_newton_setup)."""
    eng: HipEngine
    free: np.ndarray                        # bool [n_dofs], host
    free_t: torch.Tensor                    # the same on the device
    loads: torch.Tensor                     # the loads at load factor 1, float64 [n_dofs] on the device
    e0_np: Optional[np.ndarray]             # check_initial_strain's array, or None
    e0: Optional[torch.Tensor]              # the same on the device
    u: torch.Tensor                         # the start vector, float64 [n_dofs] on the device, zero on the fixed dofs
    plastic: Optional[tuple] = None         # check_plasticity's (ey, kappa) on the device, or None: elastic elements
    cable: Optional[torch.Tensor] = None    # check_cables' flags on the device (uint8 [n_elems]), or None: all bars


def _newton_setup(model, e0_np, u_initial=None, cable_np=None, plastic_np=None) -> _NewtonSetup:
    """The one host setup of solve_nr under either control and of fem/identify.py.  e0_np: check_initial_strain's
    result; like every check_* it is the caller's to run first, this is where the engine is built.  u_initial: a tensor
    or an array [n_dofs] (its fixed dofs are ignored); None: zeros.  cable_np: check_cables' result; plastic_np:
    check_plasticity's.  It launches nothing but torch's own copies and fills; _pre_check is the first to touch the kernels."""
    eng = _engine_for(model, None, None)
    dev, ndof = eng.device, model.ndof
    free = _free_mask(model)
    u = torch.zeros(ndof, dtype=torch.float64, device=dev)
    if u_initial is not None:
        u0 = u_initial.detach() if isinstance(u_initial, torch.Tensor) else torch.as_tensor(np.asarray(u_initial))
        u = u0.to(device=dev, dtype=torch.float64).reshape(-1).clone()
        if u.numel() != ndof:
            raise ValueError(f"u_initial has {u.numel()} entries, the model has {ndof} dofs")
        u[torch.from_numpy(~free).to(dev)] = 0.0
    loads = torch.from_numpy(np.ascontiguousarray(np.asarray(model.loads, dtype=float).reshape(-1))).to(dev)
    return _NewtonSetup(eng, free, torch.from_numpy(free).to(dev), loads, e0_np,
                        None if e0_np is None else torch.from_numpy(e0_np).to(dev), u,
                        plastic=None if plastic_np is None else tuple(torch.from_numpy(v).to(dev) for v in plastic_np),
                        cable=None if cable_np is None else torch.from_numpy(cable_np.astype(np.uint8)).to(dev))


def _gl_state(s: _NewtonSetup, u, ea=None):
    """The element state of a Newton solve at u: the cable state where the setup carries flags, the plastic state from the
    engine's committed (ep, alpha) where it carries yield strains, the bar state otherwise."""
    if s.cable is not None:
        return s.eng.gl_state_cable(u, s.cable, ea, s.e0)
    if s.plastic is not None:
        return s.eng.gl_state_plastic(u, s.plastic[0], s.plastic[1], ea, s.e0)
    return s.eng.gl_state(u, ea, s.e0)


def _pre_check(s: _NewtonSetup, ea=None, held=()):
    """The pre-check of a Newton solve from s.u with the element stiffnesses ea (None: the model's), the dofs `held`
    prescribed on top of the fixed ones.  A free dof no element stiffens makes K_ff singular: np.linalg.solve raises
    there (solver.py:462-467).  With initial strains the geometric stiffness may be all that holds a dof (a taut
    string), so the tangent at the starting state decides, not the linear diagonal: it must be positive on every free
    dof that is not held (a free dof that only a slack or compressed member holds is a mechanism).  That branch leaves
    the gl_state of (s.u, ea, s.e0) on the engine.  With cable flags it is taken too, with or without e0, on the cable
    state from a cleared slack set: an unstrained cable at u = 0 has e - e0 = 0, is taut and counts with its bar block.
    With yield strains it is taken too, on the plastic state from the committed (ep, alpha) the caller has just set on the
    engine (gl_plastic_reset): a perfectly plastic element that yields at the starting state holds nothing."""
    if s.e0 is None and s.cable is None and s.plastic is None:
        if bool((s.eng.diag_k().cpu().numpy()[s.free] == 0.0).any()):
            raise RuntimeError("Tangent stiffness became singular during solve")
        return
    if s.cable is not None:
        s.eng.gl_slack_clear()
    _gl_state(s, s.u, ea)
    dg = s.eng.kt_diag().cpu().numpy()
    free = s.free.copy()
    free[list(held)] = False
    bad = np.flatnonzero(free & ~(dg > 0.0))
    if bad.size:
        raise RuntimeError(f"Tangent stiffness is not positive definite at the starting state: its diagonal is "
                           f"{dg[bad[0]]:.6g} at free dof {int(bad[0])} (a slack or compressed mechanism; "
                           f"{bad.size} such dof{'s' if bad.size > 1 else ''})")


def _newton_loop(s, model, config, f_ext, u, green_lagrange, ea=None):
    """The Newton iteration of solve_nr from u at the load f_ext: u += K^-1 (f_ext - f_int(u)) by CG until
    |du| / max(|u|, min_denominator) <= tolerance.  s: the _newton_setup (its engine, free mask and initial strain);
    ea (Green-Lagrange only): E*A of every element in place of the model's (fem/identify.py).  Returns (u, converged,
    |du|/|u|, max strain of the linear branch, index of the last iteration, CG iterations).

    With s.cable (tension-only elements) it is an active-set (semismooth) Newton iteration: every iteration forms the
    cable state at u (pf_gl_state_cable: a flagged element with e - e0 < 0 is slack, no force and no tangent block),
    solves with its tangent and reads the two counts the kernel leaves, 16 bytes.  It has converged when the
    displacement test holds AND the slack set of this iteration's state is the one of the state before (the first
    iteration's count against the cleared set does not count).  There is no line search and no damping: a set that keeps
    changing runs to max_iterations and returns converged = False like any other solve that does not converge, and
    solve()'s load increments (n_increments) are the remedy.  Whenever the set changed, the tangent's diagonal is read
    before the CG solve: a free dof that only slack cables hold is a mechanism and raises RuntimeError.

    With s.plastic (elastoplastic elements) every iteration forms the plastic state at u from the engine's committed
    (ep, alpha) (pf_gl_state_plastic), never from the iterate before.  Its tangent is the consistent one, so the
    displacement test alone stops the loop.  Whenever a flag changed against the state before (the pre-check's, in the
    first iteration), the tangent's diagonal is read before the CG solve: a free dof with a diagonal <= 0 is a plastic
    mechanism (collapse) and raises RuntimeError.  Nothing is committed here: solve_nr commits its closing state."""
    eng = s.eng
    has_converged, residual_norm, max_e, ite = False, float("inf"), 0.0, -1
    cg0 = eng.pcg_iterations
    if s.cable is not None:
        eng.gl_slack_clear()
    for ite in range(config.max_iterations):
        set_changed = False
        if green_lagrange:
            _gl_state(s, u, ea)                     # the history's max |e| is read once, from the state at the final u
            if s.cable is not None:
                n_changed = eng.gl_slack_counts()[1]
                if n_changed:
                    _check_slack_mechanism(s, ite)
                set_changed = ite > 0 and n_changed > 0
            elif s.plastic is not None and eng.gl_plastic_counts()[1]:
                _check_plastic_mechanism(s, ite)
            rhs = f_ext - eng.gl_fint()
            du, _, ok, rr, bb = eng.pcg_solve(rhs, tangent=True, preconditioner=config.nr_preconditioner,
                                             n_aggregates=config.nr_aggregates, u=u)
        else:
            max_e = _max_abs_strain(model, u)
            rhs = f_ext - eng.kv_f64(u)
            du, _, ok, rr, bb = eng.pcg_solve(rhs, preconditioner=config.nr_preconditioner,
                                             n_aggregates=config.nr_aggregates)
        _check_cg_step(green_lagrange, rhs, du, ok, rr, bb, s.free_t)
        u = u + du
        residual_norm = float(torch.linalg.norm(du)) / max(float(torch.linalg.norm(u)), config.min_denominator)
        if residual_norm <= config.tolerance and not set_changed:
            has_converged = True
            break
    return u, has_converged, residual_norm, max_e, ite, eng.pcg_iterations - cg0


def _check_slack_mechanism(s, ite):
    """After a change of the slack set: the tangent of the cable state on the engine must keep a positive diagonal on
    every free dof (_pre_check's rule; one launch and one read)."""
    dg = s.eng.kt_diag().cpu().numpy()
    bad = np.flatnonzero(s.free & ~(dg > 0.0))
    if bad.size:
        raise RuntimeError(f"Tangent stiffness is not positive definite in Newton iteration {ite + 1}: its diagonal is "
                           f"{dg[bad[0]]:.6g} at free dof {int(bad[0])}, which only slack cables hold (a mechanism; "
                           f"{bad.size} such dof{'s' if bad.size > 1 else ''}).  The static solve cannot carry a "
                           "structure through a slack mechanism: use solve_dynamic with rest_tolerance")


def _check_plastic_mechanism(s, ite):
    """After a change of the yielding set: _check_slack_mechanism's rule on the plastic state on the engine."""
    dg = s.eng.kt_diag().cpu().numpy()
    bad = np.flatnonzero(s.free & ~(dg > 0.0))
    if bad.size:
        raise RuntimeError(f"Tangent stiffness is not positive definite in Newton iteration {ite + 1}: its diagonal is "
                           f"{dg[bad[0]]:.6g} at free dof {int(bad[0])}, which only yielding elements hold (a plastic "
                           f"mechanism, collapse; {bad.size} such dof{'s' if bad.size > 1 else ''}).  The load is beyond "
                           "what the structure carries: reduce it, or give the elements a hardening_ratio")


# what load control says when _check_cg_step refuses a solve: (the residual does not come down, rhs.x <= 0)
_LOAD_REFUSALS = ("Tangent stiffness became singular during solve",
                  "Tangent stiffness is not positive definite (limit point or buckling): the CG solve of "
                  "the Green-Lagrange Newton step needs an SPD tangent; reduce the load step")


def _check_cg_step(spd, rhs, x, ok, rr, bb, free_t, refusals=_LOAD_REFUSALS):
    """What solve_nr asks of a CG solve K x = rhs, under either control; refusals: the two RuntimeError messages.
    free_t: the mask the rhs.x test runs over; None: rhs is zero outside the solve's dofs already, no gather."""
    # np.linalg.solve either succeeds or raises on a singular matrix; CG shows singularity (or a hopeless
    # condition number for the Jacobi preconditioner) as a residual that does not come down at all.  An
    # inner solve that merely stops short of 1e-13 is fine: the Newton loop then acts as iterative refinement.
    if not np.isfinite(rr) or (not ok and rr > 1e-4 * bb):
        raise RuntimeError(refusals[0])
    # CG is only valid for a positive definite operator: x = K_t^-1 rhs must be an ascent direction of rhs
    if spd and bb > 0.0:
        dot = torch.dot(rhs, x) if free_t is None else torch.dot(rhs[free_t], x[free_t])
        if not float(dot) > 0.0:
            raise RuntimeError(refusals[1])


def solve_nr(model, config=None, target_load_factor=1.0, u_initial=None, plastic_state=None) -> SolverResult:
    """Classical Newton-Raphson for scalar materials (solver.py:408-512), SURVEY.md §8(f) rank 3.

    The reference assembles the dense float64 tangent (fem/assembly.py:16-75) and calls
    np.linalg.solve on K_ff; here K is applied matrix-free in float64 on the device (pf_kv_f64) and
    K_ff du = rhs is solved by conjugate gradients with the diag(K_ff) (Jacobi) preconditioner
    (pf_pcg_*) or, with config.nr_preconditioner = "two-level", Jacobi plus a coarse space of per-aggregate
    rigid-body modes (pf_pcg2_*), so the solver no longer stops at the ~2*10^4 dofs a dense K allows.  Same loop, same
    stopping rule (|du| / max(|u|, min_denominator) <= tolerance), same history record; like the
    reference, u starts from zero whatever u_initial says (:443).

    config.kinematics = "green-lagrange" replaces the linear element by the total-Lagrangian one (pf_gl_state,
    pf_gl_fint): u starts from u_initial when given, every iteration re-forms the element state at u and
    solves K_t(u) du = load_factor f_ext - f_int(u) with the Jacobi-preconditioned CG on the tangent (pf_pcgt_*) or, with
    config.nr_preconditioner = "two-level-updated", the two-level one whose coarse space follows X + u (pf_pcg2t_*).  CG needs
    K_t positive definite: under load control a limit point or buckling (rhs.du <= 0) raises RuntimeError.

    config.nr_control = "displacement" (Green-Lagrange only) passes a limit point of the load: target_load_factor is then
    the fraction of config.nr_control_displacement the control dof is held at and the load factor is solved for
    (_solve_nr_displacement).  There is no arc-length control.

    config.initial_strain (Green-Lagrange only; check_initial_strain) gives every element an eigenstrain e0,
    N = E*A (e - e0): it goes into every gl_state call, in full at every load factor, the pre-check then reads the tangent's
    diagonal at the starting state (a free dof with a diagonal <= 0 raises RuntimeError "... not positive definite ...")
    and the result carries axial_forces.

    config.cable_elements (Green-Lagrange, load control only; check_cables) flags tension-only elements: the Newton loop
    iterates on the slack set (_newton_loop), the closing state is the cable state, and the result carries slack (bool
    [n_elems]) and axial_forces with 0.0 on the slack elements; the history row counts them ("slack_elements").  An
    element that flips in the closing state has a force of zero within the tolerance; nothing more is iterated.  A set
    that does not settle returns converged = False: use solve() with more increments.

    config.yield_strain / config.hardening_ratio (Green-Lagrange, load control, bars; check_plasticity) make the elements
    elastoplastic.  plastic_state: the committed (ep, alpha) the solve starts from, a pair of arrays
    [n_elems]; None: zeros.  Every iteration forms the plastic state from that committed pair.  The closing state at the
    final u is the one that is committed: the result carries it as plastic_strain and accumulated_plastic_strain (the
    next increment's plastic_state), yielding (bool [n_elems], the elements that yielded in this solve's closing state),
    axial_forces = E*A (e - e0 - ep), and the history row counts "yielding_elements".  An unconverged solve commits
    nothing and returns the state it was given.  A free dof that only yielding elements without hardening hold is a
    plastic mechanism: RuntimeError."""
    config = config or SolverConfig()
    green_lagrange = check_kinematics(config.kinematics, config.nr_preconditioner) == "green-lagrange"
    e0_np = check_initial_strain(config, model)
    cable_np = check_cables(config, model)
    plastic_np = check_plasticity(config, model)
    if plastic_state is not None and plastic_np is None:
        raise ValueError("plastic_state needs config.yield_strain: without it the solve is elastic and would ignore it.")
    if plastic_np is not None:
        plastic_state = check_plastic_state(plastic_state if plastic_state is not None
                                            else (np.zeros(model.nelm), np.zeros(model.nelm)), model.nelm)
    if check_control(config, model) == "displacement":
        return _solve_nr_displacement(model, config, target_load_factor, u_initial, e0_np)
    if model.material.has_trainable_params():
        raise ValueError("Newton-Raphson solver with NN materials not fully supported yet. "
                         "Use solve_gd() for problems with NN parameters.")
    if green_lagrange:
        if _world_size() > 1:
            raise ValueError("kinematics 'green-lagrange' does not support a sharded (multi-GPU) run.")
    s = _newton_setup(model, e0_np, u_initial if green_lagrange else None, cable_np, plastic_np)
    if s.plastic is not None:
        s.eng.gl_plastic_reset(*plastic_state)            # the committed state every evaluation of this solve starts from
    _pre_check(s)
    eng, load_factor = s.eng, target_load_factor
    f_ext = float(load_factor) * s.loads
    u, has_converged, residual_norm, max_e, ite, _ = _newton_loop(s, model, config, f_ext, s.u, green_lagrange)
    axial = slack = None
    plastic = {}
    if green_lagrange:
        strain = _gl_state(s, u)                          # state at the final u: its strain, and f_int for the reactions
        max_e = float(strain.abs().max()) if model.nelm else 0.0
        reactions = (eng.gl_fint() - f_ext).cpu().numpy()
        if s.e0 is not None or s.cable is not None:
            axial = _axial_forces(model, strain, 0.0 if s.e0_np is None else s.e0_np)
        if s.cable is not None:
            slack = eng.gl_slack_mask()
            axial = np.where(slack, 0.0, axial)
        if s.plastic is not None:
            ep, alpha, yielding = eng.gl_plastic_state()  # of the closing state: the one that is committed
            axial = _axial_forces(model, strain, ep if s.e0_np is None else s.e0_np + ep)
            if has_converged:
                eng.gl_plastic_commit()
            else:
                ep, alpha = plastic_state
            plastic = dict(plastic_strain=ep, accumulated_plastic_strain=alpha, yielding=yielding)
    else:
        reactions = (eng.kv_f64(u) - f_ext).cpu().numpy()
    history = [{"load_factor": float(load_factor), "iterations": float(ite + 1), "residual": float(residual_norm),
                "max_strain": float(max_e), "converged": float(1.0 if has_converged else 0.0)}]
    if slack is not None:
        history[-1]["slack_elements"] = float(slack.sum())
    if plastic:
        history[-1]["yielding_elements"] = float(plastic["yielding"].sum())
    return _result(model, u.cpu().numpy(), reactions, s.free, has_converged, history, axial_forces=axial, slack=slack,
                   **plastic)


def _solve_nr_displacement(model, config, control_factor, u_initial, e0_np=None) -> SolverResult:
    """solve_nr under displacement control (Batoz-Dhatt), Green-Lagrange kinematics; DESIGN.md §7.

    The free dof c = config.nr_control_dof is held at ubar = control_factor * config.nr_control_displacement and the load
    factor lam is an unknown.  With F' the free dofs without c, K' = K_t[F', F'] and k_c = K_t[:, c], an iteration is
      R = f_int(u) - lam f,  du_c = ubar - u_c            (non-zero in the first iteration only)
      K' a = f[F'],   K' b = -R[F'] - k_c[F'] du_c        (one batched CG solve: two right-hand sides per launch)
      dlam = -(R_c + k_c[F'].b + K_cc du_c) / (k_c[F'].a - f_c)
      u[F'] += b + dlam a,  u_c = ubar,  lam += dlam
    until |du| / max(|u|, min_denominator) and |dlam| / max(|lam|, min_denominator) are both <= tolerance.  K' stays
    positive definite through a limit point of the load, so the CG solves of load control serve; a K' that is not
    (a turning point of the control displacement, or a bifurcation the right-hand sides excite) is refused.
    lam starts at f[F].f_int(u)[F] / f[F].f[F]: the previous increment's lam when u is a converged state."""
    c = int(config.nr_control_dof)
    ubar = float(control_factor) * float(config.nr_control_displacement)
    s = _newton_setup(model, e0_np, u_initial)
    _pre_check(s, held=[c])                 # solve_nr's rule; the control dof is held, so K' is what must be definite
    eng, f, u, free_t = s.eng, s.loads, s.u, s.free_t
    fc_t = free_t.clone()
    fc_t[c] = False                                     # F'
    f_fc = torch.where(fc_t, f, torch.zeros_like(f))
    f_c = float(f[c])
    have_a = bool((f_fc != 0.0).any())
    e_c = torch.zeros_like(f)
    e_c[c] = 1.0
    pcg_args = dict(tangent=True, preconditioner=config.nr_preconditioner, n_aggregates=config.nr_aggregates,
                    extra_fixed=[c])
    refusals = tuple(f"Tangent stiffness with control dof {c} removed is not positive definite ({why}): "
                     "displacement control needs an SPD K' (a turning point of the control displacement or a "
                     "bifurcation is not passed); choose another control dof or a smaller step"
                     for why in ("the CG residual does not come down", "rhs.x <= 0"))

    def checked(x, rhs, report):
        _check_cg_step(True, rhs, x, *report[1:], None, refusals)      # rhs is zero outside F'
        return x

    if s.e0 is None:                        # (with initial strains the pre-check has just formed this state)
        eng.gl_state(u, None, None)
    lam = float(torch.dot(f[free_t], eng.gl_fint()[free_t])) / float(torch.dot(f[free_t], f[free_t]))
    has_converged, residual_norm, load_residual, ite = False, float("inf"), float("inf"), -1
    for ite in range(config.max_iterations):
        if ite > 0:
            eng.gl_state(u, None, s.e0)     # (the first iterate's state is the one lam was started from)
        R = eng.gl_fint() - lam * f
        du_c = ubar - float(u[c])
        k_c = eng.kt_v_f64(e_c)             # column c of K_t, every row
        rhs_b = torch.where(fc_t, -R - k_c * du_c, torch.zeros_like(R))
        if have_a:
            X, reports = eng.pcg_solve_batch(torch.stack([f_fc, rhs_b]), u=u, **pcg_args)
            a, b = checked(X[0], f_fc, reports[0]), checked(X[1], rhs_b, reports[1])
        else:
            x, *report = eng.pcg_solve(rhs_b, u=u, **pcg_args)
            a, b = torch.zeros_like(x), checked(x, rhs_b, report)
        kc_fc = torch.where(fc_t, k_c, torch.zeros_like(k_c))
        kc_a = float(torch.dot(kc_fc, a))
        den = kc_a - f_c
        if abs(den) <= 1e-12 * (float(torch.linalg.norm(kc_fc)) * float(torch.linalg.norm(a)) + abs(f_c)):
            raise RuntimeError(f"control dof {c} does not respond to the load (k_c.a - f_c = {den:.3e}): displacement "
                               "control cannot solve for the load factor; choose another control dof")
        dlam = -(float(R[c]) + float(torch.dot(kc_fc, b)) + float(k_c[c]) * du_c) / den
        du = b + dlam * a
        du[c] = du_c
        u = u + du
        u[c] = ubar
        lam += dlam
        residual_norm = float(torch.linalg.norm(du)) / max(float(torch.linalg.norm(u)), config.min_denominator)
        load_residual = abs(dlam) / max(abs(lam), config.min_denominator)
        if residual_norm <= config.tolerance and load_residual <= config.tolerance:
            has_converged = True
            break
    strain = eng.gl_state(u, None, s.e0)
    max_e = float(strain.abs().max()) if model.nelm else 0.0
    reactions = (eng.gl_fint() - lam * f).cpu().numpy()
    history = [{"load_factor": float(lam), "iterations": float(ite + 1), "residual": float(residual_norm),
                "max_strain": float(max_e), "converged": float(1.0 if has_converged else 0.0),
                "control_factor": float(control_factor), "control_displacement": float(ubar),
                "load_residual": float(load_residual)}]
    # the control dof is free: the load carries it, it has no reaction
    return _result(model, u.cpu().numpy(), reactions, s.free, has_converged, history,
                   axial_forces=None if s.e0 is None else _axial_forces(model, strain, s.e0_np))


def _max_abs_strain(model, u) -> float:
    """max |epsilon| over the elements, epsilon = axial stretch / l0 (fem/element.py:27-28, 74-80): a
    monitor of the history record only (host, float64)."""
    uu = u.detach().cpu().numpy().astype(float)
    nodes = np.asarray(model.nodes, dtype=float)
    el = np.asarray(model.elements, dtype=int)
    if el.size == 0:
        return 0.0
    if model.dimension == 1:
        x = nodes.reshape(-1)
        l0 = np.abs(x[el[:, 1]] - x[el[:, 0]])
        eps = (uu[el[:, 1]] - uu[el[:, 0]]) / l0
    else:
        d0 = nodes[el[:, 1]] - nodes[el[:, 0]]
        l0 = np.linalg.norm(d0, axis=1)
        U = uu.reshape(-1, 2)
        du = U[el[:, 1]] - U[el[:, 0]]
        eps = ((d0[:, 0] / l0) * du[:, 0] + (d0[:, 1] / l0) * du[:, 1]) / l0
    return float(np.max(np.abs(eps)))


def solve_full_nr(*args, **kwargs) -> SolverResult:
    """solver.py:753-1037 — out of scope (and non-functional in the reference)."""
    raise NotImplementedError("solve_full_nr is outside the accelerated PINN+GD path")


def solve_hybrid(
    model: FEMModel,
    config: Optional[SolverConfig] = None,
    measured_disp: Optional[np.ndarray] = None,
    measured_dofs: Optional[List[int]] = None,
    target_load_factor: float = 1.0,
    u_initial: Optional[torch.Tensor] = None,
    plastic_state=None,
) -> SolverResult:
    """Hybrid solver (solver.py:520-692).  With NN materials phase 2 is GD again (:594-651).  plastic_state: solve_nr's,
    handed to the Newton phase (the GD phase is the linear elastic warm start it always was; with config.yield_strain its
    early return on a tight GD convergence is not taken, so the answer always comes from the plastic Newton solve)."""
    config = config or SolverConfig()
    check_kinematics(config.kinematics, config.nr_preconditioner)
    check_control(config, method="hybrid")
    check_cables(config, model, "hybrid")
    plastic = check_plasticity(config, model, "hybrid") is not None
    _say("=== HYBRID SOLVER ===")
    _say(f"Target load factor: {target_load_factor}")
    gd_result = None
    gd_config = None
    if config.preconditioning:
        _say("Phase 1: GD Preconditioning...")
        gd_config = copy.deepcopy(config)
        gd_config.max_iterations = min(300, config.max_iterations // 3)
        gd_config.tolerance = max(1e-4, config.tolerance * 10)
        try:
            gd_result = solve_gd(model, gd_config, measured_disp, measured_dofs, target_load_factor,
                                 u_initial, skip_preconditioning=True)
            _say(f"  GD Phase: {gd_result.history[-1]['iteration']} iterations")
            if (gd_result.converged and not plastic
                    and gd_result.history[-1].get("residual_norm", 1.0) < config.tolerance):
                _say("  GD achieved tight convergence, skipping NR phase")
                return gd_result
            # (with yield_strain the Newton phase always runs: the GD answer is the linear elastic one and carries no
            # plastic state, however tightly it converged)
        except NotImplementedError:
            raise
        except Exception as e:  # solver.py:584-586
            _say(f"  GD Phase failed: {e}, proceeding with cold NR")
            gd_result = None
    else:
        _say("Phase 1: GD Preconditioning SKIPPED (preconditioning=False)")

    _say("Phase 2: Newton-Raphson Finalization...")
    has_nn = model.material.has_trainable_params()
    if not has_nn:
        # scalar materials: the real GD -> NR switch (solver.py:653-692)
        _say("  Scalar materials detected. Using Newton-Raphson.")
        # a Green-Lagrange Newton solve starts from the GD result as it is (float64); the linear one ignores its start
        warm_dtype = torch.float64 if config.kinematics == "green-lagrange" else torch.float32
        u_warm = (torch.tensor(gd_result.displacements.flatten(), dtype=warm_dtype)
                  if gd_result else u_initial)
        nr_result = solve_nr(model, config, target_load_factor, u_warm, plastic_state)
        nr_iterations = nr_result.history[-1].get("iterations", 1) if nr_result.history else 1
        _say(f"  NR Phase: {nr_iterations} iterations")
        if gd_result:
            # the Newton phase is one entry, its last, whose "iteration" becomes the total of both phases
            nr_result.history = _shifted_history(gd_result.history, [dict(entry, iteration=nr_iterations)
                                                                     for entry in nr_result.history[-1:]])
        _say(f"  Hybrid Total: {nr_result.history[-1].get('iteration', nr_iterations)} iterations")
        return nr_result
    _say("  NN parameters detected. Using GD for final convergence with tight tolerance.")
    final_config = copy.deepcopy(config)
    final_config.max_iterations = config.max_iterations - (gd_config.max_iterations if gd_result else 0)
    final_config.tolerance = config.tolerance
    u_warm = (torch.tensor(gd_result.displacements.flatten(), dtype=torch.float32)
              if gd_result else u_initial)
    final_result = solve_gd(model, final_config, measured_disp, measured_dofs, target_load_factor,
                            u_warm, skip_preconditioning=True)
    if gd_result:
        final_result.history = _shifted_history(gd_result.history, final_result.history)
    total_iterations = final_result.history[-1].get("iteration", 0) if final_result.history else 0
    _say(f"  Hybrid Total: {total_iterations} iterations")
    return final_result


def solve(
    model: FEMModel,
    config: Optional[SolverConfig] = None,
    measured_disp: Optional[np.ndarray] = None,
    measured_dofs: Optional[List[int]] = None,
) -> SolverResult:
    """Universal solver with incremental loading (solver.py:1045-1167)."""
    config = config or SolverConfig()
    if config.method != "auto":
        method = config.method.lower()
    else:
        has_nn = model.material.has_trainable_params()
        has_measurements = measured_disp is not None and measured_dofs is not None
        if not has_nn and not has_measurements:
            _say("[AUTO] Selecting: Newton-Raphson (classical FEM)")
            method = "nr"
        elif has_nn:
            _say("[AUTO] Selecting: Gradient Descent (PINN)")
            method = "gd"
        else:
            _say("[AUTO] Selecting: Gradient Descent (inverse problem)")
            method = "gd"

    displacement_control = check_control(config, model, method) == "displacement"
    if check_initial_strain(config, model) is not None and method in ("gd", "full-nr"):
        raise ValueError(f"initial_strain belongs to the Green-Lagrange Newton solve (solve_nr): method {method!r} is "
                         "untouched by it.")
    check_cables(config, model, method)
    plastic = check_plasticity(config, model, method) is not None
    load_factors = check_load_factors(config, method)
    if load_factors is None:
        load_factors = [config.load_factor_initial + (iinc / config.n_increments) * (
            config.load_factor_final - config.load_factor_initial) for iinc in range(1, config.n_increments + 1)]
        load_path = [] if plastic else None
    else:
        load_path = []
    more = {}                               # with plasticity: the committed state the next increment starts from
    path = [] if displacement_control else None
    _say(f"\n{'Inc':>4} | {'Load Factor':>12} | {'Status':>10}")
    _say("-" * 40)
    result = None
    u_current = None
    for iinc, load_factor in enumerate(load_factors, 1):
        _say(f"{iinc:>4} | {load_factor:>12.4f} | {'WARM_START' if u_current is not None else 'COLD_START':>10}")
        u_initial_torch = None
        if u_current is not None:
            # the Green-Lagrange Newton solve continues from the previous increment in float64; every other solver
            # takes its warm start in float32, as the reference does
            warm_dtype = (torch.float64 if (method in ("nr", "hybrid") and config.kinematics == "green-lagrange")
                          else torch.float32)
            u_initial_torch = torch.tensor(u_current, dtype=warm_dtype, requires_grad=False)
            _say(f"    Warm start values: shape={u_initial_torch.shape}, "
                 f"range=[{u_initial_torch.min():.4f}, {u_initial_torch.max():.4f}]")
        if method == "gd":
            result = solve_gd(model, config, measured_disp, measured_dofs,
                              target_load_factor=load_factor, u_initial=u_initial_torch)
        elif method == "nr":
            result = solve_nr(model, config, target_load_factor=load_factor, u_initial=u_initial_torch, **more)
        elif method == "hybrid":
            result = solve_hybrid(model, config, measured_disp, measured_dofs,
                                  target_load_factor=load_factor, u_initial=u_initial_torch, **more)
        elif method == "full-nr":
            result = solve_full_nr(model, config, measured_disp, measured_dofs,
                                   target_load_factor=load_factor)
        else:
            raise ValueError(f"Unknown solver method: {method}")
        u_current = result.displacements.flatten()
        if displacement_control:
            # load_factor above is the control factor; the record's is the solved one
            path.append({key: result.history[-1][key] for key in ("control_displacement", "load_factor", "iterations")})
            result.path = path
        if plastic and result.plastic_strain is not None:
            more = {"plastic_state": (result.plastic_strain, result.accumulated_plastic_strain)}
        if load_path is not None:
            load_path.append({"load_factor": float(load_factor), "iterations": result.history[-1].get("iterations", 0.0),
                              "yielding_elements": result.history[-1].get("yielding_elements", 0.0)})
            result.load_path = load_path
        status = "CONVERGED" if result.converged else "FAILED"
        _say(f"{iinc:4d} | {load_factor:12.6f} | {status:>10}")
        if not result.converged:
            _say(f"[WARNING] Increment {iinc} did not converge, stopping incremental loading.")
            break
    return result
