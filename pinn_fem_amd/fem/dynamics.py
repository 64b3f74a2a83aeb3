"""Explicit dynamics of Green-Lagrange trusses: central differences with a lumped mass and
mass-proportional damping, one kernel launch per time step (pf_gl_dyn_*), thousands of steps replayed as a hipGraph.

    m_i = sum_{e at i} rho A l0_e / 2 (+ nodal_mass), the same for every dof of the node
    v_{n+1/2} = c1 v_{n-1/2} + g (lam(t_n) F - f_int(u_n)) / m,   u_{n+1} = u_n + dt v_{n+1/2}
    c1 = (1 - alpha dt/2) / (1 + alpha dt/2),  g = dt / (1 + alpha dt/2),  lam(t) = lam0 + (lam1 - lam0) min(1, t / t_ramp)

It follows a structure through a limit point of the load, where solve_nr refuses the step, and it is what reads
Material.density.  Scalar materials, one GPU, dimension 1 and 2.

Tension-only (cable) elements, DynamicsConfig.cable_elements: a flagged element with e - e0 < 0 is slack and carries N = 0, no
force and no strain energy (pf_gl_dyn_*_cable).  Only this module knows cables; a damped run with rest_tolerance comes to rest
on the equilibrium of the structure without its slack elements.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np
import torch

from .solver import (SolverConfig, _axial_forces, _newton_setup, _world_size, check_initial_strain, check_kinematics)

# steps of one captured hipGraph: a record interval longer than this is replayed in pieces
GRAPH_STEPS = 500


@dataclass
class DynamicsConfig:
    dt: Optional[float] = None              # the time step; None: dt_safety * 2 / omega_bound at the initial state
    dt_safety: float = 0.9
    t_end: Optional[float] = None           # one of t_end and n_steps
    n_steps: Optional[int] = None
    damping: float = 0.0                    # alpha of the mass-proportional damping C = alpha M
    ramp_time: float = 0.0                  # 0: a step load of load_factor_final
    load_factor_initial: float = 0.0
    load_factor_final: float = 1.0
    record_every: int = 100                 # steps between two record points (the last one is always recorded)
    record_dofs: Optional[List[int]] = None     # the dofs whose displacements are recorded; None: all of them
    nodal_mass: Optional[object] = None     # a mass added at every node (a number) or one for each node
    rest_tolerance: Optional[float] = None  # stop at a record point with kinetic energy <= this x the largest recorded
    cable_elements: Optional[object] = None     # the tension-only elements: "all" or a list of element ids; None or []: all bars


@dataclass
class DynamicsResult:
    times: np.ndarray                       # [n_records] t of every record point, the initial state first
    recorded: np.ndarray                    # [n_records, len(record_dofs)] displacements
    energies: List[dict] = field(default_factory=list)     # per record: kinetic, strain, work, total, max_velocity, omega_bound
                                            # (and slack_elements, their number, in a run with cable_elements)
    displacements: np.ndarray = None        # u at the last step, in the nodal shape
    velocities: np.ndarray = None           # v_{n-1/2} at the last step, in the nodal shape
    axial_forces: np.ndarray = None         # N = E*A (e - e0) of every element at the last step; 0.0 in a slack cable
    reactions: np.ndarray = None            # f_int - lam F on the fixed dofs at the last step
    residual_norm: float = float("nan")     # max |lam F - f_int| on the free dofs at the last step
    dt: float = float("nan")
    steps: int = 0
    at_rest: bool = False
    slack: np.ndarray = None                # bool [n_elems]: the slack cable elements at the last step (all False without cables)


def lumped_mass(model, nodal_mass=None) -> np.ndarray:
    """Mass of every node [n_nodes] in float64: half of rho A l0 of every element at the node, plus nodal_mass."""
    X = np.asarray(model.nodes, dtype=np.float64).reshape(model.nnode, model.dimension)
    el = np.asarray(model.elements, dtype=np.int64).reshape(-1, 2)
    rho_a = float(model.material.density.value()) * float(model.material.area.value())
    half = 0.5 * rho_a * np.linalg.norm(X[el[:, 1]] - X[el[:, 0]], axis=1)
    m = np.zeros(model.nnode)
    np.add.at(m, el[:, 0], half)
    np.add.at(m, el[:, 1], half)
    if nodal_mass is not None:
        m = m + np.broadcast_to(np.asarray(nodal_mass, dtype=np.float64), m.shape)
    return m


def _nodes_with_a_free_dof(model) -> np.ndarray:
    free = np.ones(model.ndof, dtype=bool)
    free[np.asarray(model.fixed_dofs, dtype=int)] = False
    return free.reshape(model.nnode, model.dimension).any(axis=1)


def cable_mask(model, cable_elements) -> Optional[np.ndarray]:
    """DynamicsConfig.cable_elements as a bool [n_elems], or None where nothing is flagged (None, an empty list).  Anything
    else than "all" or a list of distinct element ids is a ValueError."""
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


def check_dynamics(model, config: SolverConfig, dyn: DynamicsConfig) -> np.ndarray:
    """Everything solve_dynamic refuses, as a ValueError before an engine is built.  Returns the node masses."""
    if check_kinematics(config.kinematics) != "green-lagrange":
        raise ValueError("solve_dynamic needs kinematics 'green-lagrange': the time integration is built on the "
                         "total-Lagrangian element")
    if model.material.has_trainable_params():
        raise ValueError("solve_dynamic with NN materials is not supported: the dynamics read scalar E, A and density")
    if _world_size() > 1:
        raise ValueError("solve_dynamic does not support a sharded (multi-GPU) run.")
    if (dyn.t_end is None) == (dyn.n_steps is None):
        raise ValueError("DynamicsConfig needs exactly one of t_end and n_steps")
    if dyn.n_steps is not None and int(dyn.n_steps) < 1:
        raise ValueError(f"n_steps must be at least 1, got {dyn.n_steps}")
    if dyn.t_end is not None and not (math.isfinite(dyn.t_end) and dyn.t_end > 0.0):
        raise ValueError(f"t_end must be positive and finite, got {dyn.t_end}")
    if dyn.dt is not None and not (math.isfinite(dyn.dt) and dyn.dt > 0.0):
        raise ValueError(f"dt must be positive and finite, got {dyn.dt}")
    if not (math.isfinite(dyn.dt_safety) and 0.0 < dyn.dt_safety <= 1.0):
        raise ValueError(f"dt_safety must be in (0, 1], got {dyn.dt_safety}")
    if not (math.isfinite(dyn.damping) and dyn.damping >= 0.0):
        raise ValueError(f"damping must not be negative, got {dyn.damping}")
    if not (math.isfinite(dyn.ramp_time) and dyn.ramp_time >= 0.0):
        raise ValueError(f"ramp_time must not be negative, got {dyn.ramp_time}")
    if int(dyn.record_every) < 1:
        raise ValueError(f"record_every must be at least 1, got {dyn.record_every}")
    if dyn.record_dofs is not None:
        dofs = np.asarray(dyn.record_dofs)
        if dofs.ndim != 1 or dofs.dtype.kind not in "iu" or (dofs.size and (dofs.min() < 0 or dofs.max() >= model.ndof)):
            raise ValueError(f"record_dofs must be a list of dofs in 0..{model.ndof - 1}")
    if dyn.rest_tolerance is not None and not (math.isfinite(dyn.rest_tolerance) and dyn.rest_tolerance >= 0.0):
        raise ValueError(f"rest_tolerance must not be negative, got {dyn.rest_tolerance}")
    nodal = dyn.nodal_mass
    if nodal is not None:
        try:
            arr = np.asarray(nodal, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"nodal_mass must be a number or {model.nnode} numbers (one for each node)") from None
        if arr.ndim > 1 or (arr.ndim == 1 and arr.size != model.nnode) or not np.all(np.isfinite(arr)) or np.any(arr < 0.0):
            raise ValueError(f"nodal_mass must be a non-negative number or {model.nnode} of them (one for each node)")
    cable_mask(model, dyn.cable_elements)
    if not float(model.material.density.value()) > 0.0 and nodal is None:
        raise ValueError("solve_dynamic needs a positive material density or a nodal_mass: the structure has no mass")
    mass = lumped_mass(model, nodal)
    bad = np.flatnonzero(_nodes_with_a_free_dof(model) & ~(mass > 0.0))
    if bad.size:
        raise ValueError(f"node {int(bad[0])} has a free dof and no mass ({bad.size} such node{'s' if bad.size > 1 else ''}): "
                         "an explicit step divides by it")
    return mass


def omega_bound(model, strain: np.ndarray, e0, mass: np.ndarray, cable=None) -> float:
    """Upper bound of the highest frequency of K_t v = omega^2 M v from the strains of a gl_state: beta_e, the larger
    absolute eigenvalue of the element block B = (E*A / l0^3) d d^T + (N / l0) I, is the larger of |N / l0| and
    |N / l0 + E*A |d|^2 / l0^3| with |d|^2 = l0^2 (1 + 2 e), and v^T K_t v <= sum_e 2 beta_e (|v_i|^2 + |v_j|^2), so
    omega^2 <= max_i 2 sum_{e at i} beta_e / m_i over the nodes that have a free dof.
    cable: bool [n_elems], the tension-only elements.  Their beta is evaluated with e replaced by max(e, e0): a slack
    element counts with its taut, stress-free block E*A (1 + 2 e0) / l0, the largest its block is anywhere between its
    slack state and e0, so the bound holds through the steps in which it snaps taut, before the next record point
    re-evaluates it.  It is never below the bound of the elements that carry force now."""
    X = np.asarray(model.nodes, dtype=np.float64).reshape(model.nnode, model.dimension)
    el = np.asarray(model.elements, dtype=np.int64).reshape(-1, 2)
    l0 = np.linalg.norm(X[el[:, 1]] - X[el[:, 0]], axis=1)
    ea = float(np.float32(model.material.young.value())) * float(np.float32(model.material.area.value()))
    if cable is not None:
        strain = np.where(cable, np.maximum(strain, 0.0 if e0 is None else e0), strain)
    n_l0 = ea * (strain - (0.0 if e0 is None else e0)) / l0
    beta = np.maximum(np.abs(n_l0), np.abs(n_l0 + ea * (1.0 + 2.0 * strain) / l0))
    s = np.zeros(model.nnode)
    np.add.at(s, el[:, 0], beta)
    np.add.at(s, el[:, 1], beta)
    pick = _nodes_with_a_free_dof(model)
    return float(np.sqrt(np.max(2.0 * s[pick] / mass[pick]))) if pick.any() else 0.0


def stable_time_step(model, config: SolverConfig, u=None, nodal_mass=None, safety: float = 0.9, cable_elements=None) -> float:
    """safety * 2 / omega_bound at the displacements u (None: the undeformed state), with config.initial_strain and the
    tension-only elements cable_elements (as DynamicsConfig's)."""
    e0_np = check_initial_strain(config, model)
    cable = cable_mask(model, cable_elements)
    s = _newton_setup(model, e0_np, u)
    strain = s.eng.gl_state(s.u, None, s.e0).cpu().numpy()
    return safety * 2.0 / omega_bound(model, strain, e0_np, lumped_mass(model, nodal_mass), cable)


def solve_dynamic(model, config: SolverConfig, dyn: DynamicsConfig, u_initial=None, v_initial=None) -> DynamicsResult:
    """Integrate M a + alpha M v + f_int(u) = lam(t) F from (u_initial, v_initial) at t = 0 (None: zeros) by central
    differences.  The half kick of pf_gl_dyn_start turns v_initial into v_{1/2}; every later step is one launch, and a record
    interval is one replay of a hipGraph.  At every record point the energies are read (pf_gl_dyn_energy) and the bound on
    the highest frequency is re-evaluated at the current state: a dt above 2 / omega_bound raises RuntimeError naming the
    time, and so does a non-finite energy.  config.initial_strain is the e0 of every element, as in solve_nr.
    dyn.cable_elements are tension-only: slack (e - e0 < 0) they carry nothing, in the steps, the energies, the closing
    residual, the reactions and the axial forces; every record counts them ("slack_elements") and DynamicsResult.slack names
    those of the last step."""
    mass = check_dynamics(model, config, dyn)
    e0_np = check_initial_strain(config, model)
    cable = cable_mask(model, dyn.cable_elements)
    s = _newton_setup(model, e0_np, u_initial)
    eng, dev, ndof = s.eng, s.eng.device, model.ndof
    v0 = torch.zeros(ndof, dtype=torch.float64, device=dev)
    if v_initial is not None:
        v0 = torch.as_tensor(np.asarray(v_initial, dtype=np.float64).reshape(-1)).to(dev).clone()
        if v0.numel() != ndof:
            raise ValueError(f"v_initial has {v0.numel()} entries, the model has {ndof} dofs")
        v0[~s.free_t] = 0.0
    # 1 / m per dof; a node without a free dof may have no mass: its dofs never move
    minv_nodes = np.where(mass > 0.0, 1.0 / np.where(mass > 0.0, mass, 1.0), 0.0)
    minv = torch.from_numpy(np.repeat(minv_nodes, model.dimension)).to(dev)

    def strains_at(u):
        return eng.gl_state(u, None, s.e0).cpu().numpy()

    def bound_at(u):
        return omega_bound(model, strains_at(u), e0_np, mass, cable)

    def slack_at(strain):
        """The slack rule on host strains: the device's own decision, e - e0 < 0 with the same subtraction."""
        if cable is None:
            return np.zeros(model.nelm, dtype=bool)
        return cable & ((strain - e0_np if e0_np is not None else strain) < 0.0)

    w0 = bound_at(s.u)
    if not (math.isfinite(w0) and w0 > 0.0):
        raise RuntimeError("solve_dynamic: the structure has no stiffness at the initial state (omega_bound = "
                           f"{w0:g}); give dt explicitly")
    dt = float(dyn.dt) if dyn.dt is not None else dyn.dt_safety * 2.0 / w0
    n_steps = int(dyn.n_steps) if dyn.n_steps is not None else max(1, int(math.ceil(dyn.t_end / dt - 1e-9)))
    every = int(dyn.record_every)
    dofs = np.arange(ndof) if dyn.record_dofs is None else np.asarray(dyn.record_dofs, dtype=np.int64)
    dofs_t = torch.from_numpy(dofs).to(dev)
    lam0, lam1, t_ramp = float(dyn.load_factor_initial), float(dyn.load_factor_final), float(dyn.ramp_time)

    def lam_at(t):
        return lam0 + (lam1 - lam0) * min(1.0, t / t_ramp) if t_ramp > 0.0 else lam1

    times, recorded, energies = [], [], []
    kin_max = 0.0

    def record(n, u, kin, strain_e, work, vmax, wb, n_slack=None):
        nonlocal kin_max
        t = n * dt
        if not all(math.isfinite(x) for x in (kin, strain_e, work, vmax)):
            raise RuntimeError(f"solve_dynamic: non-finite energies at t = {t:.6g} (step {n}): the integration has diverged")
        if dt * wb > 2.0:
            raise RuntimeError(f"solve_dynamic: the time step {dt:.6g} is above the stability limit 2 / omega_bound = "
                               f"{2.0 / wb:.6g} at t = {t:.6g} (step {n})")
        lam = lam_at(t)
        times.append(t)
        recorded.append(u[dofs_t].cpu().numpy())
        energies.append(dict(kinetic=kin, strain=strain_e, work=lam * work, total=kin + strain_e - lam * work,
                             max_velocity=vmax, omega_bound=wb, load_factor=lam))
        if cable is not None:
            energies[-1]["slack_elements"] = int(n_slack)
        kin_max = max(kin_max, kin)

    # the initial state: the start has not run yet, so its kinetic energy is that of v_initial
    eng.dyn_begin(s.u, v0, minv, dt, float(dyn.damping), lam0, lam1, t_ramp, None, s.e0, start=False, cable=cable)
    record(0, s.u, *eng.dyn_energy(), w0, None if cable is None else slack_at(strains_at(s.u)).sum())
    eng.dyn_begin(s.u, v0, minv, dt, float(dyn.damping), lam0, lam1, t_ramp, None, s.e0, start=True, cable=cable)
    done, at_rest = 1, False
    while True:
        target = min(n_steps, (done // every + 1) * every)
        while done < target:
            k = min(GRAPH_STEPS, target - done)
            eng.dyn_steps(k)
            done += k
        u, v, n = eng.dyn_state()
        assert n == done
        record(done, u, *eng.dyn_energy(), bound_at(u), None if cable is None else eng.dyn_slack_count())
        if dyn.rest_tolerance is not None and energies[-1]["kinetic"] <= dyn.rest_tolerance * kin_max:
            at_rest = True
            break
        if done >= n_steps:
            break
    lam_end = lam_at(done * dt)
    strain = eng.gl_state(u, None, s.e0)
    slack = slack_at(strain.cpu().numpy())
    if slack.any():
        # the slack rule in the closing state: E*A = 0 on the slack elements gives fe == 0 there
        ea = float(np.float32(model.material.young.value())) * float(np.float32(model.material.area.value()))
        strain = eng.gl_state(u, torch.from_numpy(np.where(slack, 0.0, ea)).to(dev), s.e0)
    f_int = eng.gl_fint()
    out = (f_int - lam_end * s.loads).cpu().numpy()
    residual = float(np.max(np.abs(out[s.free]))) if s.free.any() else 0.0
    reactions = np.where(s.free, 0.0, out)
    axial = np.where(slack, 0.0, _axial_forces(model, strain, 0.0 if e0_np is None else e0_np))
    shape = (-1, 1) if model.dimension == 1 else (model.nnode, model.dimension)
    return DynamicsResult(times=np.array(times), recorded=np.array(recorded), energies=energies,
                          displacements=u.cpu().numpy().reshape(shape), velocities=v.cpu().numpy().reshape(shape),
                          axial_forces=axial, reactions=reactions.reshape(shape), residual_norm=residual, dt=dt, steps=done,
                          at_rest=at_rest, slack=slack)
