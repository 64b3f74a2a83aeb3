"""Explicit dynamics of Green-Lagrange trusses: central differences with a lumped mass and
mass-proportional damping, one kernel launch per time step (pf_gl_dyn_*), thousands of steps replayed as a hipGraph.

    m_i = sum_{e at i} rho A l0_e / 2 (+ nodal_mass), the same for every dof of the node
    v_{n+1/2} = c1 v_{n-1/2} + g (lam(t_n) F - f_int(u_n)) / m,   u_{n+1} = u_n + dt v_{n+1/2}
    c1 = (1 - alpha dt/2) / (1 + alpha dt/2),  g = dt / (1 + alpha dt/2),  lam(t) = lam0 + (lam1 - lam0) min(1, t / t_ramp)

It follows a structure through a limit point of the load, where solve_nr refuses the step, and it is what reads
Material.density.  Scalar materials, one GPU, dimension 1 and 2.

Tension-only (cable) elements, DynamicsConfig.cable_elements: a flagged element with e - e0 < 0 is slack and carries N = 0, no
force and no strain energy (pf_gl_dyn_*_cable).  A damped run with rest_tolerance comes to rest on the equilibrium of the
structure without its slack elements (solve_nr with SolverConfig.cable_elements reaches it by an active-set Newton iteration;
where DynamicsConfig.cable_elements is None, solve_dynamic takes the cables flagged there).

Time histories, DynamicsConfig.load_history and .support_motion: lam(t) and the scale s(t) of prescribed support displacements
u[dof](t) = amplitude s(t), each a table (piecewise linear) or a callable.  The host samples them once at the step times
t_n = n dt, 16 bytes per step for the two, and the step reads its samples by the step number of the device clock
(pf_gl_dyn_*_hist): no search on the device, and a replayed graph reads the samples of the steps it stands at.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np
import torch

from .solver import (SolverConfig, _axial_forces, _newton_setup, _world_size, cable_mask, check_initial_strain,  # noqa: F401
                     check_kinematics)

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
    cable_elements: Optional[object] = None     # the tension-only elements: "all" or a list of element ids; None: those of
                                            # SolverConfig.cable_elements; [] (or None there too): all bars
    load_history: Optional[object] = None   # lam(t) in place of the ramp: a pair (times, values) or a callable (history_samples);
                                            # ramp_time and load_factor_initial / _final must then be at their defaults
    support_motion: Optional["SupportMotion"] = None    # fixed dofs that follow a prescribed displacement


@dataclass
class SupportMotion:
    """u[dof](t) = amplitude * s(t) on the listed fixed dofs."""
    dofs: List[int]                         # distinct dofs, every one of them in model.fixed_dofs
    amplitudes: object                      # a number, or one for each of dofs
    history: object                         # s(t): a pair (times, values) or a callable, as DynamicsConfig.load_history


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


def dynamic_cables(model, config: SolverConfig, dyn: "DynamicsConfig") -> Optional[np.ndarray]:
    """The tension-only elements of a dynamic run as cable_mask's bool [n_elems] or None: dyn.cable_elements when it is
    given, otherwise config.cable_elements, so a structure's cables are flagged once.  Both given and different is a
    ValueError."""
    own = cable_mask(model, dyn.cable_elements)
    inherited = cable_mask(model, getattr(config, "cable_elements", None))
    if dyn.cable_elements is None:
        return inherited
    if getattr(config, "cable_elements", None) is not None and not np.array_equal(
            np.zeros(model.nelm, dtype=bool) if own is None else own,
            np.zeros(model.nelm, dtype=bool) if inherited is None else inherited):
        raise ValueError("DynamicsConfig.cable_elements and SolverConfig.cable_elements name different elements: give the "
                         "cables once, or the same set twice")
    return own


def history_samples(history, t: np.ndarray, what: str = "history") -> np.ndarray:
    """A time history at the times t (float64 [n]) as float64 [n].
    A pair (times, values): times strictly increasing, the history piecewise linear between the knots,
    v_j + (v_{j+1} - v_j) ((t - t_j) / (t_{j+1} - t_j)) for t_j < t < t_{j+1}, the knot's own value at a knot, the first value
    before the first knot and the last value after the last.  A callable: called once with t, it returns an array of t's
    shape.  Anything else, and any value that is not finite, is a ValueError naming `what`."""
    t = np.asarray(t, dtype=np.float64)
    if callable(history):
        try:
            out = np.asarray(history(t.copy()), dtype=np.float64)
        except (TypeError, ValueError) as err:
            raise ValueError(f"{what}: the callable did not return numbers ({err})") from None
        if out.shape != t.shape:
            raise ValueError(f"{what}: the callable returned the shape {out.shape} for times of the shape {t.shape}")
        if not np.all(np.isfinite(out)):
            raise ValueError(f"{what}: the callable returned a value that is not finite")
        return np.ascontiguousarray(out)
    try:
        times, values = history
        times, values = np.asarray(times, dtype=np.float64), np.asarray(values, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be a pair (times, values) or a callable") from None
    if times.ndim != 1 or values.ndim != 1 or times.size < 1 or times.size != values.size:
        raise ValueError(f"{what}: times and values must be two lists of one length, at least 1, got the shapes "
                         f"{times.shape} and {values.shape}")
    if not (np.all(np.isfinite(times)) and np.all(np.isfinite(values))):
        raise ValueError(f"{what}: times and values must be finite")
    if np.any(np.diff(times) <= 0.0):
        raise ValueError(f"{what}: times must be strictly increasing")
    if times.size == 1:
        return np.full(t.shape, values[0])
    j = np.clip(np.searchsorted(times, t, side="right") - 1, 0, times.size - 2)         # t_j <= t < t_{j+1} inside the table
    out = values[j] + (values[j + 1] - values[j]) * ((t - times[j]) / (times[j + 1] - times[j]))
    out = np.where(t == times[j], values[j], out)
    return np.where(t <= times[0], values[0], np.where(t >= times[-1], values[-1], out))


def support_amplitudes(model, motion) -> np.ndarray:
    """SupportMotion's dofs and amplitudes as the amplitude of every dof, float64 [n_dofs] (0.0: the dof is not moved).
    Anything malformed is a ValueError."""
    if not isinstance(motion, SupportMotion):
        raise ValueError("support_motion must be a SupportMotion(dofs, amplitudes, history)")
    try:
        dofs = np.asarray(motion.dofs)
        amp = np.asarray(motion.amplitudes, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("support_motion: dofs must be a list of dofs and amplitudes a number or a list of numbers") from None
    if dofs.ndim != 1 or dofs.size < 1 or dofs.dtype.kind not in "iu":
        raise ValueError("support_motion: dofs must be a list of at least one integer dof")
    if np.unique(dofs).size != dofs.size:
        raise ValueError("support_motion names a dof twice")
    loose = np.setdiff1d(dofs, np.asarray(model.fixed_dofs, dtype=np.int64))
    if loose.size:
        raise ValueError(f"support_motion: dof {int(loose[0])} is not in fixed_dofs: only a support can be moved")
    if amp.ndim > 1 or (amp.ndim == 1 and amp.size != dofs.size):
        raise ValueError(f"support_motion: amplitudes must be a number or {dofs.size} numbers (one for each of dofs)")
    if not np.all(np.isfinite(amp)):
        raise ValueError("support_motion: amplitudes must be finite")
    out = np.zeros(model.ndof)
    out[dofs.astype(np.int64)] = amp
    return out


# the times check_dynamics tries a callable history on, before the step times are known
_PROBE_TIMES = np.array([0.0, 0.5, 1.0])


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
    dynamic_cables(model, config, dyn)
    if getattr(config, "yield_strain", None) is not None:
        raise ValueError("solve_dynamic does not support yield_strain: the step kernels are elastic and would silently "
                         "answer for the structure that never yields.")
    if dyn.load_history is not None:
        if (dyn.ramp_time, dyn.load_factor_initial, dyn.load_factor_final) != (0.0, 0.0, 1.0):
            raise ValueError("load_history takes the place of the ramp: ramp_time, load_factor_initial and load_factor_final "
                             "must be left at their defaults")
        history_samples(dyn.load_history, _PROBE_TIMES, "load_history")
    if dyn.support_motion is not None:
        support_amplitudes(model, dyn.support_motion)
        history_samples(dyn.support_motion.history, _PROBE_TIMES, "support_motion.history")
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
    those of the last step.
    dyn.load_history takes the place of the ramp and dyn.support_motion moves fixed dofs, u[dof](t) = amplitude s(t).  Both are
    sampled once, at t_n = n dt for n = 0 .. n_steps + 1 (history_samples; a callable is called once with all of them, after
    check_dynamics has tried it on three times of its own), 16 bytes per step for the two, and the steps read the samples by
    their number; the records' load_factor and work, and the load factor of the closing residual and reactions, are those
    samples.  u_initial on a moved dof is replaced by amplitude s(0).  With support motion the recorded `total` is not a
    conserved quantity: the supports do work on the structure, and their own kinetic energy is not counted (v stays 0 on a
    fixed dof)."""
    mass = check_dynamics(model, config, dyn)
    e0_np = check_initial_strain(config, model)
    cable = dynamic_cables(model, config, dyn)
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

    # the histories at the step times: step n reads sample n, and writes the supports of step n + 1
    t_samples = np.arange(n_steps + 2, dtype=np.float64) * dt
    lam_samples = None if dyn.load_history is None else history_samples(dyn.load_history, t_samples, "load_history")
    support = None
    if dyn.support_motion is not None:
        amp = support_amplitudes(model, dyn.support_motion)
        support = (amp, history_samples(dyn.support_motion.history, t_samples, "support_motion.history"))
        moved = amp != 0.0
        s.u[torch.from_numpy(moved).to(dev)] = torch.from_numpy(amp[moved] * support[1][0]).to(dev)
    hist = dict(load_samples=lam_samples, support=support)

    def lam_at(n):
        if lam_samples is not None:
            return float(lam_samples[min(n, n_steps + 1)])
        t = n * dt
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
        lam = lam_at(n)
        times.append(t)
        recorded.append(u[dofs_t].cpu().numpy())
        energies.append(dict(kinetic=kin, strain=strain_e, work=lam * work, total=kin + strain_e - lam * work,
                             max_velocity=vmax, omega_bound=wb, load_factor=lam))
        if cable is not None:
            energies[-1]["slack_elements"] = int(n_slack)
        kin_max = max(kin_max, kin)

    # the initial state: the start has not run yet, so its kinetic energy is that of v_initial
    eng.dyn_begin(s.u, v0, minv, dt, float(dyn.damping), lam0, lam1, t_ramp, None, s.e0, start=False, cable=cable, **hist)
    record(0, s.u, *eng.dyn_energy(), w0, None if cable is None else slack_at(strains_at(s.u)).sum())
    eng.dyn_begin(s.u, v0, minv, dt, float(dyn.damping), lam0, lam1, t_ramp, None, s.e0, start=True, cable=cable, **hist)
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
    lam_end = lam_at(done)
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
