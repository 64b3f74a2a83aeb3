"""Explicit dynamics of Green-Lagrange trusses, CPU side: the float64 restatement of tests/gl_dynamics_reference.py pinned
to closed forms (the taut string's frequencies, the two-bar truss's far equilibrium), the stability bound against the true
highest frequency, the host code of pinn_fem_amd/fem/dynamics.py (masses, bound, every refusal) against the restatement,
and the JSON / CLI / ABI surface.  tests/test_gl_dynamics_f64.py holds the device to the same restatement.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gl_dynamics_reference as gd
import gl_reference as gl
from device_driver import irregular_truss_with_supports
from helpers import ROOT
from pinn_fem_amd.fem import dynamics as dyn
from pinn_fem_amd.fem.model import FEMModel, Material
from pinn_fem_amd.fem.solver import SolverConfig

HERE = os.path.dirname(os.path.abspath(__file__))
EA, YOUNG, AREA = 1000.0, 2000.0, 0.5


def irregular(rho_a=1.0, load_seed=None):
    """The 257-element irregular truss of the device tests (121 nodes, hubs of odd and even degree) as a gd.Truss."""
    nodes, el, fixed = irregular_truss_with_supports(257, np.random.default_rng(1257))
    loads = None if load_seed is None else np.random.default_rng(load_seed).standard_normal(nodes.size)
    return gd.Truss(nodes, el, fixed, 2, EA, None, gd.lumped_mass(nodes, el, rho_a, 2), loads)


def _model(T, density, e0=None, loads=None):
    return FEMModel(nodes=T.X, elements=T.el, material=Material(YOUNG, AREA, density),
                    loads=np.zeros(T.n) if loads is None else loads, fixed_dofs=np.flatnonzero(~T.free), dimension=2)


def _config(**kw):
    return SolverConfig(method="nr", kinematics="green-lagrange", **kw)


# ---------------------------------------------------------------------------------------------------------------------
# the bound
# ---------------------------------------------------------------------------------------------------------------------
def test_mesh_has_hubs_of_odd_and_even_degree():
    T = irregular()
    assert T.n_nodes == 121 and T.ne == 257
    high = T.degree[::2][T.degree[::2] >= 5]
    assert (high % 2 == 1).any() and (high % 2 == 0).any()


@pytest.mark.parametrize("which", ["string", "truss"])
def test_bound_is_above_the_true_highest_frequency(which):
    """omega_bound >= omega_max of K_t v = omega^2 M v (scipy.linalg.eigvalsh), at rest and at a deformed state; on the
    8-element string 357.95 against 351.07.  The package's host bound, fed the restatement's strains, is the restatement's."""
    T = gd.string()[0] if which == "string" else irregular()
    rng = np.random.default_rng(5)
    for u in (np.zeros(T.n), np.where(T.free, 0.05 * rng.standard_normal(T.n), 0.0)):
        bound, true = T.omega_bound(u), T.omega_true(u)
        print(f"{which}: bound {bound:.4f}, true {true:.4f}")
        assert true <= bound <= 3.0 * true
        e0 = None if which == "truss" else T.e0
        model = _model(T, 1.0 if which == "string" else 2.0)
        mass = dyn.lumped_mass(model)
        assert np.allclose(np.repeat(mass, 2), T.mass, rtol=1e-15, atol=0.0)
        assert dyn.omega_bound(model, T.strain(u)[0], e0, mass) == pytest.approx(bound, rel=1e-13)
    if which == "string":
        assert T.omega_bound(np.zeros(T.n)) == pytest.approx(357.95, abs=5e-3)
        assert T.omega_true(np.zeros(T.n)) == pytest.approx(351.07, abs=5e-3)


@pytest.mark.parametrize("which", ["string", "truss"])
def test_step_above_the_true_limit_diverges_and_the_safe_one_does_not(which):
    """From a random field of 1e-6: 300 steps of 1.05 * 2 / omega_true grow it by more than 1e6 (or to a non-finite value), 2000
    steps of 0.9 * 2 / omega_bound keep it within 1e3 of where it started (the energy is conserved, a soft mode may take it)."""
    T = gd.string()[0] if which == "string" else irregular()
    u0 = np.where(T.free, 1e-6 * np.random.default_rng(6).standard_normal(T.n), 0.0)
    zero = np.zeros(T.n)
    with np.errstate(all="ignore"):
        u, _ = T.run(u0, zero, 0, 300, 1.05 * 2.0 / T.omega_true(zero))
    growth = np.max(np.abs(u)) / np.max(np.abs(u0))
    print(f"{which}: growth above the limit {growth:.3e}")
    assert not np.isfinite(growth) or growth > 1e6
    u, _ = T.run(u0, zero, 0, 2000, T.stable_time_step(zero, 0.9))
    growth = np.max(np.abs(u)) / np.max(np.abs(u0))
    print(f"{which}: growth at 0.9 of the bound {growth:.3e}")
    assert np.isfinite(growth) and growth < 1e3


# ---------------------------------------------------------------------------------------------------------------------
# the taut string
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k, n_expected", [(1, 567), (3, 199)])
def test_taut_string_returns_after_one_discrete_period(k, n_expected):
    """8 elements on [-1, 1], E*A = 1000, e0 = -1e-3 (T = 1), rho A = 0.5: mode k has omega_k = 2 sqrt(T / (m h)) sin(k pi / 16).
    With N = ceil(period / (0.9 * 2 / omega_bound)) steps of dt = 2 sin(pi / N) / omega_k, the discrete period, and
    v_{-1/2} = u_0 (1 - cos(2 pi / N)) / dt the linear scheme returns exactly; at a = 1e-5 the restatement misses by 3.8e-6 a
    (k = 1) and 5.9e-6 a (k = 3), the quadratic axial coupling.  The half kick from v_0 = 0 is the same orbit.  With the
    tension doubled the same run misses by 1.86 a: the frequency is the tension's."""
    a = 1e-5
    T, h, tension = gd.string()
    zero = np.zeros(T.n)
    omega = gd.string_frequency(k, 8, tension, T.mass[3], h)
    N = int(np.ceil(2.0 * np.pi / omega / (0.9 * 2.0 / T.omega_bound(zero))))
    assert N == n_expected
    dt = 2.0 * np.sin(np.pi / N) / omega
    u0 = gd.string_mode(k, 8, a)
    v = u0 * (1.0 - np.cos(2.0 * np.pi / N)) / dt
    u, _ = T.run(u0, v, 0, N, dt)
    miss = np.max(np.abs(u - u0)) / a
    u1, vh = T.start(u0, zero, dt)
    u, _ = T.run(u1, vh, 1, N - 1, dt)
    miss_start = np.max(np.abs(u - u0)) / a
    doubled = gd.string(e0=-2e-3)[0]
    u, _ = doubled.run(u0, v, 0, N, dt)
    miss_doubled = np.max(np.abs(u - u0)) / a
    print(f"mode {k}: {N} steps, miss {miss:.3e} a, from the half kick {miss_start:.3e} a, tension doubled {miss_doubled:.3f} a")
    assert miss <= 1e-5 and miss_start <= 1e-5 and miss_doubled > 1.0


# ---------------------------------------------------------------------------------------------------------------------
# the two-bar truss through its limit point
# ---------------------------------------------------------------------------------------------------------------------
def two_bar_snap():
    """b = 1, h = 0.1, E*A = 1000, rho A = 1, a step load of 1.5 times the limit load, alpha = the linear apex frequency,
    dt = half the bound.  Returns (TwoBar, Truss, load, alpha, dt)."""
    tb = gl.TwoBar(a=1.0, h=0.1, ea=EA)
    load = 1.5 * tb.p_lim
    T = gd.Truss(tb.nodes, tb.el, tb.fixed, 2, EA, None, gd.lumped_mass(tb.nodes, tb.el, 1.0, 2), tb.loads(load))
    alpha = float(np.sqrt(tb.tangent(0.0) / T.mass[5]))
    return tb, T, load, alpha, 0.5 * 2.0 / T.omega_bound(np.zeros(6))


def test_two_bar_snaps_to_the_far_root():
    """20 000 steps end beyond w = 2 h on the far root of P(w) = load to 1e-12 of h (the restatement: 5.6e-16 h, residual
    2.8e-15): a state load control refuses, since the load is above the limit load."""
    tb, T, load, alpha, dt = two_bar_snap()
    zero = np.zeros(6)
    u, v = T.start(zero, zero, dt, alpha=alpha)
    u, v = T.run(u, v, 1, 19999, dt, alpha=alpha)
    w, far = -u[5], gd.two_bar_far_root(tb, load)
    residual = np.max(np.abs((T.loads - T.f_int(u))[T.free]))
    print(f"two-bar: w = {w:.15f}, far root {far:.15f}, miss {abs(w - far) / tb.h:.2e} h, residual {residual:.2e}")
    assert load > tb.p_lim and far > 2.0 * tb.h
    assert abs(w - far) <= 1e-12 * tb.h and abs(u[4]) <= 1e-12 * tb.h and residual <= 1e-12 * load


def test_heavy_damping_approaches_the_static_solution_monotonically():
    """Below the limit load with alpha = 4 times the linear apex frequency (overdamped): the apex drop grows at every step,
    never passes the static solution and ends on it."""
    tb, _, _, alpha, dt = two_bar_snap()
    load = 0.5 * tb.p_lim
    T = gd.Truss(tb.nodes, tb.el, tb.fixed, 2, EA, None, gd.lumped_mass(tb.nodes, tb.el, 1.0, 2), tb.loads(load))
    u_static, _, ok = gl.newton(tb.nodes, tb.el, tb.loads(load), tb.fixed, EA, 2, tol=1e-14)
    assert ok
    zero = np.zeros(6)
    u, v = T.start(zero, zero, dt, alpha=4.0 * alpha)
    drops = [0.0, -u[5]]
    for n in range(1, 6000):
        u, v = T.step(u, v, n, dt, alpha=4.0 * alpha)
        drops.append(-u[5])
    drops, w = np.array(drops), -u_static[5]
    print(f"overdamped: static drop {w:.6e}, last {drops[-1]:.6e}")
    assert np.all(np.diff(drops) >= -1e-15 * w) and np.all(drops <= w * (1.0 + 1e-12))
    assert abs(drops[-1] - w) <= 1e-9 * w


# ---------------------------------------------------------------------------------------------------------------------
# energy
# ---------------------------------------------------------------------------------------------------------------------
def energy_band(T, n_steps, fraction):
    """(largest |total - total_0| over the run, largest |f.u|) of a step load from rest, total = kinetic + strain - f.u."""
    zero = np.zeros(T.n)
    dt = fraction * 2.0 / T.omega_bound(zero)
    u, v = T.start(zero, zero, dt)
    totals, works = [], []
    for n in range(1, n_steps + 1):
        kin, strain, work, _ = T.energies(u, v)
        totals.append(kin + strain - work)
        works.append(abs(work))
        u, v = T.step(u, v, n, dt)
    return float(np.max(np.abs(np.array(totals)))), float(np.max(works))


def test_undamped_energy_stays_within_the_band():
    """A step load (standard normal on every dof) on the irregular truss from rest, 512 steps at 0.8 of the bound.  The
    total kinetic + strain - f.u starts at 0; with the velocity half a step behind the displacement it is conserved only
    to O(dt^2).  Measured on the CPU with these loads: 7.11e-3 of the largest |f.u| (2.30e-2 against 3.24); asserted with
    a margin of 2, 1.43e-2."""
    band, work = energy_band(irregular(load_seed=7), 512, 0.8)
    print(f"energy band {band:.3e}, largest |f.u| {work:.3e}, ratio {band / work:.3e}")
    assert band <= 1.43e-2 * work


# ---------------------------------------------------------------------------------------------------------------------
# check_dynamics
# ---------------------------------------------------------------------------------------------------------------------
def test_check_dynamics_refusals(monkeypatch):
    T = gd.string()[0]
    model, good = _model(T, 1.0), dyn.DynamicsConfig(n_steps=10)
    assert np.allclose(np.repeat(dyn.check_dynamics(model, _config(), good), 2), T.mass)
    cases = [
        ("green-lagrange", model, SolverConfig(method="nr"), good),
        ("exactly one of t_end and n_steps", model, _config(), dyn.DynamicsConfig()),
        ("exactly one of t_end and n_steps", model, _config(), dyn.DynamicsConfig(n_steps=10, t_end=1.0)),
        ("n_steps must be at least 1", model, _config(), dyn.DynamicsConfig(n_steps=0)),
        ("t_end must be positive", model, _config(), dyn.DynamicsConfig(t_end=-1.0)),
        ("dt must be positive", model, _config(), dyn.DynamicsConfig(n_steps=10, dt=0.0)),
        ("dt must be positive", model, _config(), dyn.DynamicsConfig(n_steps=10, dt=float("nan"))),
        ("damping must not be negative", model, _config(), dyn.DynamicsConfig(n_steps=10, damping=-1.0)),
        ("ramp_time must not be negative", model, _config(), dyn.DynamicsConfig(n_steps=10, ramp_time=-1.0)),
        ("record_every must be at least 1", model, _config(), dyn.DynamicsConfig(n_steps=10, record_every=0)),
        ("record_dofs", model, _config(), dyn.DynamicsConfig(n_steps=10, record_dofs=[0, T.n])),
        ("record_dofs", model, _config(), dyn.DynamicsConfig(n_steps=10, record_dofs=[-1])),
        ("record_dofs", model, _config(), dyn.DynamicsConfig(n_steps=10, record_dofs=[0.5])),
        ("positive material density or a nodal_mass", _model(T, 0.0), _config(), good),
        ("positive material density or a nodal_mass", _model(T, -1.0), _config(), good),
        ("nodal_mass", model, _config(), dyn.DynamicsConfig(n_steps=10, nodal_mass=[1.0, 2.0])),
        ("nodal_mass", model, _config(), dyn.DynamicsConfig(n_steps=10, nodal_mass=-1.0)),
        ("has a free dof and no mass", _model(T, 0.0), _config(), dyn.DynamicsConfig(n_steps=10, nodal_mass=[1.0] * 4 + [0.0] * 5)),
        ("rest_tolerance", model, _config(), dyn.DynamicsConfig(n_steps=10, rest_tolerance=-1.0)),
    ]
    for match, m, c, d in cases:
        with pytest.raises(ValueError, match=match):
            dyn.check_dynamics(m, c, d)
    # a density of zero is fine when every node with a free dof is given a mass
    assert dyn.check_dynamics(_model(T, 0.0), _config(), dyn.DynamicsConfig(n_steps=10, nodal_mass=0.125)).min() == 0.125
    # NN materials
    import torch
    from pinn_fem_amd.fem.properties import NNProperty
    from pinn_fem_amd.nets import SimpleNN
    torch.manual_seed(0)
    young = NNProperty(net=SimpleNN(hidden_layers=2, neurons_per_layer=4, input_dim=3), input_dim=3, enforce_positive=True,
                       scale=YOUNG)
    nn_model = FEMModel(nodes=T.X, elements=T.el, material=Material(young, AREA, 1.0), loads=np.zeros(T.n),
                        fixed_dofs=np.flatnonzero(~T.free), dimension=2)
    with pytest.raises(ValueError, match="NN materials"):
        dyn.check_dynamics(nn_model, _config(), good)
    # a sharded run
    monkeypatch.setattr(dyn, "_world_size", lambda: 2)
    with pytest.raises(ValueError, match="sharded"):
        dyn.check_dynamics(model, _config(), good)


def test_solve_dynamic_checks_before_it_builds_an_engine():
    """Every refusal comes before the engine: without a GPU a refused call is a ValueError, never the engine's error."""
    T = gd.string()[0]
    with pytest.raises(ValueError, match="exactly one of"):
        dyn.solve_dynamic(_model(T, 1.0), _config(), dyn.DynamicsConfig())
    with pytest.raises(ValueError, match="initial_strain"):
        dyn.solve_dynamic(_model(T, 1.0), _config(initial_strain=[0.1, 0.2]), dyn.DynamicsConfig(n_steps=4))


# ---------------------------------------------------------------------------------------------------------------------
# JSON, CLI and ABI surface
# ---------------------------------------------------------------------------------------------------------------------
def test_json_inputs_parse_to_a_dynamics_block():
    from pinn_fem_amd import fem
    from pinn_fem_amd.cli import generic as g
    assert fem.solve_dynamic is dyn.solve_dynamic and fem.DynamicsConfig is dyn.DynamicsConfig
    p = g.parse_problem(os.path.join(HERE, "nl_inputs", "taut_string_vibration.json"))
    d = p["dynamics"]["config"]
    assert isinstance(d, dyn.DynamicsConfig) and d.n_steps == 567 and d.t_end is None and d.record_dofs == [9]
    assert p["solver_config"].kinematics == "green-lagrange" and p["solver_config"].initial_strain == -0.001
    T, h, tension = gd.string()
    assert d.dt == 2.0 * np.sin(np.pi / 567) / gd.string_frequency(1, 8, tension, T.mass[3], h)
    assert np.array_equal(np.array(p["dynamics"]["u_initial"]), gd.string_mode(1, 8, 1e-5)) and p["dynamics"]["v_initial"] is None
    assert np.allclose(np.repeat(dyn.check_dynamics(p["model"], p["solver_config"], d), 2), T.mass, rtol=1e-15)
    p = g.parse_problem(os.path.join(HERE, "nl_inputs", "two_bar_snap_dynamic.json"))
    d = p["dynamics"]["config"]
    tb, T, load, alpha, _ = two_bar_snap()
    assert d.n_steps == 20000 and d.dt is None and d.dt_safety == 0.5 and d.damping == alpha and d.rest_tolerance == 1e-12
    assert np.array_equal(p["model"].loads, tb.loads(load))
    assert np.allclose(np.repeat(dyn.check_dynamics(p["model"], p["solver_config"], d), 2), T.mass, rtol=1e-15)
    # without the key nothing changes
    assert "dynamics" not in g.parse_problem(os.path.join(HERE, "nl_inputs", "taut_string.json"))


def test_json_dynamics_block_is_checked(tmp_path):
    import json
    from pinn_fem_amd.cli import generic as g
    doc = json.load(open(os.path.join(HERE, "nl_inputs", "two_bar_snap_dynamic.json")))
    for block in ({"n_steps": 10, "steps": 3}, [1, 2], {"n_steps": "many"}):
        bad = dict(doc, accel=dict(doc["accel"], dynamics=block))
        (tmp_path / "bad.json").write_text(json.dumps(bad))
        with pytest.raises(ValueError, match="accel.dynamics"):
            g.parse_problem(str(tmp_path / "bad.json"))
    both = dict(doc, accel=dict(doc["accel"], identify_nr={"groups": None, "levels": []}))
    (tmp_path / "both.json").write_text(json.dumps(both))
    with pytest.raises(ValueError, match="both dynamics and an identification"):
        g.parse_problem(str(tmp_path / "both.json"))


def test_abi_surface():
    from pinn_fem_amd import _capi
    lib = _capi.load()
    names = ("pf_gl_dyn_start", "pf_gl_dyn_steps", "pf_gl_dyn_graph_create", "pf_gl_dyn_energy")
    header = open(os.path.join(ROOT, "include", "pinnfem_hip.h")).read()
    for name in names:
        assert re.search(r"^int " + name + r"\(", header, re.M) and name in _capi.SYMBOLS and hasattr(lib, name)
    assert lib.pf_abi_version() == 9
    assert lib.pf_sizeof(7) == C.sizeof(_capi.PfDyn) == 8 * 8 + 5 * 8
    assert [f[0] for f in _capi.PfDyn._fields_] == ["minv", "f_ext", "ea", "e0", "u0", "u1", "v", "clock", "dt", "alpha",
                                                    "lam0", "lam1", "t_ramp"]
    assert _capi.PF_DYN_ENERGY_COUNT == int(re.search(r"#define PF_MAX_NODE_BLOCKS (\d+)", header).group(1)) * 4 + 4


def test_argument_errors_are_rejected_on_the_host():
    """Null records and a bad mesh are PF_ERR_ARG with the function's name in front, before any HIP call: this runs without
    a GPU."""
    from pinn_fem_amd import _capi
    lib = _capi.load()
    p, g, d = _capi.PfProblem(), _capi.PfGl(), _capi.PfDyn()
    graph = C.c_void_p()
    calls = {"pf_gl_dyn_start": lambda: lib.pf_gl_dyn_start(C.byref(p), C.byref(g), C.byref(d), None),
             "pf_gl_dyn_steps": lambda: lib.pf_gl_dyn_steps(C.byref(p), C.byref(g), C.byref(d), 1, None),
             "pf_gl_dyn_graph_create": lambda: lib.pf_gl_dyn_graph_create(C.byref(p), C.byref(g), C.byref(d), 1, None, C.byref(graph)),
             "pf_gl_dyn_energy": lambda: lib.pf_gl_dyn_energy(C.byref(p), C.byref(g), C.byref(d), None, None)}
    for name, call in calls.items():
        assert call() == _capi.PF_ERR_ARG
        assert lib.pf_last_error().decode().startswith(name + ": bad mesh")
    assert not graph
