"""Tension-only (cable) elements in the explicit dynamics, without a GPU: the restatement tests/gl_cable_reference.py pinned to
closed forms (free flight, the bilinear oscillator, the guyed mast against Newton solves of the structure without its slack
guy), the stability bound with cables against a dense eigensolve, the host code of pinn_fem_amd/fem/dynamics.py pinned to the
restatement, and the surface: check_dynamics' refusals, the JSON forms and the C ABI.  The measured figures are printed in
front of every assertion.
"""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

import gl_cable_reference as gc
import gl_dynamics_reference as gd
import gl_reference as gl
from device_driver import irregular_truss_with_supports
from helpers import ROOT
from pinn_fem_amd.fem import dynamics as dyn
from pinn_fem_amd.fem.model import FEMModel, Material
from pinn_fem_amd.fem.solver import SolverConfig

HERE = os.path.dirname(os.path.abspath(__file__))
EA, YOUNG, AREA = 1000.0, 2000.0, 0.5
DT = 2.0 ** -10


def _config(**kw):
    return SolverConfig(method="nr", kinematics="green-lagrange", **kw)


def _model(T, density=1.0, loads=None):
    return FEMModel(nodes=T.X if T.dim == 2 else T.X.reshape(-1), elements=T.el, material=Material(YOUNG, AREA, density),
                    loads=T.loads if loads is None else loads, fixed_dofs=np.flatnonzero(~T.free), dimension=T.dim)


# ---------------------------------------------------------------------------------------------------------------------
# closed forms
# ---------------------------------------------------------------------------------------------------------------------
def test_free_flight_is_exact():
    """One slack cable under a load away from its support flies freely: u_n = -(F / m)(n dt)^2 / 2 to the bit (every factor a
    power of two: F / m = 4, dt = 2^-10), -0.0078125 after 64 steps and -0.125 after 256; |u| stays below l0 = 1, past which
    the 1-D element flips over and is taut again.  The same run as a bar is held back by the element."""
    T = gc.one_cable(-1.0)
    assert T.mass[1] == 0.25 and T.cable.all()
    zero = np.zeros(2)
    u1, v1 = T.start(zero, zero, DT)
    for n, want in ((64, -0.0078125), (256, -0.125)):
        u = T.run(u1, v1, 1, n - 1, DT)[0]
        print(f"free flight, {n} steps: u {u[1]!r}, closed form {want!r}")
        assert u[1] == want == -(1.0 / 0.25) * (n * DT) ** 2 / 2.0 and u[0] == 0.0 and T.slack(u).all()
        assert T.energies(u, v1)[1] == 0.0 and T.energies(u, v1)[4] == 1
    bar = gc.one_cable(-1.0)
    bar.cable[:] = False
    ub = bar.run(*bar.start(zero, zero, DT), 1, 255, DT)[0]
    print(f"the same run as a bar ends at {ub[1]:.3e}")
    assert abs(ub[1]) < 1e-2 and not bar.slack(ub).any()


def test_bilinear_oscillator_phases():
    """The same element under a load of +1 from v0 = -0.5: slack at once, back at u = 0 after 2 |v0| m / F = 0.25, then taut
    for 2 (pi - atan2(|v0| / omega, F / k)) / omega = 0.05367 with omega = sqrt(k / m), k = E A / l0 (the linear spring; the
    strain's quadratic term is 3e-3 of it here).  Both durations to within 2 dt, the granularity of detecting a change of
    state, over three periods."""
    T = gc.one_cable(1.0)
    m, k, f, v0 = 0.25, EA, 1.0, -0.5
    omega = math.sqrt(k / m)
    t_slack = 2.0 * abs(v0) * m / f
    t_taut = 2.0 * (math.pi - math.atan2(abs(v0) / omega, f / k)) / omega
    assert t_slack == 0.25 and abs(t_taut - 0.05367) < 5e-5
    zero = np.zeros(2)
    u1, v1 = T.start(zero, np.array([0.0, v0]), DT)
    assert T.slack(u1).all()                    # slack at once
    n_steps = int(3.2 * (t_slack + t_taut) / DT)
    _, _, at, ever = T.state_changes(u1, v1, 1, n_steps, DT)
    times = [0.0] + [n * DT for n in at]
    print("state changes at", [f"{t:.4f}" for t in times[1:]])
    assert len(at) >= 6 and ever.all()
    for i in range(6):
        duration, want = times[i + 1] - times[i], (t_slack if i % 2 == 0 else t_taut)
        print(f"phase {i} ({'slack' if i % 2 == 0 else 'taut'}): {duration:.5f}, closed form {want:.5f}")
        assert abs(duration - want) <= 2.0 * DT


def mast_run(T, dt=0.01, alpha=17.7, every=100, tol=1e-26, n_max=20000):
    """The damped run of guyed_mast_slack.json on the restatement, with solve_dynamic's rest rule."""
    zero = np.zeros(T.n)
    u, v = T.start(zero, zero, dt, alpha)
    n, kin_max = 1, 0.0
    while n < n_max:
        k = every - n % every
        u, v = T.run(u, v, n, k, dt, alpha=alpha)
        n += k
        kin = T.energies(u, v)[0]
        kin_max = max(kin_max, kin)
        if kin <= tol * kin_max:
            return u, n, True
    return u, n, False


@pytest.mark.parametrize("load", [2.0, 0.2])
def test_guyed_mast_rests_on_the_structure_without_its_slack_guy(load):
    """A mast with two pretensioned guys under a side load at the top, damped to rest.  Load 2.0: the leeward guy is slack, and
    the run ends on gl_reference.newton of the two-element structure without that guy to 1e-12 of max |u| (the Newton
    tolerance is 1e-10 with quadratic convergence) and more than 1e-2 from the all-bar Newton solution.  Load 0.2: nothing
    goes slack and the run ends on the all-bar solution.
    dt = 0.01, a tenth of the bound: the rest rule compares with the largest RECORDED kinetic energy, and at 0.9 of the bound
    the first record (step 100) comes after the motion has died down to 1e-9, so that 1e-26 of it is below what round-off of
    the residual lets the velocity reach (kinetic energy 2e-33); at dt = 0.01 the first record holds 2.6e-4."""
    T, nodes, el, fixed, e0 = gc.guyed_mast(load)
    u, n, rest = mast_run(T)
    slack = T.slack(u)
    keep = [i for i in range(3) if not slack[i]]
    reduced = gc.guyed_mast(load, elements=keep)
    u_red, _, ok_red = gl.newton(nodes, reduced[2], T.loads, fixed, EA, 2, e0=reduced[4])
    u_bar, _, ok_bar = gl.newton(nodes, el, T.loads, fixed, EA, 2, e0=e0)
    miss = np.max(np.abs(u - u_red)) / np.max(np.abs(u_red))
    print(f"load {load}: at rest after {n} steps, slack {slack.tolist()}, u_top {u[2:4]}, miss to the reduced structure "
          f"{miss:.2e} max |u|, to the all-bar solution {np.max(np.abs(u - u_bar)):.2e} at max |u| {np.max(np.abs(u)):.2e}")
    assert rest and ok_red and ok_bar and miss <= 1e-12
    if load == 2.0:
        assert slack.tolist() == [False, False, True]
        assert np.max(np.abs(u - u_bar)) > 1e-2
    else:
        assert not slack.any()


# ---------------------------------------------------------------------------------------------------------------------
# the bound
# ---------------------------------------------------------------------------------------------------------------------
def multi_step_cables():
    """The 257-element truss of the device tests with the seeded half flagged, under their multi-step load (20 x standard
    normal from rest at half the bound of the undeformed truss, rho A = 1)."""
    nodes, el, fixed = irregular_truss_with_supports(257, np.random.default_rng(1257))
    loads = 20.0 * np.random.default_rng(100).standard_normal(nodes.size)
    T = gc.CableTruss(nodes, el, fixed, 2, EA, None, gd.lumped_mass(nodes, el, 1.0, 2), loads, gc.seeded_half(257))
    return T, 0.5 * T.stable_time_step(np.zeros(T.n))


def test_cable_bound_lies_between_the_active_set_and_the_all_bar_bound():
    """After 256 steps of the multi-step load many flagged elements are slack and many have changed state on the way.  There
    the highest frequency of the tangent with the slack blocks zeroed (scipy.linalg.eigvalsh) <= the cable bound <= the
    all-bar bound at u = 0 (68.05 <= 89.33 <= 89.90 with 89 elements slack and 121 that changed state on the way); and
    dynamics.omega_bound(..., cable=...), fed the restatement's strains, is the restatement's.  The first inequality is the
    bound's claim.  The second is a fact of this case, not a theorem: strains reach 0.2 here, and a stretched element's
    block is larger than at rest, so other draws of the flags end a few percent above the bound at rest; solve_dynamic
    therefore re-evaluates the bound at every record point."""
    T, dt = multi_step_cables()
    zero = np.zeros(T.n)
    u, v, at, ever = T.state_changes(zero, zero, 0, 256, dt)
    n_slack = int(T.slack(u).sum())
    active, bound, bar0 = T.omega_active(u), T.omega_bound(u), T.omega_bound(zero)
    print(f"{int(T.cable.sum())} flagged, {n_slack} slack after 256 steps, {int(ever.sum())} elements changed state at {len(at)} "
          f"steps; active set {active:.2f} <= cable bound {bound:.2f} <= all-bar bound at rest {bar0:.2f}")
    assert T.cable.sum() == 121 and n_slack == 89 and ever.sum() == 121
    assert active <= bound <= bar0
    assert bar0 == gd.Truss.omega_bound(T, zero)            # at rest nothing is clipped
    model = _model(T, density=2.0)              # rho A = 1
    mass = dyn.lumped_mass(model)
    assert np.allclose(np.repeat(mass, 2), T.mass, rtol=1e-15, atol=0.0)
    assert dyn.omega_bound(model, T.strain(u)[0], None, mass, cable=T.cable) == pytest.approx(bound, rel=1e-13)
    assert dyn.omega_bound(model, T.strain(u)[0], None, mass) == pytest.approx(gd.Truss.omega_bound(T, u), rel=1e-13)
    # with an initial strain: a slack element counts with E A (1 + 2 e0) / l0
    M = gc.guyed_mast(2.0)[0]
    um = np.zeros(8)
    um[2] = 0.05
    assert M.slack(um).tolist() == [False, False, True]
    want = EA * (1.0 + 2.0 * -1e-3) / 5.0
    assert M.beta(um)[2] == pytest.approx(want, rel=1e-15) and gd.Truss.beta(M, um)[2] < want
    mm = _model(M)
    assert dyn.omega_bound(mm, M.strain(um)[0], M.e0, dyn.lumped_mass(mm), cable=M.cable) == pytest.approx(M.omega_bound(um), rel=1e-13)


# ---------------------------------------------------------------------------------------------------------------------
# check_dynamics, JSON, ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_check_dynamics_refuses_bad_cable_elements():
    T = gc.guyed_mast(2.0)[0]
    model = _model(T)
    for good in (None, [], "all", [1, 2], [2], np.array([0, 1])):
        dyn.check_dynamics(model, _config(), dyn.DynamicsConfig(n_steps=10, cable_elements=good))
    for bad in ("every", "ALL", "", [0.5], [1.0, 2.0], ["1"], [[1, 2]], 1, [3], [-1], [0, 3], [1, 1], [2, 1, 2], [True]):
        with pytest.raises(ValueError, match="cable_elements"):
            dyn.check_dynamics(model, _config(), dyn.DynamicsConfig(n_steps=10, cable_elements=bad))
    # before an engine is built: without a GPU a refused call is a ValueError, never the engine's error
    with pytest.raises(ValueError, match="cable_elements"):
        dyn.solve_dynamic(model, _config(), dyn.DynamicsConfig(n_steps=10, cable_elements=[7]))
    with pytest.raises(ValueError, match="cable_elements"):
        dyn.stable_time_step(model, _config(), cable_elements="some")


def test_no_cables_is_one_configuration_downstream():
    """None and an empty list are the same thing to everything behind check_dynamics: no mask, so the engine is begun with
    cable=None and goes through the bar entry points."""
    T = gc.guyed_mast(2.0)[0]
    model = _model(T)
    assert dyn.DynamicsConfig().cable_elements is None
    assert dyn.cable_mask(model, None) is None and dyn.cable_mask(model, []) is None and dyn.cable_mask(model, ()) is None
    assert dyn.cable_mask(model, "all").tolist() == [True, True, True]
    assert dyn.cable_mask(model, [2, 1]).tolist() == [False, True, True]
    strain, mass = T.strain(np.zeros(8))[0], dyn.lumped_mass(model)
    assert dyn.omega_bound(model, strain, T.e0, mass, cable=dyn.cable_mask(model, [])) == dyn.omega_bound(model, strain, T.e0, mass)


def test_json_inputs_parse_to_cable_elements(tmp_path):
    from pinn_fem_amd.cli import generic as g
    p = g.parse_problem(os.path.join(HERE, "nl_inputs", "guyed_mast_slack.json"))
    d = p["dynamics"]["config"]
    assert d.cable_elements == [1, 2] and d.damping == 17.7 and d.rest_tolerance == 1e-26 and d.record_every == 100
    assert d.n_steps == 20000 and p["solver_config"].initial_strain == [0.0, -0.001, -0.001]
    T = gc.guyed_mast(2.0)[0]
    assert np.array_equal(np.asarray(p["model"].nodes), T.X) and np.array_equal(np.asarray(p["model"].elements), T.el)
    assert np.array_equal(np.asarray(p["model"].loads).reshape(-1), T.loads)
    assert np.array_equal(np.repeat(dyn.check_dynamics(p["model"], p["solver_config"], d), 2), T.mass)
    assert dyn.cable_mask(p["model"], d.cable_elements).tolist() == T.cable.tolist()
    assert d.dt < 0.9 * T.stable_time_step(np.zeros(8))
    p = g.parse_problem(os.path.join(HERE, "nl_inputs", "cable_free_flight.json"))
    d = p["dynamics"]["config"]
    assert d.cable_elements == "all" and d.dt == DT and d.n_steps == 256 and p["model"].dimension == 1
    F = gc.one_cable(-1.0)
    assert np.array_equal(np.repeat(dyn.check_dynamics(p["model"], p["solver_config"], d), 1), F.mass)
    assert np.array_equal(np.asarray(p["model"].loads).reshape(-1), F.loads)
    # a file without the key: the field keeps its default
    assert g.parse_problem(os.path.join(HERE, "nl_inputs", "two_bar_snap_dynamic.json"))["dynamics"]["config"].cable_elements is None
    # a bad value passes the parser's shape check and is check_dynamics' to refuse
    doc = json.load(open(os.path.join(HERE, "nl_inputs", "guyed_mast_slack.json")))
    doc["accel"]["dynamics"]["cable_elements"] = "most"
    (tmp_path / "bad.json").write_text(json.dumps(doc))
    p = g.parse_problem(str(tmp_path / "bad.json"))
    with pytest.raises(ValueError, match="cable_elements"):
        dyn.check_dynamics(p["model"], p["solver_config"], p["dynamics"]["config"])


def test_abi_surface():
    from pinn_fem_amd import _capi
    lib = _capi.load()
    header = open(os.path.join(ROOT, "include", "pinnfem_hip.h")).read()
    for name in ("pf_gl_dyn_start_cable", "pf_gl_dyn_steps_cable", "pf_gl_dyn_graph_create_cable", "pf_gl_dyn_energy_cable"):
        assert re.search(r"^int " + name + r"\(const pf_problem\* p, const pf_gl\* g, const pf_dyn\* dyn, const unsigned char\* cable,",
                         header, re.M), name
        assert name in _capi.SYMBOLS and hasattr(lib, name)
    assert lib.pf_abi_version() == 9 == _capi.PF_ABI_VERSION
    assert lib.pf_sizeof(7) == C.sizeof(_capi.PfDyn) == 104
    blocks = int(re.search(r"#define PF_MAX_NODE_BLOCKS (\d+)", header).group(1))
    assert re.search(r"#define PF_DYN_CABLE_ENERGY_COUNT \(5 \+ 5 \* PF_MAX_NODE_BLOCKS\)", header)
    assert _capi.PF_DYN_CABLE_ENERGY_COUNT == 5 + 5 * blocks and _capi.PF_DYN_ENERGY_COUNT == 4 + 4 * blocks


def test_null_cable_and_bad_arguments_are_rejected_on_the_host():
    """A null cable is PF_ERR_ARG with the function's name in front, and so is, with a cable given, what the bar entry points
    refuse (here: the bad mesh of an empty record), before any HIP call: this runs without a GPU."""
    from pinn_fem_amd import _capi
    lib = _capi.load()
    p, g, d = _capi.PfProblem(), _capi.PfGl(), _capi.PfDyn()
    graph = C.c_void_p()
    flags = (C.c_ubyte * 4)()
    head = (C.byref(p), C.byref(g), C.byref(d))
    for cable, text in ((None, "null cable"), (C.cast(flags, C.c_void_p), "bad mesh")):
        calls = {"pf_gl_dyn_start_cable": lambda: lib.pf_gl_dyn_start_cable(*head, cable, None),
                 "pf_gl_dyn_steps_cable": lambda: lib.pf_gl_dyn_steps_cable(*head, cable, 1, None),
                 "pf_gl_dyn_graph_create_cable": lambda: lib.pf_gl_dyn_graph_create_cable(*head, cable, 1, None, C.byref(graph)),
                 "pf_gl_dyn_energy_cable": lambda: lib.pf_gl_dyn_energy_cable(*head, cable, None, None)}
        for name, call in calls.items():
            assert call() == _capi.PF_ERR_ARG
            assert lib.pf_last_error().decode().startswith(name + ": " + text), lib.pf_last_error()
    assert not graph
