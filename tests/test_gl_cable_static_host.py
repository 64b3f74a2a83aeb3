"""Tension-only (cable) elements in the static Green-Lagrange Newton solve, without a GPU: the restatement
tests/gl_cable_static_reference.py (gl_reference.newton with the slack rule as an active-set iteration) pinned to
gl_reference.newton of the structures without their slack elements and to closed forms, and the surface of the package:
the refusals, SolverConfig.cable_elements, the JSON forms, solve_dynamic's inheritance rule and the C ABI.  The measured
figures are printed in front of every assertion.

The bound 1e-12 of max |u| between two Newton solutions of one structure is test_gl_cable_host.py's: both stop at
|du| / |u| <= 1e-10 with quadratic convergence, so what is left of either is of the order 1e-20 and round-off decides.
"""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import gl_cable_reference as gc
import gl_cable_static_reference as gs
import gl_reference as gl
from helpers import ROOT
from pinn_fem_amd.fem import dynamics as dyn
from pinn_fem_amd.fem import identify, prestress, solver
from pinn_fem_amd.fem.model import FEMModel, Material

HERE = os.path.dirname(os.path.abspath(__file__))
EA, YOUNG, AREA = 1000.0, 2000.0, 0.5
SAME_SOLUTION = 1e-12           # of max |u| (see above)
# the Newton stop leaves u uncertain by 1e-10 |u|, |u| <= 3.2 here, so a strain by about 3e-10: a slack decision is well
# defined where every flagged element is 1e-6 away from e - e0 = 0
SET_MARGIN = 1e-6


def _model(nodes, el, loads, fixed, dim=2):
    return FEMModel(nodes=nodes, elements=el, material=Material(YOUNG, AREA, 1.0), loads=loads, fixed_dofs=fixed, dimension=dim)


def _mast_model():
    T, nodes, el, fixed, e0 = gc.guyed_mast(2.0)
    return _model(nodes, el, T.loads, fixed), e0


def _cfg(**kw):
    return solver.SolverConfig(**{**dict(method="nr", kinematics="green-lagrange", max_iterations=50, tolerance=1e-10), **kw})


# ---------------------------------------------------------------------------------------------------------------------
# 1. the restatement
# ---------------------------------------------------------------------------------------------------------------------
def test_guyed_mast_ends_on_the_structure_without_its_slack_guy():
    """Load 2, e0 = -1e-3 on the guys, from u = 0: the leeward guy goes slack once, and the active-set Newton ends on
    gl.newton of the mast with elements (0, 1) alone, 2e-2 away from the all-bar solution (test_gl_cable_host.py's 1e-2)."""
    T, nodes, el, fixed, e0 = gc.guyed_mast(2.0)
    u, it, ok, slack, changes = gs.newton_cable(nodes, el, T.loads, fixed, EA, 2, T.cable, e0=e0)
    reduced = gc.guyed_mast(2.0, elements=[0, 1])
    u_red, _, ok_red = gl.newton(nodes, reduced[2], T.loads, fixed, EA, 2, e0=reduced[4])
    u_bar, _, ok_bar = gl.newton(nodes, el, T.loads, fixed, EA, 2, e0=e0)
    miss = np.max(np.abs(u - u_red)) / np.max(np.abs(u_red))
    away = np.max(np.abs(u - u_bar))
    print(f"guyed mast: {it} iterations, the set changed {changes} time(s), slack {slack.tolist()}, miss to the reduced "
          f"structure {miss:.2e} max |u|, all-bar solution {away:.2e} away")
    assert ok and ok_red and ok_bar and slack.tolist() == [False, False, True] and changes == 1
    assert miss <= SAME_SOLUTION and away > 1e-2


# the restatement's own iteration counts: (one increment, each of four increments)
GIRDER_ITERATIONS = {8: (6, [5, 5, 5, 4]), 64: (6, [5, 5, 5, 5])}


@pytest.mark.parametrize("n_panels", [8, 64])
def test_xbraced_girder_ends_on_the_girder_without_its_slack_diagonals(n_panels):
    """Classic counter-bracing: under the tip load (5 % of the span) one diagonal of every panel goes slack.  In one
    increment and in four, the result is gl.newton of the girder without those diagonals, started from it."""
    nodes, el, unit, fixed, tip, cable = gs.xbraced_girder(n_panels)
    loads = gs.GIRDER_LOADS[n_panels] * unit
    u, it, ok, slack, changes = gs.newton_cable(nodes, el, loads, fixed, EA, 2, cable)
    margin = gs.slack_set(nodes, el, u, 2, cable)[1]
    u4, slack4, its4 = gs.incremental_cable(nodes, el, loads, fixed, EA, 2, cable, 4)
    scale = np.max(np.abs(u))
    for label, got, s in (("one increment", u, slack), ("four increments", u4, slack4)):
        u_red, it_red, ok_red = gl.newton(nodes, el[~s], loads, fixed, EA, 2, u0=got)
        miss = np.max(np.abs(got - u_red)) / scale
        print(f"{n_panels} panels, {label}: tip {got[tip]:.6f} ({-got[tip] / n_panels:.4f} of the span), {int(s.sum())} slack, "
              f"miss to the reduced girder {miss:.2e} max |u| (its Newton: {it_red} iteration(s))")
        assert ok_red and miss <= SAME_SOLUTION
        assert s.reshape(n_panels, 5)[:, :3].sum() == 0 and s.reshape(n_panels, 5)[:, 3:].sum(axis=1).tolist() == [1] * n_panels
    print(f"{n_panels} panels: {it} iterations ({changes} with a changed set), four increments {its4}, smallest |e - e0| "
          f"over the flagged elements {margin:.2e}")
    assert ok and abs(-u[tip] / n_panels - 0.05) <= 1e-3
    assert margin >= SET_MARGIN
    assert (it, its4) == GIRDER_ITERATIONS[n_panels]
    assert np.array_equal(slack, slack4) and np.max(np.abs(u - u4)) / scale <= SAME_SOLUTION


@pytest.mark.parametrize("load", [50.0, -50.0])
def test_bilinear_1d(load):
    """Nodes 0, 1, 2, both ends fixed, element 0-1 a bar and 1-2 a cable.  A load on node 1 towards node 2 slackens the cable:
    the single bar's closed form.  A load away from node 2: the two-element answer, the cable taut."""
    x, el, fixed, cable = gs.bilinear_1d()
    loads = np.array([0.0, load, 0.0])
    u, it, ok, slack, _ = gs.newton_cable(x, el, loads, fixed, EA, 1, cable)
    assert ok and u[0] == 0.0 and u[2] == 0.0
    if load > 0.0:
        got = gl.bar_1d_load(EA, 1.0, u[1])
        print(f"towards the cable: u = {u[1]:.9f} in {it} iterations, bar_1d_load(u) / load - 1 = {got / load - 1.0:.2e}")
        assert slack.tolist() == [False, True] and abs(got / load - 1.0) <= 1e-12
    else:
        u_two, _, ok_two = gl.newton(x, el, loads, fixed, EA, 1)
        print(f"away from the cable: u = {u[1]:.9f} in {it} iterations, two-element answer {u_two[1]:.9f}")
        assert ok_two and not slack.any() and abs(u[1] - u_two[1]) <= SAME_SOLUTION * abs(u_two[1])


def test_one_cable_pushed_towards_its_support_is_a_mechanism():
    """One cable, one free node, the load pushes towards the support: taut at u = 0 (e = 0), so the first iteration solves
    and compresses it; the second finds nothing holding the node."""
    with pytest.raises(gs.Mechanism) as err:
        gs.newton_cable(np.array([0.0, 1.0]), np.array([[0, 1]]), np.array([0.0, -1.0]), np.array([0]), EA, 1, True)
    assert err.value.iteration == 2 and err.value.dof == 1 and err.value.value == 0.0
    # the same load on a bar is an ordinary solve
    assert gl.newton(np.array([0.0, 1.0]), np.array([[0, 1]]), np.array([0.0, -1.0]), np.array([0]), EA, 1)[2]


# ---------------------------------------------------------------------------------------------------------------------
# 2. the surface
# ---------------------------------------------------------------------------------------------------------------------
def test_every_refusal(monkeypatch):
    monkeypatch.setattr(solver, "_engine_for", lambda *a, **k: pytest.fail("an engine was built"))
    model, e0 = _mast_model()

    def refused(match, config, runs=("solve_nr", "solve")):
        for name in runs:
            with pytest.raises(ValueError, match=match):
                solver.solve_nr(model, config, 1.0) if name == "solve_nr" else solver.solve(model, config)

    refused("cable_elements needs kinematics 'green-lagrange'", _cfg(kinematics="linear", cable_elements=[1, 2]))
    refused("cable_elements does not support nr_control 'displacement'",
            _cfg(cable_elements=[1, 2], nr_control="displacement", nr_control_dof=2, nr_control_displacement=0.1))
    refused('must be "all" or a list of element ids', _cfg(cable_elements="most"))
    refused("element ids in 0..2", _cfg(cable_elements=[1, 3]))
    refused("names an element twice", _cfg(cable_elements=[1, 1]))
    refused("belongs to the Green-Lagrange Newton solve", _cfg(cable_elements=[1, 2], method="gd"), runs=("solve",))
    with pytest.raises(ValueError, match="cable_elements needs kinematics"):
        solver.solve_hybrid(model, _cfg(kinematics="linear", cable_elements="all"))
    # the identifications: the sensitivities treat every element as a bar
    config, levels = _cfg(cable_elements=[1, 2], initial_strain=e0), [(1.0, [2], [0.01])]
    for run in (lambda: identify.identify_nr(model, config, levels, groups=[0, 1, 1]),
                lambda: identify.misfit_and_gradient(model, config, levels, np.full(3, EA)),
                lambda: prestress.identify_prestress(model, config, levels, [-1, 0, 0])):
        with pytest.raises(ValueError, match="does not support cable_elements: the sensitivities treat every element as a bar"):
            run()
    # NN materials and sharded runs, where Green-Lagrange is refused already
    monkeypatch.setattr(solver, "_world_size", lambda: 2)
    refused("cable_elements does not support a sharded", _cfg(cable_elements=[1, 2]), runs=("solve_nr",))
    monkeypatch.setattr(solver, "_world_size", lambda: 1)
    monkeypatch.setattr(type(model.material), "has_trainable_params", lambda self: True)
    refused("cable_elements needs scalar materials", _cfg(cable_elements=[1, 2]), runs=("solve_nr",))


def test_no_cables_is_one_configuration_downstream():
    model, _ = _mast_model()
    assert solver.SolverConfig().cable_elements is None
    for nothing in (None, [], ()):
        assert solver.check_cables(_cfg(cable_elements=nothing), model) is None
        # no kinematics is asked of a configuration without cables
        assert solver.check_cables(_cfg(kinematics="linear", cable_elements=nothing), model) is None
    assert solver.check_cables(_cfg(cable_elements="all"), model).tolist() == [True, True, True]
    assert solver.check_cables(_cfg(cable_elements=[2, 1]), model).tolist() == [False, True, True]
    # cable_mask moved to solver.py; dynamics keeps the name
    assert dyn.cable_mask is solver.cable_mask and dyn.cable_mask(model, [2]).tolist() == [False, False, True]
    # the setup without flags carries none, and the result's new field stays None
    fields = solver._NewtonSetup._fields
    assert fields[-1] == "cable" and solver._NewtonSetup._field_defaults["cable"] is None
    assert solver.SolverResult.__dataclass_fields__["slack"].default is None


def test_json_inputs_and_res_json_keys(monkeypatch):
    from pinn_fem_amd.cli import generic
    p = generic.parse_problem(os.path.join(HERE, "nl_inputs", "guyed_mast_static.json"))
    T, nodes, el, fixed, e0 = gc.guyed_mast(2.0)
    assert p["solver_config"].cable_elements == [1, 2] and p["solver_config"].initial_strain == e0.tolist()
    assert p["solver_config"].kinematics == "green-lagrange" and p.get("dynamics") is None
    assert np.array_equal(np.asarray(p["model"].nodes), nodes) and np.array_equal(np.asarray(p["model"].elements), el)
    assert solver.check_cables(p["solver_config"], p["model"]).tolist() == T.cable.tolist()
    p = generic.parse_problem(os.path.join(HERE, "nl_inputs", "xbraced_girder_static.json"))
    nodes, el, unit, fixed, tip, cable = gs.xbraced_girder(8)
    assert np.array_equal(np.asarray(p["model"].nodes), nodes) and np.array_equal(np.asarray(p["model"].elements), el)
    assert np.array_equal(np.asarray(p["model"].loads).reshape(-1), gs.GIRDER_LOADS[8] * unit)
    assert solver.check_cables(p["solver_config"], p["model"]).tolist() == cable.tolist() and p["solver_config"].n_increments == 4
    # "all", a file without the key, a value of the wrong shape
    data = {"accel": {"kinematics": "green-lagrange", "cable_elements": "all"}}
    assert generic._solver_config_from(data).cable_elements == "all"
    assert generic._solver_config_from({"accel": {}}).cable_elements is None
    for bad in ("most", [1.5], [True], {"ids": [1]}, 3):
        with pytest.raises(ValueError, match="accel.cable_elements"):
            generic._solver_config_from({"accel": {"kinematics": "green-lagrange", "cable_elements": bad}})

    def fake(slack, axial):
        return lambda **kw: solver.SolverResult(displacements=np.zeros((4, 2)), reactions=np.zeros((4, 2)), converged=True,
                                                history=[{"iterations": 1.0}], axial_forces=axial, slack=slack)
    parsed = {"model": _mast_model()[0], "solver_config": solver.SolverConfig(), "measured_data": {}, "accel": {}}
    old_keys = ["success", "converged", "iterations", "history", "displacements", "reactions"]
    monkeypatch.setattr(generic, "solve", fake(None, None))
    assert list(generic.solve_problem(parsed)) == old_keys
    monkeypatch.setattr(generic, "solve", fake(np.array([False, False, True]), np.array([3.0, 2.0, 0.0])))
    out = generic.solve_problem(parsed)
    assert sorted(out) == sorted(old_keys + ["axial_forces", "slack_elements"])
    assert out["slack_elements"] == [2] and out["axial_forces"] == [3.0, 2.0, 0.0]
    json.dumps(out)


def test_solve_dynamic_takes_the_cables_of_the_solver_config():
    model, e0 = _mast_model()
    both = lambda c, d: dyn.dynamic_cables(model, _cfg(cable_elements=c), dyn.DynamicsConfig(n_steps=1, cable_elements=d))
    assert both(None, None) is None and both([], None) is None and both(None, []) is None
    assert both([1, 2], None).tolist() == [False, True, True]               # inherited
    assert both(None, [1, 2]).tolist() == [False, True, True]               # its own, as before
    assert both([2, 1], [1, 2]).tolist() == [False, True, True]             # the same set twice
    assert both("all", [0, 1, 2]).tolist() == [True, True, True]
    for c, d in (([1, 2], [1]), ([1], "all"), ([1, 2], [])):
        with pytest.raises(ValueError, match="name different elements"):
            both(c, d)
    # check_dynamics runs the rule before an engine is built
    with pytest.raises(ValueError, match="name different elements"):
        dyn.check_dynamics(model, _cfg(cable_elements=[1, 2]), dyn.DynamicsConfig(n_steps=1, cable_elements=[1]))
    with pytest.raises(ValueError, match="cable_elements"):
        dyn.check_dynamics(model, _cfg(cable_elements="most"), dyn.DynamicsConfig(n_steps=1))


def test_abi_declares_the_cable_state():
    from pinn_fem_amd import _capi
    lib = _capi.load()
    header = open(os.path.join(ROOT, "include", "pinnfem_hip.h")).read()
    P, G, V = _capi._PP, _capi._PG, C.c_void_p
    decl = re.search(r"\bint pf_gl_state_cable\(([^;]*)\);", header)
    assert decl
    assert [" ".join(a.split()) for a in decl.group(1).split(",")] == [
        "const pf_problem* p", "const pf_gl* g", "const double* ea", "const double* e0", "const unsigned char* cable",
        "unsigned char* slack", "double* counts", "const double* u", "void* stream"]
    assert _capi.SYMBOLS["pf_gl_state_cable"] == (C.c_int, [P, G, V, V, V, V, V, V, V]) and hasattr(lib, "pf_gl_state_cable")
    assert lib.pf_abi_version() == 9 == _capi.PF_ABI_VERSION and re.search(r"#define PF_ABI_VERSION 9\b", header)
    blocks = int(re.search(r"#define PF_MAX_NODE_BLOCKS (\d+)", header).group(1))
    assert re.search(r"#define PF_GL_CABLE_COUNT \(2 \+ 2 \* PF_MAX_NODE_BLOCKS\)", header)
    assert _capi.PF_GL_CABLE_COUNT == 2 + 2 * blocks
    # the bar entry points and the record keep their shapes
    assert _capi.SYMBOLS["pf_gl_state"] == (C.c_int, [P, G, V, V]) and _capi.SYMBOLS["pf_gl_state_e0"] == (C.c_int, [P, G, V, V, V, V])
    assert [f[0] for f in _capi.PfGl._fields_] == ["d0", "kt", "fe", "strain"]


def test_null_operands_are_rejected_on_the_host():
    """A null cable, slack or counts is PF_ERR_ARG naming the bar entry points, before the mesh is looked at and before any
    HIP call: this runs without a GPU."""
    from pinn_fem_amd import _capi
    lib = _capi.load()
    p, g = _capi.PfProblem(), _capi.PfGl()
    flags, counts = (C.c_ubyte * 4)(), (C.c_double * 4)()
    f, c = C.cast(flags, C.c_void_p), C.cast(counts, C.c_void_p)
    for cable, slack, cnt in ((None, f, c), (f, None, c), (f, f, None)):
        assert lib.pf_gl_state_cable(C.byref(p), C.byref(g), None, None, cable, slack, cnt, None, None) == _capi.PF_ERR_ARG
        text = lib.pf_last_error().decode()
        assert text.startswith("pf_gl_state_cable: null cable, slack or counts") and "pf_gl_state_e0" in text, text
    assert lib.pf_gl_state_cable(C.byref(p), C.byref(g), None, None, f, f, c, None, None) == _capi.PF_ERR_ARG
    assert lib.pf_last_error().decode().startswith("pf_gl_state_cable: bad argument")
