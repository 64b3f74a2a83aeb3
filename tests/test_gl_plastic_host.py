"""Elastoplastic bars in the Green-Lagrange Newton solve, without a GPU: the restatement tests/gl_plastic_reference.py pinned
to finite differences, to gl_reference's elastic element, to the 1-D closed forms and to the small-strain closed forms of the
three-bar truss, the load programs the device tests repeat, and the surface of the package: the refusals, the configuration,
the JSON forms and the C ABI.  The measured figures are printed in front of every assertion.
"""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import gl_plastic_reference as gp
import gl_reference as gl
from gl_plastic_driver import FIELD_SEEDS, KAPPAS, field_case
from helpers import ROOT
from pinn_fem_amd.fem import dynamics as dyn
from pinn_fem_amd.fem import identify, prestress, solver
from pinn_fem_amd.fem.model import FEMModel, Material

HERE = os.path.dirname(os.path.abspath(__file__))
EA, YOUNG, AREA = 1000.0, 2000.0, 0.5
EY = gp.EY


def _model(nodes, el, loads, fixed, dim=2):
    return FEMModel(nodes=nodes, elements=el, material=Material(YOUNG, AREA, 1.0), loads=loads, fixed_dofs=fixed, dimension=dim)


def _cfg(**kw):
    return solver.SolverConfig(**{**dict(method="nr", kinematics="green-lagrange", max_iterations=50, tolerance=1e-10), **kw})


# ---------------------------------------------------------------------------------------------------------------------
# 1. the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FIELD_SEEDS))
@pytest.mark.parametrize("kappa_name", KAPPAS)
@pytest.mark.parametrize("with_e0_ea", [False, True])
def test_margin_condition_of_the_device_seeds(name, kappa_name, with_e0_ea):
    """|f - 2^-40 r| >= 1e-6 ey on every element of both fields: device and host take the same branch everywhere, and no
    element is left out of any comparison.  Some elements yield (3 % at least), and not all do."""
    nodes, el, fixed, dim, u, other, kappa, ep_n, al_n, e0, ea = field_case(name, kappa_name, with_e0_ea)
    for label, field in (("u", u), ("other", other)):
        margin = gp.yield_margin(nodes, el, field, dim, EY, kappa, ep_n, al_n, e0)
        plastic = gp.element_state_plastic(nodes, el, field, EA, dim, EY, kappa, ep_n, al_n, e0)[5]
        print(f"{name}, kappa {kappa_name}, e0/ea {with_e0_ea}, {label}: margin {margin:.2e} ey, {plastic.mean():.2f} plastic")
        assert margin >= gp.MARGIN and 0.03 < plastic.mean() < 0.97


def test_margin_condition_of_the_grid_stride_field():
    from gl_plastic_driver import wrap_case
    x, el, fixed, u = wrap_case()
    margin = gp.yield_margin(x, el, u, 1, EY, 0.05)
    plastic = gp.element_state_plastic(x, el, u, EA, 1, EY, 0.05)[5]
    print(f"{len(el)} elements: margin {margin:.2e} ey, {plastic.mean():.2f} plastic, {int(plastic[-37:].sum())} of the last 37")
    assert margin >= gp.MARGIN and plastic[-37:].any() and not plastic[-37:].all()


def _fd_case(seed):
    from device_driver import irregular_truss_with_supports
    rng = np.random.default_rng(seed)
    nodes, el, fixed = irregular_truss_with_supports(63, rng)
    u = gp.seeded_field(nodes, el, 2, rng, amplitude=1.5e-2)
    kappa = rng.uniform(0.0, 0.5, len(el))
    ep_n, al_n = gp.seeded_state(len(el), rng)
    e0 = rng.uniform(-3e-4, 3e-4, len(el))
    return nodes, el, u, kappa, ep_n, al_n, e0


def test_consistent_tangent_against_central_differences():
    """K_t v against (f_int(u + h v) - f_int(u - h v)) / 2h with h |v| = 1e-9 of a length, on a seeded field whose every
    element keeps a margin of 1e-3 ey, so no element changes its branch inside the stencil (h moves a strain by < 1e-8 ey).
    The central difference is second order: its truncation is nothing here; its round-off is a few 2^-53 of the element
    forces (up to 5 here) over h |v| = 1e-9, about 1e-6, against |K v| of the order E A |v| / l0 ~ 1e3: 1e-9 of max |K v|.
    The bound is 1e-7 of max |K v|.  The tangent that keeps E A where an element is plastic (the mutant) is off by
    1 / (1 + kappa) of a plastic element's stiffness, of the order of |K v| itself, and must be rejected."""
    nodes, el, u, kappa, ep_n, al_n, e0 = _fd_case(91)
    args = (EA, 2, EY, kappa, ep_n, al_n, e0)
    margin = gp.yield_margin(nodes, el, u, 2, EY, kappa, ep_n, al_n, e0)
    plastic = gp.element_state_plastic(nodes, el, u, *args)[5]
    assert margin >= 1e-3 and 0.2 < plastic.mean() < 0.9
    rng = np.random.default_rng(92)
    worst, worst_mutant = 0.0, np.inf
    for _ in range(4):
        v = rng.standard_normal(u.size)
        h = 1e-9 / np.max(np.abs(v))
        fd = (gp.f_int_plastic(nodes, el, u + h * v, *args) - gp.f_int_plastic(nodes, el, u - h * v, *args)) / (2.0 * h)
        kv = gp.k_t_plastic(nodes, el, u, *args) @ v
        kv_mutant = gp.k_t_plastic(nodes, el, u, *args, tangent="elastic") @ v
        worst = max(worst, np.max(np.abs(kv - fd)) / np.max(np.abs(kv)))
        worst_mutant = min(worst_mutant, np.max(np.abs(kv_mutant - fd)) / np.max(np.abs(kv)))
    print(f"consistent tangent: {plastic.mean():.2f} plastic, margin {margin:.1e} ey, K v against central differences "
          f"{worst:.2e} of max |K v|; the elastic-modulus mutant {worst_mutant:.2e}")
    assert worst <= 1e-7
    assert worst_mutant > 1e-2


def test_elastic_limit_is_the_bar_to_the_byte():
    nodes, el, u, kappa, _, _, e0 = _fd_case(93)
    u = 20.0 * u                                                     # |du| / l0 up to 0.3
    for zz in (None, e0):
        bar = gl.element_state(nodes, el, u, EA, 2, zz)
        got = gp.element_state_plastic(nodes, el, u, EA, 2, np.inf, kappa, 0.0, 0.0, zz)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got[:3], bar[:3]))
        assert not got[5].any() and not got[3].any() and not got[4].any()


@pytest.mark.parametrize("kappa", [0.0, 0.1, 0.5])
def test_bar_1d_closed_forms(kappa):
    """A virgin bar stretched to e_max = 3 ey: N = E A (ey + kappa e) / (1 + kappa) on the way; after unloading to N = 0 the
    strain is (e_max - ey) / (1 + kappa) (elastic unloading of slope E A from the expanded surface); pushed on, it yields
    in compression when tr reaches the expanded radius ey + kappa alpha, not ey."""
    l0 = 2.0
    x, el, fixed = gp.bar_1d(l0)
    e_of = lambda end: (2.0 * l0 * end + end * end) / (2.0 * l0 * l0)
    end_of = lambda e: l0 * (np.sqrt(1.0 + 2.0 * e) - 1.0)
    for e in (1.5 * EY, 2.0 * EY, 3.0 * EY):
        st = gp.element_state_plastic(x, el, [0.0, end_of(e)], EA, 1, EY, kappa)
        assert st[5][0] and abs(st[6]["n"][0] / gp.bar_1d_force(EA, EY, kappa, e_of(end_of(e))) - 1.0) <= 1e-12
    e_max = e_of(end_of(3.0 * EY))
    st = gp.element_state_plastic(x, el, [0.0, end_of(3.0 * EY)], EA, 1, EY, kappa)
    ep, al = st[3], st[4]
    assert abs(ep[0] / ((e_max - EY) / (1.0 + kappa)) - 1.0) <= 1e-12 and al[0] == ep[0]
    # unloaded: N = 0 at e = ep, through newton_plastic at zero load from the stretched state
    u, it, ok, ep2, al2, plastic = gp.newton_plastic(x, el, np.array([0.0, 1.0]), fixed, EA, 1, EY, kappa, ep, al, lam=0.0,
                                                     u0=[0.0, end_of(3.0 * EY)])
    e_res = e_of(u[1])
    print(f"kappa {kappa}: residual strain {e_res:.6e}, closed form {(e_max - EY) / (1.0 + kappa):.6e}, {it} iterations")
    assert ok and not plastic.any() and abs(e_res / ((e_max - EY) / (1.0 + kappa)) - 1.0) <= 1e-9
    assert ep2.tobytes() == ep.tobytes() and al2.tobytes() == al.tobytes()
    # reverse loading: elastic down to tr = -(ey + kappa alpha), plastic beyond
    radius = EY + kappa * al[0]
    for factor, want in ((0.999, False), (1.001, True)):
        st = gp.element_state_plastic(x, el, [0.0, end_of(ep[0] - factor * radius)], EA, 1, EY, kappa, ep, al)
        assert bool(st[5][0]) == want
    if kappa > 0.0:                                              # the virgin radius would have yielded well before
        assert radius > 1.05 * EY


def test_three_bar_truss_against_the_small_strain_closed_forms():
    T = gp.ThreeBar()
    n_of = lambda o, ep: gp.element_state_plastic(T.nodes, T.el, o["u"], T.ea, 2, EY, 0.0, ep, 0.0)[6]["n"]
    out = gp.load_program(T.nodes, T.el, T.loads, T.fixed, T.ea, 2, EY, 0.0, gp.THREE_BAR_PROGRAM)
    assert len(out) == len(gp.THREE_BAR_PROGRAM) and all(o["converged"] for o in out)
    its = [o["iterations"] for o in out]
    yielding = [o["yielding"].tolist() for o in out]
    print(f"three-bar program: iterations {its}, centre bar yielding {[y[1] for y in yielding]}")
    assert max(its) <= 5
    # first yield at 1 / sqrt 2 = 0.7071: nothing yields up to 0.7, the centre bar alone from 0.8 on
    assert [y[1] for y in yielding] == [False] * 4 + [True] * 3 + [False, False, True, False, True]
    assert not any(y[0] or y[2] for y in yielding)
    # the first-yield load factor itself, by bisection on the restatement from the virgin state, against 1 / sqrt 2
    lo, hi = 0.7, 0.8
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        yields = gp.newton_plastic(T.nodes, T.el, T.loads, T.fixed, T.ea, 2, EY, 0.0, lam=mid)[5].any()
        lo, hi = (lo, mid) if yields else (mid, hi)
    print(f"  first yield at load factor {hi:.6f}, small-strain {T.first_yield:.6f}, miss {abs(hi / T.first_yield - 1.0):.2e}")
    assert abs(hi / T.first_yield - 1.0) <= 2e-3
    # N_centre = P / (1 + 1 / sqrt 2) before first yield, to 2e-3 relative (the kinematics differ by O(ey))
    for o in out[:4]:
        n = n_of(o, 0.0)
        miss = abs(n[1] / T.centre_force_elastic(o["load_factor"]) - 1.0)
        print(f"  load factor {o['load_factor']}: N_centre {n[1]:.6f}, small-strain {T.centre_force_elastic(o['load_factor']):.6f}, miss {miss:.2e}")
        assert miss <= 2e-3
    # yielding: the centre bar carries N_y
    for o in out[4:7]:
        assert abs(n_of(o, o["ep"])[1] / T.n_y - 1.0) <= 1e-12
    # unloaded from 0.97: the centre residual N_y - P_max / (1 + 1 / sqrt 2), to 5e-3 of N_y, self-equilibrated to round-off
    o = out[8]
    assert o["load_factor"] == 0.0
    n = n_of(o, o["ep"])
    miss = abs(n[1] - T.centre_residual(0.97)) / T.n_y
    f_res = gp.f_int_plastic(T.nodes, T.el, o["u"], T.ea, 2, EY, 0.0, o["ep"], o["al"])
    print(f"  unloaded from 0.97: residual forces {n}, closed form centre {T.centre_residual(0.97):.6f}, miss {miss:.2e} of N_y, "
          f"|f_int| at the free node {np.max(np.abs(f_res[6:])):.2e}")
    assert miss <= 5e-3 and n[1] < 0.0 < n[0] and abs(n[0] - n[2]) <= 1e-12
    # (the Newton stop leaves f_int at about K |du| ~ 1e3 * 1e-10 |u|; 1e-12 of N_y is well above its square)
    assert np.max(np.abs(f_res[6:])) <= 1e-12 * T.n_y
    # back at 0.97 after the reversed cycle: perfect plasticity, so the same displacement
    assert abs(out[11]["u"][7] / out[6]["u"][7] - 1.0) <= 1e-12


def test_warren_cantilever_cycle_and_the_reason_for_the_threshold():
    nodes, el, loads, fixed, tip = gp.warren_first_yield()
    out = gp.load_program(nodes, el, loads, fixed, EA, 2, EY, gp.WARREN_KAPPA, gp.WARREN_PROGRAM)
    counts, its = [int(o["yielding"].sum()) for o in out], [o["iterations"] for o in out]
    print(f"8-panel cantilever, kappa {gp.WARREN_KAPPA}, first-yield tip load {-loads[tip]:.6f}: yielding {counts}, "
          f"iterations {its}, tip {[round(float(o['u'][tip]), 5) for o in out]}")
    assert all(o["converged"] for o in out) and counts == [0, 1, 3, 5, 6, 0, 0] and max(its) <= 6
    elastic = gl.newton(nodes, el, 0.0 * loads, fixed, EA, 2)[0]
    assert not elastic.any() and out[-1]["u"][tip] < -0.1            # a permanent tip deflection, downward
    # every converged state keeps the margin against the state it started from: the device's flags are the host's
    ep, al = np.zeros(len(el)), np.zeros(len(el))
    for o in out:
        margin = gp.yield_margin(nodes, el, o["u"], 2, EY, gp.WARREN_KAPPA, ep, al)
        assert margin >= 100.0 * gp.MARGIN, (o["load_factor"], margin)
        ep, al = o["ep"], o["al"]
    # f > 0 as the yield test: the elements that ended 1.6 on the surface take the plastic tangent on the way down
    bare = gp.load_program(nodes, el, loads, fixed, EA, 2, EY, gp.WARREN_KAPPA, gp.WARREN_PROGRAM, threshold=0.0)
    print(f"  with f > 0: {[(o['load_factor'], o['iterations'], o['converged']) for o in bare]}")
    assert [o["converged"] for o in bare] == [True] * 5 + [False] and bare[-1]["load_factor"] == 0.8


def test_compression_mechanism_of_a_perfectly_plastic_bar():
    """A 1-D bar with kappa = 0 at -1.2 N_y: the first iteration is elastic and lands beyond yield, the second has
    E A_t = 0 and B = N / l0 = -N_y / l0."""
    l0 = 2.0
    x, el, fixed = gp.bar_1d(l0)
    with pytest.raises(gp.Mechanism) as err:
        gp.newton_plastic(x, el, np.array([0.0, -1.2 * EA * EY]), fixed, EA, 1, EY, 0.0)
    print(f"mechanism: {err.value}")
    assert err.value.iteration == 2 and err.value.dof == 1 and abs(err.value.value / (-EA * EY / l0) - 1.0) <= 1e-12
    assert gp.newton_plastic(x, el, np.array([0.0, -1.2 * EA * EY]), fixed, EA, 1, EY, 0.1)[2]       # hardening carries it


# ---------------------------------------------------------------------------------------------------------------------
# 2. the surface
# ---------------------------------------------------------------------------------------------------------------------
def _three_bar_model():
    T = gp.ThreeBar()
    return _model(T.nodes, T.el, T.loads, T.fixed)


def test_every_refusal(monkeypatch):
    monkeypatch.setattr(solver, "_engine_for", lambda *a, **k: pytest.fail("an engine was built"))
    model = _three_bar_model()

    def refused(match, config, runs=("solve_nr", "solve"), **kw):
        for name in runs:
            with pytest.raises(ValueError, match=match):
                solver.solve_nr(model, config, 1.0, **kw) if name == "solve_nr" else solver.solve(model, config)

    refused("yield_strain needs kinematics 'green-lagrange'", _cfg(kinematics="linear", yield_strain=EY))
    refused("yield_strain does not support nr_control 'displacement'",
            _cfg(yield_strain=EY, nr_control="displacement", nr_control_dof=7, nr_control_displacement=0.1))
    refused("yield_strain does not support cable_elements", _cfg(yield_strain=EY, cable_elements=[1]))
    refused("yield_strain has 2 entries, the model has 3 elements", _cfg(yield_strain=[EY, EY]))
    refused("hardening_ratio has 4 entries", _cfg(yield_strain=EY, hardening_ratio=[0.0] * 4))
    for bad in (0.0, -EY, float("nan"), [EY, 0.0, EY], "soft"):
        refused("yield_strain must be", _cfg(yield_strain=bad))
    for bad in (-0.1, float("inf"), float("nan"), [0.0, -1.0, 0.0]):
        refused("hardening_ratio must be finite and not negative", _cfg(yield_strain=EY, hardening_ratio=bad))
    for method in ("gd", "full-nr"):
        refused("belongs to the Green-Lagrange Newton solve", _cfg(yield_strain=EY, method=method), runs=("solve",))
    with pytest.raises(ValueError, match="yield_strain needs kinematics"):
        solver.solve_hybrid(model, _cfg(kinematics="linear", yield_strain=EY))
    # the state handed in
    zero = np.zeros(3)
    refused("plastic_state needs config.yield_strain", _cfg(), runs=("solve_nr",), plastic_state=(zero, zero))
    for bad, match in (((zero[:2], zero), "entries"), ((zero, [0.0, np.nan, 0.0]), "non-finite"), ((zero, [0.0, -1e-9, 0.0]), "alpha"),
                       (zero, "pair"), ((zero, zero, zero), "pair")):
        refused("plastic_state.*" + match, _cfg(yield_strain=EY), runs=("solve_nr",), plastic_state=bad)
    # load_factors
    refused("load_factors belongs to solve\\(\\) with method 'nr'", _cfg(load_factors=[0.5, 1.0], method="hybrid"), runs=("solve",))
    refused("load_factors does not support nr_control", _cfg(load_factors=[0.5], nr_control="displacement", nr_control_dof=7,
                                                              nr_control_displacement=0.1), runs=("solve",))
    for bad in ([], [0.5, float("nan")], "up", [[0.5]]):
        refused("load_factors must be", _cfg(load_factors=bad), runs=("solve",))
    # the identifications and the dynamics: elastic inside, so they refuse
    config, levels = _cfg(yield_strain=EY), [(1.0, [7], [-0.001])]
    for run in (lambda: identify.identify_nr(model, config, levels, groups=[0, 1, 0]),
                lambda: identify.misfit_and_gradient(model, config, levels, np.full(3, EA)),
                lambda: prestress.identify_prestress(model, config, levels, [-1, 0, -1])):
        with pytest.raises(ValueError, match="identification does not support yield_strain"):
            run()
    with pytest.raises(ValueError, match="solve_dynamic does not support yield_strain"):
        dyn.solve_dynamic(model, config, dyn.DynamicsConfig(n_steps=1))
    # NN materials and sharded runs
    monkeypatch.setattr(solver, "_world_size", lambda: 2)
    refused("yield_strain does not support a sharded", _cfg(yield_strain=EY), runs=("solve_nr",))
    monkeypatch.setattr(solver, "_world_size", lambda: 1)
    monkeypatch.setattr(type(model.material), "has_trainable_params", lambda self: True)
    refused("yield_strain needs scalar materials", _cfg(yield_strain=EY), runs=("solve_nr",))


def test_the_configuration_without_plasticity_and_its_forms():
    model = _three_bar_model()
    base = solver.SolverConfig()
    assert base.yield_strain is None and base.hardening_ratio == 0.0 and base.load_factors is None
    assert solver.check_plasticity(_cfg(), model) is None and solver.check_load_factors(_cfg()) is None
    # no kinematics is asked of a configuration without plasticity
    assert solver.check_plasticity(_cfg(kinematics="linear", hardening_ratio=0.3), model) is None
    ey, kappa = solver.check_plasticity(_cfg(yield_strain=EY), model)
    assert ey.tolist() == [EY] * 3 and kappa.tolist() == [0.0] * 3 and ey.dtype == kappa.dtype == np.float64
    ey, kappa = solver.check_plasticity(_cfg(yield_strain=[EY, np.inf, 2 * EY], hardening_ratio=[0.0, 0.1, 0.5], initial_strain=1e-4), model)
    assert ey.tolist() == [EY, np.inf, 2 * EY] and kappa.tolist() == [0.0, 0.1, 0.5]
    assert solver.check_plasticity(_cfg(yield_strain=EY, method="hybrid"), model, "hybrid") is not None
    assert solver.check_load_factors(_cfg(load_factors=(0.5, 1, -0.5))) == [0.5, 1.0, -0.5]
    fields = solver._NewtonSetup._fields
    assert "plastic" in fields and solver._NewtonSetup._field_defaults["plastic"] is None
    for name in ("plastic_strain", "accumulated_plastic_strain", "yielding", "load_path"):
        assert solver.SolverResult.__dataclass_fields__[name].default is None


def test_json_inputs_and_res_json_keys(monkeypatch):
    from pinn_fem_amd.cli import generic
    p = generic.parse_problem(os.path.join(HERE, "nl_inputs", "three_bar_plastic.json"))
    T = gp.ThreeBar()
    sc = p["solver_config"]
    assert sc.yield_strain == EY and sc.hardening_ratio == 0.0 and sc.load_factors == gp.THREE_BAR_PROGRAM
    assert sc.kinematics == "green-lagrange" and sc.method == "nr"
    assert np.array_equal(np.asarray(p["model"].nodes), T.nodes) and np.array_equal(np.asarray(p["model"].elements), T.el)
    assert np.array_equal(np.asarray(p["model"].loads).reshape(-1), T.loads)
    assert np.array_equal(np.sort(np.asarray(p["model"].fixed_dofs)), T.fixed)
    p = generic.parse_problem(os.path.join(HERE, "nl_inputs", "warren_plastic_cycle.json"))
    nodes, el, loads, fixed, tip = gp.warren_first_yield()
    sc = p["solver_config"]
    assert sc.yield_strain == EY and sc.hardening_ratio == gp.WARREN_KAPPA and sc.load_factors == gp.WARREN_PROGRAM
    assert np.array_equal(np.asarray(p["model"].nodes), nodes) and np.array_equal(np.asarray(p["model"].elements), el)
    assert np.array_equal(np.asarray(p["model"].loads).reshape(-1), loads)
    assert solver.check_plasticity(sc, p["model"]) is not None
    # lists with null, a file without the key, values of the wrong shape
    data = {"accel": {"kinematics": "green-lagrange", "plasticity": {"yield_strain": [EY, None, 2e-3], "hardening_ratio": [0, 0.1, 0.2]}}}
    sc = generic._solver_config_from(data)
    assert sc.yield_strain == [EY, float("inf"), 2e-3] and sc.hardening_ratio == [0, 0.1, 0.2] and sc.load_factors is None
    sc = generic._solver_config_from({"accel": {}})
    assert sc.yield_strain is None and sc.hardening_ratio == 0.0 and sc.load_factors is None
    for bad in (EY, {"hardening_ratio": 0.1}, {"yield_strain": "soft"}, {"yield_strain": [EY, "x"]}, {"yield_strain": True},
                {"yield_strain": EY, "hardening_ratio": "stiff"}, {"yield_strain": EY, "kinematic": 0.1}):
        with pytest.raises(ValueError, match="accel.plasticity"):
            generic._solver_config_from({"accel": {"kinematics": "green-lagrange", "plasticity": bad}})
    for bad in ([], "up", [0.5, None], 1.0):
        with pytest.raises(ValueError, match="accel.load_factors"):
            generic._solver_config_from({"accel": {"load_factors": bad}})

    def fake(**more):
        return lambda **kw: solver.SolverResult(displacements=np.zeros((4, 2)), reactions=np.zeros((4, 2)), converged=True,
                                                history=[{"iterations": 1.0}], **more)
    parsed = {"model": _three_bar_model(), "solver_config": solver.SolverConfig(), "measured_data": {}, "accel": {}}
    old_keys = ["success", "converged", "iterations", "history", "displacements", "reactions"]
    monkeypatch.setattr(generic, "solve", fake())
    assert list(generic.solve_problem(parsed)) == old_keys
    path = [{"load_factor": 1.0, "iterations": 4.0, "yielding_elements": 1.0}]
    monkeypatch.setattr(generic, "solve", fake(axial_forces=np.array([0.5, 1.0, 0.5]), plastic_strain=np.array([0.0, 1e-4, 0.0]),
                                               accumulated_plastic_strain=np.array([0.0, 2e-4, 0.0]),
                                               yielding=np.array([False, True, False]), load_path=path))
    out = generic.solve_problem(parsed)
    assert sorted(out) == sorted(old_keys + ["axial_forces", "plastic_strain", "accumulated_plastic_strain", "yielding_elements",
                                             "load_path"])
    assert out["yielding_elements"] == [1] and out["plastic_strain"] == [0.0, 1e-4, 0.0] and out["load_path"] == path
    assert out["accumulated_plastic_strain"] == [0.0, 2e-4, 0.0]
    json.dumps(out)


def test_abi_declares_the_plastic_state():
    from pinn_fem_amd import _capi
    lib = _capi.load()
    header = open(os.path.join(ROOT, "include", "pinnfem_hip.h")).read()
    P, G, V = _capi._PP, _capi._PG, C.c_void_p
    decl = re.search(r"\bint pf_gl_state_plastic\(([^;]*)\);", header)
    assert decl
    assert [" ".join(a.split()) for a in decl.group(1).split(",")] == [
        "const pf_problem* p", "const pf_gl* g", "const double* ea", "const double* e0", "const pf_gl_plastic* pl",
        "const double* u", "void* stream"]
    assert _capi.SYMBOLS["pf_gl_state_plastic"] == (C.c_int, [P, G, V, V, C.POINTER(_capi.PfGlPlastic), V, V])
    assert hasattr(lib, "pf_gl_state_plastic")
    struct = re.search(r"typedef struct pf_gl_plastic \{(.*?)\} pf_gl_plastic;", header, re.S)
    names = [line.split(";")[0].split()[-1].lstrip("*") for line in struct.group(1).strip().splitlines()]
    assert names == [f[0] for f in _capi.PfGlPlastic._fields_] == ["ey", "kappa", "ep_n", "al_n", "ep", "al", "yielding", "counts"]
    assert lib.pf_sizeof(8) == C.sizeof(_capi.PfGlPlastic) == 64 and lib.pf_sizeof(9) == _capi.PF_ERR_ARG
    assert lib.pf_abi_version() == 9 == _capi.PF_ABI_VERSION and re.search(r"#define PF_ABI_VERSION 9\b", header)
    # the bar and cable entry points and the records keep their shapes
    assert _capi.SYMBOLS["pf_gl_state"] == (C.c_int, [P, G, V, V]) and _capi.SYMBOLS["pf_gl_state_e0"] == (C.c_int, [P, G, V, V, V, V])
    assert _capi.SYMBOLS["pf_gl_state_cable"] == (C.c_int, [P, G, V, V, V, V, V, V, V])
    assert [f[0] for f in _capi.PfGl._fields_] == ["d0", "kt", "fe", "strain"] and lib.pf_sizeof(6) == C.sizeof(_capi.PfGl)


def test_null_and_alias_operands_are_rejected_on_the_host():
    """A null record, a null pointer in it and an update in place are PF_ERR_ARG with a text that begins with the function's
    name, before the mesh is looked at and before any HIP call: this runs without a GPU."""
    from pinn_fem_amd import _capi
    lib = _capi.load()
    p, g = _capi.PfProblem(), _capi.PfGl()
    bufs = [(C.c_double * 4)() for _ in range(8)]
    names = [f[0] for f in _capi.PfGlPlastic._fields_]

    def record(**swap):
        pl = _capi.PfGlPlastic()
        for name, buf in zip(names, bufs):
            setattr(pl, name, swap.get(name, C.cast(buf, C.c_void_p)))
        return pl

    def call(pl):
        rc = lib.pf_gl_state_plastic(C.byref(p), C.byref(g), None, None, None if pl is None else C.byref(pl), None, None)
        return rc, lib.pf_last_error().decode()

    for pl in [None] + [record(**{name: None}) for name in names]:
        rc, text = call(pl)
        assert rc == _capi.PF_ERR_ARG and text.startswith("pf_gl_state_plastic: null plastic record or a null pointer in it"), text
        assert "pf_gl_state_e0" in text
    for out, inp in (("ep", "ep_n"), ("al", "al_n")):
        rc, text = call(record(**{out: C.cast(bufs[names.index(inp)], C.c_void_p)}))
        assert rc == _capi.PF_ERR_ARG and text.startswith("pf_gl_state_plastic: ep == ep_n or al == al_n"), text
    rc, text = call(record())
    assert rc == _capi.PF_ERR_ARG and text.startswith("pf_gl_state_plastic: bad argument")
