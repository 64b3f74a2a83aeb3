"""The Green-Lagrange truss element on the host: the float64 restatement of tests/gl_reference.py against finite
differences, rigid motions and the two-bar closed form, and the package's configuration, JSON and ABI surface of the
feature.  No GPU."""
import json
import os

import numpy as np
import pytest

import gl_reference as gl

U53 = 2.0 ** -53
HERE = os.path.dirname(os.path.abspath(__file__))


def _random_truss(rng, n_elems=10):
    nodes, el = gl.irregular_truss(n_elems, rng, hub_degree=3)
    return nodes, el, rng.uniform(0.5, 2.0, len(el))


def test_tangent_is_the_derivative_of_the_internal_force():
    """f_int is cubic in u, so the central difference (f(u + h v) - f(u - h v)) / 2h equals K_t v + h^2/6 f'''[v, v, v]
    EXACTLY, and the third derivative is elementwise 3 E A |dv|^2 dv / l0^3 (the t^3 coefficient of
    (|d + t dv|^2 - l0^2)(d + t dv), times 6 E A / (2 l0^3)).  What is left is round-off of the two force evaluations:
    each dof's force is a sum of terms of total magnitude F (f_int_scale) carrying some 10 roundings each, so
    |difference| <= 2 * 16 * 2^-53 F / (2 h), and K_t v itself rounds at 16 * 2^-53 |K_t||v|."""
    rng = np.random.default_rng(1)
    nodes, el, ea = _random_truss(rng)
    n = nodes.size
    u = 0.2 * rng.standard_normal(n)
    v = rng.standard_normal(n)
    h = 1e-4
    K, Kabs = gl.k_t(nodes, el, u, ea, 2), gl.k_t(nodes, el, u, ea, 2, absolute=True)
    fd = (gl.f_int(nodes, el, u + h * v, ea, 2) - gl.f_int(nodes, el, u - h * v, ea, 2)) / (2 * h)
    t = gl.element_state(nodes, el, u, ea, 2)[3]
    V = v.reshape(-1, 2)
    dv = V[el[:, 1]] - V[el[:, 0]]
    third = (3.0 * ea * np.sum(dv * dv, axis=1) / t["l0"] ** 3)[:, None] * dv
    trunc = np.zeros_like(V)
    np.add.at(trunc, el[:, 1], third)
    np.add.at(trunc, el[:, 0], -third)
    trunc = (h * h / 6.0) * trunc.reshape(-1)
    scale = np.maximum(gl.f_int_scale(nodes, el, u + h * v, ea, 2), gl.f_int_scale(nodes, el, u - h * v, ea, 2))
    bound = 16 * U53 * scale / h + 16 * U53 * (Kabs @ np.abs(v))
    err = np.abs(fd - K @ v - trunc)
    print(f"finite difference: worst error / bound {np.max(err / bound):.3f}; truncation term up to {np.max(np.abs(trunc)):.2e}; "
          f"relative to |K_t v| {np.max(err) / np.max(np.abs(K @ v)):.2e}")
    assert np.max(np.abs(trunc)) > 100 * np.max(bound)         # the truncation term is really there, and accounted for
    assert np.all(err <= bound)
    assert abs(K - K.T).max() == 0.0 or abs(K - K.T).max() <= 4 * U53 * abs(K).max()


def test_rigid_motion_gives_no_force():
    """A rotation plus translation of the whole mesh leaves every strain zero: 2 d0.du + du.du cancels.  The field is
    rigid only up to its rounding to float64 (rigid_motion_rounding), so the exact force of the rounded field
    (f_int_exact, rational arithmetic) is |K_t| times that rounding at most, and the float64 restatement is held to
    the round-off of its terms around it: 8 * 2^-53 of the terms' magnitude for the strain (f_int_scale) plus the
    roundings of the force itself (16 allowed in all)."""
    rng = np.random.default_rng(2)
    nodes, el, ea = _random_truss(rng, 40)
    shift = (3.0, -2.0)
    u = gl.rigid_motion(nodes, 0.7, shift)
    f, exact = gl.f_int(nodes, el, u, ea, 2), gl.f_int_exact(nodes, el, u, ea, 2)
    scale = gl.f_int_scale(nodes, el, u, ea, 2)
    from_rounding = gl.k_t(nodes, el, u, ea, 2, absolute=True) @ gl.rigid_motion_rounding(nodes, shift)
    print(f"rigid motion: max |f_int| {np.max(np.abs(f)):.2e} (E A up to {ea.max():.2f}), |f_int - exact| worst "
          f"{np.max(np.abs(f - exact) / scale) / U53:.2f} * 2^-53 scale, exact force {np.max(np.abs(exact) / from_rounding):.3f} "
          f"of what the field's rounding allows")
    assert np.all(np.abs(exact) <= from_rounding)
    assert np.all(np.abs(f - exact) <= 16 * U53 * scale)
    # the issue measured |f_int| <= 4e-16 E A on its own 10-element truss; the factor 4 is this test's allowance for a
    # field three times as far from the origin (its rounding is what the force is made of) and 40 elements
    assert np.max(np.abs(f)) <= 4 * 4e-16 * ea.max()
    # an exactly representable rigid motion (coordinates on a 2^-20 grid, quarter turn, dyadic shift): no rounding in the
    # field, every strain exactly zero, the force exactly zero
    grid = np.round(nodes * 2.0 ** 20) / 2.0 ** 20
    assert not gl.f_int(grid, el, gl.quarter_turn(grid, (3.0, -2.5)), ea, 2).any()
    # the exact force agrees with the restatement where nothing cancels, too
    u2 = 0.2 * rng.standard_normal(u.size)
    assert np.all(np.abs(gl.f_int(nodes, el, u2, ea, 2) - gl.f_int_exact(nodes, el, u2, ea, 2))
                  <= 16 * U53 * gl.f_int_scale(nodes, el, u2, ea, 2))
    # the linear element does not have this property
    K0 = gl.k_t(nodes, el, np.zeros_like(u), ea, 2)
    assert np.max(np.abs(K0 @ u)) > 1e-2 * ea.min()


def test_two_bar_truss_closed_form():
    tb = gl.TwoBar()
    assert abs(tb.p_lim - 0.379198) < 1e-6
    assert abs(tb.tangent(tb.w_lim)) < 1e-15 and abs(tb.tangent(tb.h) + 0.985) < 1e-3
    for frac, n_inc in ((0.5, 1), (0.9, 10)):
        p = frac * tb.p_lim
        u, its = gl.incremental(tb.nodes, tb.el, tb.loads(p), tb.fixed, tb.ea, 2, n_inc, tol=1e-10)
        w = -u[5]
        print(f"two-bar {frac} P_lim: w = {w:.15f}, P(w)/P - 1 = {tb.load(w) / p - 1:.2e}, Newton iterations {its}")
        assert 0 < w < tb.w_lim and u[4] == 0.0
        assert abs(tb.load(w) / p - 1.0) <= 8 * U53 * 10          # a converged Newton: a handful of roundings
        strain = gl.element_state(tb.nodes, tb.el, u, tb.ea, 2)[0]
        assert np.allclose(strain, tb.strain(w), rtol=1e-13, atol=0.0)
        # the tangent on the free dofs: horizontal 2 ea a^2 / l0^3 + 2 N / l0, vertical the closed form
        K = gl.k_t(tb.nodes, tb.el, u, tb.ea, 2).toarray()
        assert abs(K[5, 5] - tb.tangent(w)) <= 1e-13 * abs(K[5, 5]) and abs(K[4, 5]) <= 1e-13 * K[4, 4]


def test_bar_1d_closed_form():
    x = np.array([0.0, 2.5])
    for u1 in (0.4, -0.3, 1e-9):
        f = gl.f_int(x, np.array([[0, 1]]), np.array([0.0, u1]), 7.0, 1)
        want = gl.bar_1d_load(7.0, 2.5, u1)
        assert abs(f[1] - want) <= 8 * U53 * abs(want) and f[0] == -f[1]


# ---- the package's surface ------------------------------------------------------------------------------------------
def _two_bar_model(young=2000.0, area=0.5):
    from pinn_fem_amd.fem.model import FEMModel, Material
    tb = gl.TwoBar()
    return FEMModel(nodes=tb.nodes, elements=tb.el, material=Material(young, area, 1.0), loads=tb.loads(0.1),
                    fixed_dofs=tb.fixed, dimension=2)


def test_unknown_kinematics_is_rejected_with_the_accepted_values():
    from pinn_fem_amd.fem.solver import SolverConfig, solve_nr
    assert SolverConfig().kinematics == "linear"
    with pytest.raises(ValueError, match=r"unknown kinematics 'updated'.*'linear'.*'green-lagrange'"):
        solve_nr(_two_bar_model(), SolverConfig(kinematics="updated"))


def test_green_lagrange_rejects_two_level_nn_materials_and_sharded_runs(monkeypatch):
    """All three are refused before any engine (and so any GPU) is touched."""
    from pinn_fem_amd.fem import solver
    from pinn_fem_amd.fem.properties import NNProperty
    from pinn_fem_amd.nets import SimpleNN
    monkeypatch.setattr(solver, "_engine_for", lambda *a, **k: pytest.fail("an engine was built"))
    cfg = solver.SolverConfig(kinematics="green-lagrange")
    with pytest.raises(ValueError, match="two-level"):
        solver.solve_nr(_two_bar_model(), solver.SolverConfig(kinematics="green-lagrange", nr_preconditioner="two-level"))
    nn = NNProperty(net=SimpleNN(hidden_layers=1, neurons_per_layer=4, input_dim=3), input_dim=3, enforce_positive=True,
                    scale=2000.0)
    with pytest.raises(ValueError, match="NN materials"):
        solver.solve_nr(_two_bar_model(young=nn), cfg)
    monkeypatch.setattr(solver, "_world_size", lambda: 2)
    with pytest.raises(ValueError, match="sharded"):
        solver.solve_nr(_two_bar_model(), cfg)


def test_json_kinematics(tmp_path):
    from pinn_fem_amd.cli.generic import parse_problem
    path = os.path.join(HERE, "nl_inputs", "two_bar_green_lagrange.json")
    parsed = parse_problem(path)
    assert parsed["solver_config"].kinematics == "green-lagrange" and parsed["solver_config"].method == "nr"
    with open(path) as f:
        data = json.load(f)

    def parse_with(accel):
        p = tmp_path / "case.json"
        p.write_text(json.dumps(dict(data, accel=accel)))
        return parse_problem(str(p))

    assert parse_with({})["solver_config"].kinematics == "linear"
    with pytest.raises(ValueError, match=r"unknown kinematics 'corotational'.*'linear'.*'green-lagrange'"):
        parse_with({"kinematics": "corotational"})
    with pytest.raises(ValueError, match="two-level"):
        parse_with({"kinematics": "green-lagrange", "nr_preconditioner": "two-level"})
    assert parse_with({"kinematics": "linear", "nr_preconditioner": "two-level"})["solver_config"].nr_preconditioner == "two-level"


def test_abi_declares_the_green_lagrange_entry_points():
    import ctypes as C
    import re
    from pinn_fem_amd import _capi
    names = ("pf_gl_state", "pf_gl_fint", "pf_kt_v_f64", "pf_pcgt_begin", "pf_pcgt_iterations", "pf_pcgt_graph_create",
             "pf_pcgt_state")
    header = open(os.path.join(os.path.dirname(HERE), "include", "pinnfem_hip.h")).read()
    assert _capi.PF_ABI_VERSION == 9 and re.search(r"#define PF_ABI_VERSION 9\b", header)
    for name in names:
        assert name in _capi.SYMBOLS, name
        assert re.search(r"\bint %s\(" % name, header), name
    assert [f[0] for f in _capi.PfGl._fields_] == ["d0", "kt", "fe", "strain"]
    assert C.sizeof(_capi.PfGl) == 4 * C.sizeof(C.c_void_p)
    # kt follows p in every pf_pcgt_* signature: one more pointer than the pf_pcg_* twin
    for tail in ("begin", "iterations", "graph_create", "state"):
        lin, tan = _capi.SYMBOLS["pf_pcg_" + tail][1], _capi.SYMBOLS["pf_pcgt_" + tail][1]
        assert tan == lin[:1] + [C.c_void_p] + lin[1:], tail


def test_kinematics_in_the_other_solvers(monkeypatch):
    """solve_gd assembles the linear element: it says so when the configuration asks for green-lagrange.  solve_hybrid
    checks the name before it starts."""
    from pinn_fem_amd.fem import solver

    class Stop(Exception):
        pass

    def no_engine(*a, **k):
        raise Stop()
    monkeypatch.setattr(solver, "_engine_for", no_engine)
    with pytest.warns(RuntimeWarning, match="solve_gd uses the linear element"), pytest.raises(Stop):
        solver.solve_gd(_two_bar_model(), solver.SolverConfig(kinematics="green-lagrange"))
    with pytest.raises(ValueError, match="unknown kinematics"):
        solver.solve_hybrid(_two_bar_model(), solver.SolverConfig(kinematics="updated"))
    with pytest.raises(ValueError, match="two-level"):
        solver.solve_hybrid(_two_bar_model(), solver.SolverConfig(kinematics="green-lagrange", nr_preconditioner="two-level"))
