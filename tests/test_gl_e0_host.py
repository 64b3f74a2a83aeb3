"""Initial strains in the Green-Lagrange truss solve on the host: the float64 restatement of tests/gl_e0_reference.py against
finite differences and closed forms, then the package's configuration, JSON, CLI and ABI surface of the feature.  No GPU."""
import ctypes as C
import inspect
import json
import os
import re

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import gl_reference as gl
import gl_e0_reference as g0
from device_driver import truss_model

U53 = 2.0 ** -53
HERE = os.path.dirname(os.path.abspath(__file__))
EA = 1000.0


# ---- 1. the restatement ------------------------------------------------------------------------------------------------
def test_tangent_is_the_derivative_of_the_internal_force_with_a_random_e0():
    """tests/test_gl_host.py's argument carries over: e0 shifts N by a constant, so f_int stays cubic in u with the same
    third derivative 3 E A |dv|^2 dv / l0^3, and (f(u + h v) - f(u - h v)) / 2h = K_t v + h^2/6 f'''[v, v, v] exactly.  What is
    left is the round-off of the two force evaluations, 16 * 2^-53 of the terms' magnitude each (gl.f_int_scale: with
    |e0| next to e_abs, in front of the cancellation of e - e0), over h, and K_t v's own 16 * 2^-53 |K_t||v|."""
    rng = np.random.default_rng(1)
    nodes, el = gl.irregular_truss(10, rng, hub_degree=3)
    ea, e0 = rng.uniform(0.5, 2.0, len(el)), rng.uniform(-2e-2, 2e-2, len(el))
    n = nodes.size
    u, v, h = 0.2 * rng.standard_normal(n), rng.standard_normal(n), 1e-4
    K = gl.k_t(nodes, el, u, ea, 2, e0=e0)
    fd = (gl.f_int(nodes, el, u + h * v, ea, 2, e0=e0) - gl.f_int(nodes, el, u - h * v, ea, 2, e0=e0)) / (2 * h)
    t = gl.element_state(nodes, el, u, ea, 2, e0=e0)[3]
    V = v.reshape(-1, 2)
    dv = V[el[:, 1]] - V[el[:, 0]]
    third = (3.0 * ea * np.sum(dv * dv, axis=1) / t["l0"] ** 3)[:, None] * dv
    trunc = np.zeros_like(V)
    np.add.at(trunc, el[:, 1], third)
    np.add.at(trunc, el[:, 0], -third)
    trunc = (h * h / 6.0) * trunc.reshape(-1)
    scale = np.maximum(gl.f_int_scale(nodes, el, u + h * v, ea, 2, e0=e0), gl.f_int_scale(nodes, el, u - h * v, ea, 2, e0=e0))
    bound = 16 * U53 * scale / h + 16 * U53 * (abs(K) @ np.abs(v))
    err = np.abs(fd - K @ v - trunc)
    print(f"finite difference: worst error / bound {np.max(err / bound):.3f}, truncation term up to {np.max(np.abs(trunc)):.2e}")
    assert np.all(err <= bound)
    assert abs(K - K.T).max() <= 4 * U53 * abs(K).max()
    # the prestress is in the tangent: the geometric part differs from the unstrained element's by -(E A e0 / l0) I
    K_0 = gl.k_t(nodes, el, u, ea, 2)
    assert abs(K - K_0).max() > 1e-3 * abs(K_0).max()
    # and the force is the derivative of the energy sum E A l0 (e - e0)^2 / 2 (quartic: the h^2 term is f'' [v, v, v] / 6)
    W = lambda s: gl.energy(nodes, el, u + s * v, ea, 2, e0=e0)
    dW = (W(h) - W(-h)) / (2 * h)
    want = float(gl.f_int(nodes, el, u, ea, 2, e0=e0) @ v)
    assert abs(dW - want) <= 1e-6 * abs(want)        # h^2 = 1e-8 times W''' / W', which is of order 10 here


def test_zero_e0_is_the_unstrained_element_and_a_rigid_motion_gives_no_force():
    rng = np.random.default_rng(2)
    nodes, el = gl.irregular_truss(10, rng, hub_degree=3)
    ea = rng.uniform(0.5, 2.0, len(el))
    u = 0.2 * rng.standard_normal(nodes.size)
    for e0 in (0.0, np.zeros(len(el))):
        for a, b in zip(gl.element_state(nodes, el, u, ea, 2, e0=e0)[:3], gl.element_state(nodes, el, u, ea, 2)[:3]):
            assert np.array_equal(a, b)
    grid = np.round(nodes * 2.0 ** 20) / 2.0 ** 20
    assert not gl.f_int(grid, el, gl.quarter_turn(grid, (3.0, -2.5)), ea, 2, e0=0.0).any()
    # with an initial strain a rigid motion leaves the self-stress as it was, turned with the structure
    e0 = rng.uniform(-1e-3, 1e-3, len(el))
    f0 = gl.f_int(grid, el, np.zeros(grid.size), ea, 2, e0=e0).reshape(-1, 2)
    f1 = gl.f_int(grid, el, gl.quarter_turn(grid, (3.0, -2.5)), ea, 2, e0=e0).reshape(-1, 2)
    assert np.array_equal(f1, np.stack([-f0[:, 1], f0[:, 0]], axis=1))


def test_e0_omitted_zero_and_zeros_are_the_same_bytes():
    """The one element with its e0 keyword: omitted, 0.0 and np.zeros(ne) give the same bytes in element_state, f_int, k_t,
    element_sensitivity and newton, and a non-zero e0 changes every one of them.  A 2-D irregular truss of 257 elements with
    |du| / l0 of about 0.3 and a 1-D chain of 5; the Newton solves start from a tenth of that field under the internal
    force of another such field."""
    rng = np.random.default_rng(3)
    nodes, el = gl.irregular_truss(257, rng)
    fixed = np.unique(np.concatenate([[0, 1, 2], rng.choice(nodes.size, size=nodes.size // 10, replace=False)]))
    x, el1, fixed1 = g0.heated_bar(5)
    for X, elements, fix, dim in ((nodes, el, fixed, 2), (x, el1, fixed1, 1)):
        ne, n, P = len(elements), X.size, X.reshape(-1, dim)
        l0 = float(np.mean(np.linalg.norm(P[elements[:, 1]] - P[elements[:, 0]], axis=1)))
        u = 0.3 * l0 / np.sqrt(2.0 * dim) * rng.standard_normal(n)
        ea, a = rng.uniform(0.5, 2.0, ne), rng.standard_normal(n)
        free = gl.free_mask(n, fix)
        loads = gl.f_int(X, elements, np.where(free, 0.1 * u, 0.0), ea, dim)

        def everything(**kw):
            strain, fe, B, t = gl.element_state(X, elements, u, ea, dim, **kw)
            u_n, it, ok = gl.newton(X, elements, loads, fix, ea, dim, u0=0.1 * u[::-1], **kw)
            assert ok
            out = [strain, fe, B, t["n"], t["e0"], gl.f_int(X, elements, u, ea, dim, **kw),
                   gl.k_t(X, elements, u, ea, dim, **kw).toarray(), gl.element_sensitivity(X, elements, u, a, dim, **kw), u_n]
            return [np.ascontiguousarray(o).tobytes() for o in out], it

        plain, it = everything()
        assert everything(e0=0.0) == (plain, it) and everything(e0=np.zeros(ne)) == (plain, it)
        for e0 in (-2e-3, 1e-3 * rng.standard_normal(ne)):
            other = everything(e0=e0)[0]
            assert other[0] == plain[0]                                      # the total strain does not contain e0
            assert all(o != p for o, p in zip(other[1:], plain[1:]))


@pytest.mark.parametrize("e0", [-1e-3, -1e-2])
@pytest.mark.parametrize("p", [0.01, 1.0, 20.0])
def test_taut_string_closed_form(e0, p):
    """P = 2 E A (w^2 / (2 a^2) - e0) w / a at the Newton solution from u = 0; a converged Newton iteration on one dof
    leaves a handful of roundings: 16 * 2^-53.  K_ff stays positive definite at every iterate."""
    ts = g0.TautString(ea=EA, e0=e0)
    eigs = []
    u, it, ok = gl.newton(ts.nodes, ts.el, ts.loads(p), ts.fixed, EA, 2, tol=1e-10,
                          on_iterate=lambda u, K, free, rhs: eigs.append(gl.min_eig_ff(K, free)), e0=e0)
    w = u[3]
    print(f"taut string e0 = {e0}, P = {p}: {it} iterations, w = {w:.12f}, P(w)/P - 1 = {ts.load(w) / p - 1:.2e}, "
          f"smallest eigenvalue {min(eigs):.3e}")
    assert ok and 3 <= it <= 15 and u[2] == 0.0 and w > 0.0
    assert abs(ts.load(w) / p - 1.0) <= 16 * U53
    assert min(eigs) > 0.0
    n = gl.axial_forces(ts.nodes, ts.el, u, EA, 2, e0=e0)
    assert np.allclose(n, ts.force(w), rtol=1e-13, atol=0.0)
    # without the pretension the transverse dof has no stiffness at u = 0
    K0 = gl.k_t(ts.nodes, ts.el, np.zeros(6), EA, 2)
    assert K0[3, 3] == 0.0 and abs(gl.k_t(ts.nodes, ts.el, np.zeros(6), EA, 2, e0=e0)[3, 3] / (2.0 * EA * -e0) - 1.0) <= 4 * U53


def test_heated_bar_between_supports():
    """Uniform e0 = alpha dT on a 1-D chain of equal elements held at both ends: u = 0 is the solution and N = -E A e0
    exactly (the inner nodes see N - N)."""
    x, el, fixed = g0.heated_bar(12)
    e0 = 1.2e-5 * 40.0
    assert not gl.f_int(x, el, np.zeros(len(x)), EA, 1, e0=e0)[1:-1].any()
    u, it, ok = gl.newton(x, el, np.zeros(len(x)), fixed, EA, 1, e0=e0)
    assert ok and it == 1 and not u.any()
    n = gl.axial_forces(x, el, u, EA, 1, e0=e0)
    assert np.all(n == -EA * e0)
    f = gl.f_int(x, el, u, EA, 1, e0=e0)
    assert abs(f[0] / (EA * e0) - 1.0) <= 4 * U53 and f[-1] == -f[0]          # the supports hold the compression


def test_lack_of_fit_leaves_a_determinate_girder_stress_free():
    """cantilever_warren(8) with one support dof released is statically determinate (31 bars + 3 supports = 2 * 17): a
    random lack of fit moves it and stresses nothing.  Bound: the residual is evaluated with some 10 roundings of terms of
    E A |e0| per incidence, and a cantilever's bar forces answer a unit nodal force with up to 2 * n_panels (the lever arm
    span / height): 10 * 16 * 2^-53 E A max|e0|.  The clamped girder is once redundant and keeps a self-stress."""
    nodes, el, unit, fixed, _ = gl.cantilever_warren(8)
    e0 = np.random.default_rng(0).uniform(-2e-3, 2e-3, len(el))
    u, it, ok = gl.newton(nodes, el, 0.0 * unit, np.array([0, 1, 2]), EA, 2, e0=e0)
    n = gl.axial_forces(nodes, el, u, EA, 2, e0=e0)
    bound = 10 * 16 * U53 * EA * np.max(np.abs(e0))
    print(f"determinate girder: {it} iterations, max |u| = {np.max(np.abs(u)):.3e}, max |N| = {np.max(np.abs(n)):.2e} (bound {bound:.2e})")
    assert ok and np.max(np.abs(u)) > 1e-3 and np.max(np.abs(n)) <= bound
    u, it, ok = gl.newton(nodes, el, 0.0 * unit, fixed, EA, 2, e0=e0)
    n = gl.axial_forces(nodes, el, u, EA, 2, e0=e0)
    print(f"clamped girder: max |N| = {np.max(np.abs(n)):.3f}")
    assert ok and np.max(np.abs(n)) > 0.5


def test_prestressed_two_bar_closed_form():
    """P(w) = E A ((w^2 - 2 h w) / (2 l0^2) - e0) (w - h) 2 / l0 against the restatement's Newton solve below the limit
    point, as tests/test_gl_host.py holds the unstrained one: 8 * 2^-53 * 10."""
    tb = g0.PrestressedTwoBar(ea=EA, e0=-1e-3)
    assert abs(tb.tangent(tb.w_lim)) <= 1e-14 and tb.load(0.0) < 0.0 < tb.p_lim < gl.TwoBar(ea=EA).p_lim
    h = 1e-6
    assert abs((tb.load(0.3 + h) - tb.load(0.3 - h)) / (2 * h) - tb.tangent(0.3)) <= 1e-9
    for frac in (0.0, 0.3, 0.8):
        p = frac * tb.p_lim
        u, it, ok = gl.newton(tb.nodes, tb.el, tb.loads(p), tb.fixed, EA, 2, tol=1e-12, e0=tb.e0)
        w = -u[5]
        print(f"prestressed two-bar {frac} P_lim: {it} iterations, w = {w:.12f}, P(w) - P = {tb.load(w) - p:.2e}")
        assert ok and 0.0 < w < tb.w_lim and u[4] == 0.0
        assert abs(tb.load(w) - p) <= 80 * U53 * tb.p_lim
        K = gl.k_t(tb.nodes, tb.el, u, EA, 2, e0=tb.e0).toarray()
        assert abs(K[5, 5] - tb.tangent(w)) <= 1e-13 * abs(K[5, 5])


def test_cable_chain_converges_from_zero():
    """256 collinear unit elements, e0 = -1e-2, equal nodal loads for a sag of 2 % of the span: six Newton iterations from
    u = 0 with rhs.du > 0 throughout, and the Jacobi-CG run (the device solve's yardstick) lands on the direct one."""
    nodes, el, loads, fixed = g0.cable_chain(256)
    ascent = []

    def watch(u, K, free, rhs):
        du = np.zeros_like(rhs)
        du[free] = spla.spsolve(gl.restrict(K, free), rhs[free])
        ascent.append(float(rhs @ du))
    u, it, ok = gl.newton(nodes, el, loads, fixed, EA, 2, on_iterate=watch, e0=-1e-2)
    u_cg, it_cg, ok_cg = gl.newton(nodes, el, loads, fixed, EA, 2, linear_solve=gl.jacobi_cg(1e-13), e0=-1e-2)
    sag = -u[1::2].min() / 256.0
    print(f"cable chain: {it} iterations (CG {it_cg}), sag {sag:.4f} of the span, CG against direct "
          f"{np.max(np.abs(u_cg - u)) / np.max(np.abs(u)):.2e}")
    assert ok and ok_cg and it == it_cg == 6 and min(ascent) > 0.0 and 0.015 < sag < 0.02


def test_adjoint_gradient_against_central_differences():
    """dJ/dq of the prestressed girder (every group, all factors 1) against central differences of J at the steps h and
    h / 2.  Their own truncation error is known from the pair: fd(h) - fd(h / 2) is three times the error of fd(h / 2) to
    leading order, so |g - fd(h / 2)| is held to |fd(h) - fd(h / 2)|; to that comes the round-off of the differenced
    J: its Newton states carry cond(K) 2^-53, about 1e-12 relative, over h / 2.  The sensitivity without e0 (the
    unstrained kernel's) is off by far more than that."""
    case = g0.warren_case()
    q = np.zeros(case.n_groups)
    J, g = case.objective(q, tol=1e-12)
    fd = {}
    for h in (2e-3, 1e-3):
        fd[h] = np.array([(case.objective(q + h * np.eye(4)[k], tol=1e-12)[0] - case.objective(q - h * np.eye(4)[k], tol=1e-12)[0])
                          / (2 * h) for k in range(4)])
    bound = np.abs(fd[2e-3] - fd[1e-3]) + 1e-12 * J / 1e-3
    err = np.abs(g - fd[1e-3])
    print(f"adjoint gradient {g}: against central differences {err / np.abs(g)} relative, bound {bound / np.abs(g)}")
    assert np.all(err <= bound) and np.all(bound <= 1e-5 * np.abs(g))
    # -(e / l0) d.(a_j - a_i) in place of -((e - e0) / l0) d.(a_j - a_i), on the same states and adjoints
    sens = gl.element_sensitivity
    try:
        gl.element_sensitivity = lambda nodes, el, u, a, dim, e0: sens(nodes, el, u, a, dim, e0=0.0)
        g_blind = case.objective(q, tol=1e-12)[1]
    finally:
        gl.element_sensitivity = sens
    print(f"without e0 in the sensitivity: {np.abs(g_blind - g) / np.abs(g)} relative")
    assert np.all(np.abs(g_blind - fd[1e-3]) > 100 * bound)


def test_identification_needs_the_prestress():
    """The restatement's Levenberg-Marquardt on data generated with e0 in +-1e-3: with e0 in the model it recovers the
    factors to its own error; with e0 left out it misses them by more than 100 times that."""
    case, run = g0.reference_run(True)
    _, blind = g0.reference_run(False)
    err, err_blind = np.max(np.abs(run["factors"] - case.factors)), np.max(np.abs(blind["factors"] - case.factors))
    print(f"with e0: {run['evaluations']} evaluations, stop {run['stop']}, error {err:.2e}; without: {blind['evaluations']} "
          f"evaluations, stop {blind['stop']}, error {err_blind:.2e}")
    assert run["stop"] == "misfit" and err <= 1e-8 and err_blind > 100 * err and err_blind > 1e-2


# ---- 2. check_initial_strain -------------------------------------------------------------------------------------------
def _model(loads=None):
    ts = g0.TautString()
    return truss_model(ts.nodes, ts.el, ts.loads(1.0) if loads is None else loads, ts.fixed)


def test_every_refusal_of_check_initial_strain(monkeypatch):
    from pinn_fem_amd.fem import identify, solver
    monkeypatch.setattr(solver, "_engine_for", lambda *a, **k: pytest.fail("an engine was built"))
    model = _model()
    cfg = lambda e0, **kw: solver.SolverConfig(kinematics="green-lagrange", initial_strain=e0, **kw)

    def refused(match, config):
        with pytest.raises(ValueError, match=match):
            solver.check_initial_strain(config, model)
        with pytest.raises(ValueError, match=match):
            solver.solve_nr(model, config, 1.0)
        config.method = "nr"
        with pytest.raises(ValueError, match=match):
            solver.solve(model, config)
        levels = [(1.0, [3], [0.1])]
        for run in (lambda: identify.misfit_and_gradient(model, config, levels, np.full(2, EA)),
                    lambda: identify.residuals_and_jacobian(model, config, levels, np.full(2, EA), [0, 0]),
                    lambda: identify.identify_nr(model, config, levels, groups=[0, 0])):
            with pytest.raises(ValueError):
                run()

    linear = solver.SolverConfig(initial_strain=-1e-3)
    refused("needs kinematics 'green-lagrange'", linear)
    with pytest.raises(ValueError, match="solve_gd and the linear solve_nr are untouched"):
        solver.check_initial_strain(linear, model)
    refused("initial_strain has 3 entries, the model has 2 elements", cfg([0.0, 0.0, 0.0]))
    refused("initial_strain has 1 entries, the model has 2 elements", cfg([0.0]))
    for bad in (np.nan, np.inf, -np.inf):
        refused("non-finite", cfg([0.0, bad]))
        refused("non-finite", cfg(bad))
    for bad in (0.5, -0.5, 0.7, [0.0, -0.6]):
        refused("smaller than 0.5 in magnitude", cfg(bad))
    refused("must be a number or 2 numbers", cfg("tight"))
    # displacement control runs the same check first; the GD methods are untouched by an initial strain and say so
    refused("smaller than 0.5", cfg(0.5, nr_control="displacement", nr_control_dof=3, nr_control_displacement=0.1))
    for method in ("gd", "full-nr"):
        with pytest.raises(ValueError, match="belongs to the Green-Lagrange Newton solve"):
            solver.solve(model, cfg(-1e-3, method=method))


def test_check_initial_strain_on_good_values():
    from pinn_fem_amd.fem import solver
    model = _model()
    cfg = lambda e0: solver.SolverConfig(kinematics="green-lagrange", initial_strain=e0)
    assert solver.SolverConfig().initial_strain is None
    assert solver.check_initial_strain(solver.SolverConfig(), model) is None
    assert solver.check_initial_strain(cfg(None), model) is None
    for given in (-1e-3, np.float32(-1e-3), [-1e-3, 2e-3], np.array([-1e-3, 2e-3]), (0, 0.25)):
        out = solver.check_initial_strain(cfg(given), model)
        assert out.dtype == np.float64 and out.shape == (2,) and out.flags.c_contiguous
        assert np.array_equal(out, np.broadcast_to(np.asarray(given, dtype=np.float64), (2,)))
    fields = list(solver.SolverResult.__dataclass_fields__)
    assert fields[-1] == "axial_forces" and solver.SolverResult.__dataclass_fields__["axial_forces"].default is None
    assert list(inspect.signature(solver.check_initial_strain).parameters) == ["config", "model"]


def test_engine_signatures():
    from pinn_fem_amd.engine import HipEngine
    sig = inspect.signature(HipEngine.gl_state).parameters
    assert list(sig) == ["self", "u", "ea", "e0"] and sig["e0"].default is None
    sig = inspect.signature(HipEngine.gl_sensitivity).parameters
    assert list(sig) == ["self", "u", "a", "out", "e0"] and sig["e0"].default is None
    assert list(inspect.signature(HipEngine.kt_diag).parameters) == ["self"]


# ---- 3. JSON, CLI, ABI -------------------------------------------------------------------------------------------------
def test_json_key(tmp_path):
    from pinn_fem_amd.cli.generic import parse_problem
    path = os.path.join(HERE, "nl_inputs", "taut_string.json")
    parsed = parse_problem(path)
    cfg = parsed["solver_config"]
    assert cfg.initial_strain == -1e-3 and cfg.kinematics == "green-lagrange" and cfg.method == "nr"
    ts = g0.TautString(ea=EA, e0=-1e-3)
    model = parsed["model"]
    assert np.array_equal(model.nodes, ts.nodes) and np.array_equal(model.elements, ts.el)
    assert np.array_equal(model.loads, ts.loads(1.0)) and sorted(model.fixed_dofs) == ts.fixed.tolist()
    with open(path) as f:
        data = json.load(f)

    def parse_with(value):
        accel = dict(data["accel"])
        if value is None:
            del accel["initial_strain"]
        else:
            accel["initial_strain"] = value
        (tmp_path / "case.json").write_text(json.dumps(dict(data, accel=accel)))
        return parse_problem(str(tmp_path / "case.json"))["solver_config"]

    assert parse_with(None).initial_strain is None
    assert parse_with([-1e-3, 2e-3]).initial_strain == [-1e-3, 2e-3] and parse_with(0).initial_strain == 0.0
    for bad in ("tight", [0.0, "x"], True, [True, 0.0], {"value": 0.0}, [[0.0, 0.0]]):
        with pytest.raises(ValueError, match="accel.initial_strain must be a number or a list"):
            parse_with(bad)
    # an input without the key parses to the configuration it always gave
    old = parse_problem(os.path.join(HERE, "nl_inputs", "two_bar_green_lagrange.json"))["solver_config"]
    assert old.initial_strain is None


def test_res_json_gains_axial_forces_only_with_an_initial_strain(monkeypatch):
    from pinn_fem_amd.cli import generic
    from pinn_fem_amd.fem import solver

    def fake(axial):
        return lambda **kw: solver.SolverResult(displacements=np.zeros((3, 2)), reactions=np.zeros((3, 2)), converged=True,
                                                history=[{"iterations": 1.0}], axial_forces=axial)
    parsed = {"model": _model(), "solver_config": solver.SolverConfig(), "measured_data": {}, "accel": {}}
    monkeypatch.setattr(generic, "solve", fake(None))
    old_keys = ["success", "converged", "iterations", "history", "displacements", "reactions"]
    assert list(generic.solve_problem(parsed)) == old_keys
    monkeypatch.setattr(generic, "solve", fake(np.array([1.0, 2.0])))
    out = generic.solve_problem(parsed)
    assert sorted(out) == sorted(old_keys + ["axial_forces"]) and out["axial_forces"] == [1.0, 2.0]
    json.dumps(out)
    out = generic.solve_problem(dict(parsed, accel={"compact_output": True}))
    assert "axial_forces" not in out and np.array_equal(out["_arrays"]["axial_forces"], [1.0, 2.0])


def test_abi_declares_the_three_entry_points():
    from pinn_fem_amd import _capi
    header = open(os.path.join(os.path.dirname(HERE), "include", "pinnfem_hip.h")).read()
    assert _capi.PF_ABI_VERSION == 9 and re.search(r"#define PF_ABI_VERSION 9\b", header)
    P, G, V, I = _capi._PP, _capi._PG, C.c_void_p, C.c_int
    want = {
        "pf_gl_state_e0": (["const pf_problem* p", "const pf_gl* g", "const double* ea", "const double* e0", "const double* u",
                            "void* stream"], [P, G, V, V, V, V]),
        "pf_gl_sens_e0": (["const pf_problem* p", "const pf_gl* g", "const double* e0", "const double* u", "const double* a",
                           "int accumulate", "double* out", "void* stream"], [P, G, V, V, V, I, V, V]),
        "pf_kt_diag_f64": (["const pf_problem* p", "const double* kt", "double* out", "void* stream"], [P, V, V, V]),
    }
    for name, (params, argtypes) in want.items():
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert decl, name
        assert [" ".join(a.split()) for a in decl.group(1).split(",")] == params, name
        assert _capi.SYMBOLS[name] == (C.c_int, argtypes), name
    # the entry points they extend keep their signatures, and no struct changed
    assert _capi.SYMBOLS["pf_gl_state"] == (C.c_int, [P, G, V, V]) and _capi.SYMBOLS["pf_gl_state_ea"] == (C.c_int, [P, G, V, V, V])
    assert _capi.SYMBOLS["pf_gl_sens"] == (C.c_int, [P, G, V, V, I, V, V])
    assert [f[0] for f in _capi.PfGl._fields_] == ["d0", "kt", "fe", "strain"]
    assert C.sizeof(_capi.PfGl) == 4 * C.sizeof(C.c_void_p)


def test_nr_scale_takes_an_initial_strain():
    tool = open(os.path.join(os.path.dirname(HERE), "tools", "nr_scale.py")).read()
    assert re.search(r'"--initial-strain",\s*type=float,\s*default=None', tool) and "initial_strain=args.initial_strain" in tool
