"""Identification of a prestress on the CPU: the restatement tests/identify_prestress_reference.py against finite
differences and its own evaluation counts, the covariance under noise, every refusal of check_prestress before an engine is
built, the rejected-trial rule of the loop, and the JSON / CLI / ABI / tool surface.  No GPU.
"""
import ctypes as C
import inspect
import json
import os
import re

import numpy as np
import pytest

import gl_reference as gl
import identify_prestress_reference as pr
import identify_reference as ir
from device_driver import case_model

HERE = os.path.dirname(os.path.abspath(__file__))
U53 = 2.0 ** -53
POINTS = ((np.zeros(4), np.zeros(4)), (np.array([0.1, -0.2, 0.05, 0.3]), np.array([-5e-4, 2e-4, 3e-4, -1e-4])))


# ---- 1. the right-hand side and the Jacobian -----------------------------------------------------------------------------
def test_prestress_rhs_is_the_difference_quotient_of_the_internal_force():
    """f_int is affine in e0, so (f_int(e0) - f_int(e0 + tau 1_h)) / tau is row h exactly; e0 in multiples of 2^-20 and
    tau = 2^-10 make e0 + tau exact.  Allowed, per dof: each f_int carries at most (16 + deg) 2^-53 of gl.f_int_scale (the 16
    roundings of fe's chain on the magnitude in front of the cancellation of e - e0, test_gl_e0_f64.py's count, and deg - 1
    of the node sum), their difference 2^-53 (|f1| + |f2|), all over tau; the row itself (5 + deg) 2^-53 of
    gl.prestress_rhs_scale (6 roundings per term, deg - 1 of the sum)."""
    case = pr.warren_case(True, True)
    rng = np.random.default_rng(3)
    n = len(case.loads)
    u = 0.2 * rng.standard_normal(n)
    ea = case.ea(POINTS[1][0])
    e0 = rng.integers(-1000, 1001, len(case.el)) * 2.0 ** -20
    tau = 2.0 ** -10
    deg = np.repeat(np.bincount(case.el.reshape(-1), minlength=n // 2), 2)
    rows = gl.prestress_rhs(case.nodes, case.el, u, ea, case.pgroups, 4, 2)
    scale = gl.prestress_rhs_scale(case.nodes, case.el, u, ea, case.pgroups, 4, 2)
    f1 = gl.f_int(case.nodes, case.el, u, ea, 2, e0=e0)
    s1 = gl.f_int_scale(case.nodes, case.el, u, ea, 2, e0=e0)
    for h in range(4):
        e0_h = e0 + tau * (case.pgroups == h)
        f2 = gl.f_int(case.nodes, case.el, u, ea, 2, e0=e0_h)
        s2 = gl.f_int_scale(case.nodes, case.el, u, ea, 2, e0=e0_h)
        allowed = ((16 + deg) * U53 * (s1 + s2) + U53 * (np.abs(f1) + np.abs(f2))) / tau + (5 + deg) * U53 * scale[h]
        err = np.abs((f1 - f2) / tau - rows[h])
        print(f"group {h}: worst error / allowed {np.max(err / allowed):.3f}, max |row| {np.max(np.abs(rows[h])):.3e}")
        assert np.all(err <= allowed) and np.any(rows[h] != 0.0)
    # elements of no group (-1) and ids above the range add nothing
    stray = np.where(np.arange(len(case.el)) % 3 == 0, -1, case.pgroups)
    part = gl.prestress_rhs(case.nodes, case.el, u, ea, stray, 4, 2)
    rest = gl.prestress_rhs(case.nodes, case.el, u, ea, np.where(stray == -1, case.pgroups, -1), 4, 2)
    assert np.allclose(part + rest, rows, rtol=0.0, atol=8 * U53 * np.max(scale))


def _central(case, q, t, h):
    fd = np.zeros((case.n_rows, 8))
    for c in range(8):
        e = np.zeros(8)
        e[c] = h
        up = ir.case_residuals(case, q + e[:4], jacobian=False, tol=1e-12, t=t + e[4:])[0]
        down = ir.case_residuals(case, q - e[:4], jacobian=False, tol=1e-12, t=t - e[4:])[0]
        fd[:, c] = (up - down) / (2 * h)
    return fd


def test_jacobian_and_gradient_against_central_differences():
    """A_q and A_t against (rho(x + h e_c) - rho(x - h e_c)) / 2h and 2 A^T rho against the central difference of J = rho.rho,
    h = 1e-5 in q and in t (strain units), states converged to 1e-12.  Bound 1e-8 of the largest entry of the block (the two
    blocks differ by an order of magnitude), test_identify_gn_host.py's: the truncation term is h^2 = 1e-10 times
    rho''' / 6 rho' = O(10); t enters like q, through forces E A t against E A, so its scale of nonlinearity is O(1) too.
    The gradient is not small against its own truncation term where rho is small, so it gets an absolute bound per
    component c from the same O(10) per derivative (|rho''| <= 10 |rho'|, |rho'''| <= 100 |rho'|, rho' = A_c):
    J''' = 6 rho'.rho'' + 2 rho.rho''', so h^2 J''' / 6 <= h^2 (10 |A_c|^2 + 34 |rho| |A_c|), plus the rounding of the two
    sums of 90 squares over h, 100 * 2^-53 J / h."""
    case = pr.warren_case(True, True)
    h = 1e-5
    for q, t in POINTS:
        rho, A, _, _ = ir.case_residuals(case, q, tol=1e-12, t=t)
        fd = _central(case, q, t, h)
        g, g_fd = 2.0 * A.T @ rho, np.zeros(8)
        for c in range(8):
            e = np.zeros(8)
            e[c] = h
            up = ir.case_residuals(case, q + e[:4], jacobian=False, tol=1e-12, t=t + e[4:])[0]
            down = ir.case_residuals(case, q - e[:4], jacobian=False, tol=1e-12, t=t - e[4:])[0]
            g_fd[c] = (up @ up - down @ down) / (2 * h)
        norms, r = np.linalg.norm(A, axis=0), np.linalg.norm(rho)
        g_allowed = h * h * (10.0 * norms ** 2 + 34.0 * r * norms) + 100 * U53 * (rho @ rho) / h
        for name, cols in (("A_q", slice(0, 4)), ("A_t", slice(4, 8))):
            err = np.max(np.abs(A[:, cols] - fd[:, cols])) / np.max(np.abs(A[:, cols]))
            g_err = np.max(np.abs(g[cols] - g_fd[cols]) / g_allowed[cols])
            print(f"q = {q}, t = {t}: max |{name}| = {np.max(np.abs(A[:, cols])):.3e}, against differences {err:.2e}; its part of "
                  f"2 A^T rho (max {np.max(np.abs(g[cols])):.3e}) against the difference of J: error / allowed {g_err:.3f}")
            assert err <= 1e-8 and g_err <= 1.0
        assert A.shape == (90, 8) and rho.shape == (90,)


def test_joint_jacobian_is_well_conditioned():
    """The singular values of the joint Jacobian at x = 0 with unit columns: 2.1 .. 0.080, so the eight
    parameters are determined together; the raw columns differ by the scale gap, which the LM step does not see."""
    case = pr.warren_case(True, True)
    A = ir.case_residuals(case, np.zeros(4), t=np.zeros(4))[1]
    norms = np.linalg.norm(A, axis=0)
    s = np.linalg.svd(A / norms, compute_uv=False)
    print(f"column norms {norms}, singular values of the unit-column Jacobian {s}")
    assert abs(s[0] - 2.1) <= 0.05 and abs(s[-1] - 0.080) <= 0.005 and s[0] / s[-1] < 30.0
    assert norms[4:].min() > norms[:4].max()


# ---- 2. the loop ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, count", [("warren-prestress", 3), ("warren-prestress-no-base", 3), ("warren-joint", 5),
                                         ("warren-joint-no-base", 5), ("cable", 5)])
def test_levenberg_marquardt_evaluation_counts(name, count):
    """With misfit_tolerance 1e-15 from x = 0 (the cable: t = -5e-3): 3 evaluations for the offsets alone, 5 for offsets and
    factors, 5 for the cable, every step accepted, and the count does not hinge on round-off: the last misfit above 1e-15
    is more than 150 times it and the first below more than 150 times under it."""
    case, run = pr.reference_run(name)
    misfits = [h["misfit"] for h in run["history"]]
    t_err = np.max(np.abs(run["t"] - case.offsets))
    q_err = np.max(np.abs(run["factors"] - case.factors)) if case.n_q else 0.0
    print(f"{name}: {run['evaluations']} evaluations, stop {run['stop']!r}, J per evaluation {[f'{m:.1e}' for m in misfits]}, "
          f"t error {t_err:.2e}, factor error {q_err:.2e}")
    assert run["evaluations"] == count == len(misfits) and run["stop"] == "misfit"
    assert all(h["accepted"] for h in run["history"])
    assert misfits[-2] > 150 * 1e-15 and misfits[-1] < 1e-15 / 150
    assert t_err <= 1e-8 and q_err <= 1e-8


def test_left_out_prestress_goes_into_the_factors():
    """The factors alone, fitted to the measurements of the prestressed structure without the offsets (the base e0 known):
    an error above 1e-2 in the factors, against 1e-9 with the offsets identified alongside (the reason for identifying
    the prestress)."""
    case = pr.warren_case(True, True)
    blind = ir.Case(case.nodes, case.el, case.loads, case.fixed, 0, case.ea0, case.groups, case.factors, case.levels,
                    e0=case.e0_base)
    run = ir.identify_factors(blind, misfit_tolerance=1e-15, max_evaluations=30, e0=case.e0_base)
    err = np.max(np.abs(run["factors"] - case.factors))
    print(f"factors without the offsets: {run['factors']}, error {err:.3f}, misfit {run['misfit']:.2e}, stop {run['stop']!r}")
    assert err > 1e-2 and run["misfit"] > 1e-9


def test_cable_from_a_nearly_slack_start_and_the_slack_refusal():
    """The cable from t = -1e-3 (a tenth of its pretension) with next to no damping still arrives at -1e-2; from t = 0 the
    first evaluation is refused (no stiffness across), and that error propagates."""
    case = pr.cable_case()
    run = ir.identify_prestress(case, t0=np.array([-1e-3]), damping=1e-9, misfit_tolerance=1e-15)
    print(f"cable from -1e-3: {run['evaluations']} evaluations, stop {run['stop']!r}, history {run['history']}")
    assert run["stop"] == "misfit" and abs(run["t"][0] + 1e-2) <= 1e-9
    with pytest.raises(ir.Refused, match="slack"):
        ir.identify_prestress(case, t0=np.zeros(1))


def test_noisy_measurements_and_the_covariance():
    """Gaussian noise of 1e-4 on every measurement (seed 0), test_identify_gn_host.py's rule: the loop stops on the gradient
    or the step; the estimated standard deviations of (q, t) are those of sigma^2 (A~^T A~)^-1 with the known sigma and
    the unweighted Jacobian A~ = sqrt|m| A to within three standard errors of a variance estimate, 3 / sqrt(2 (M - P));
    and every parameter lies within 4 estimated standard deviations of the truth."""
    case = pr.noisy_case()
    run = ir.identify_prestress(case)
    A = run["jacobian"]
    M, P = A.shape
    std = np.sqrt(np.diag(pr.covariance(A, run["misfit"])))
    m = len(case.levels[0][1])
    known = np.sqrt(np.diag(pr.covariance(np.sqrt(m) * A, pr.NOISE_SIGMA ** 2 * (M - P))))
    off = (np.concatenate([run["q"] - np.log(case.factors), run["t"] - case.offsets])) / std
    print(f"noisy: {run['evaluations']} evaluations, stop {run['stop']!r}, J = {run['misfit']:.3e}, std of (q, t) {std}, "
          f"std / known - 1 = {std / known - 1.0} (allowed {3 / np.sqrt(2 * (M - P)):.3f}), (x - x_true) / std = {off}")
    assert run["stop"] in ("gradient", "step") and (M, P) == (90, 8)
    assert np.max(np.abs(std / known - 1.0)) <= 3.0 / np.sqrt(2.0 * (M - P))
    assert np.max(np.abs(off)) <= 4.0


def test_the_loop_rejects_a_trial_whose_evaluation_raises():
    """prestress._levenberg_marquardt on rho(x) = x - (1, 2) with an evaluation that raises RuntimeError on its second call
    only: that trial is a rejected step (accepted False, misfit None, the message under "error", mu 10 times larger next),
    it counts as an evaluation, and the loop goes on to the solution.  The first evaluation's error propagates."""
    from pinn_fem_amd.fem import prestress
    target = np.array([1.0, 2.0])
    calls = []

    def evaluate(x, states=None, jacobian=True):
        calls.append((x.copy(), states, jacobian))
        if len(calls) == 2:
            raise RuntimeError("Tangent stiffness is not positive definite at the starting state: slack")
        return x - target, (np.eye(2) if jacobian else None), ["state"]

    describe = lambda x: {"factors": None, "prestress": x.copy()}
    x, rho, A, states, history, stop, evaluations = prestress._levenberg_marquardt(
        evaluate, np.zeros(2), describe, 50, 1e-12, 1e-20, 1e-3, 1e-12)
    print(f"stop {stop!r}, {evaluations} evaluations, history {history}")
    assert stop == "misfit" and np.allclose(x, target, atol=1e-9) and evaluations == len(history)
    assert history[1]["accepted"] is False and history[1]["misfit"] is None and "slack" in history[1]["error"]
    assert history[1]["damping"] == 1e-3 and history[2]["damping"] == pytest.approx(1e-2) and history[2]["accepted"]
    assert all("error" not in h for i, h in enumerate(history) if i != 1)
    assert calls[1][2] is False and calls[3][1] == ["state"]          # the trial without a Jacobian, A at the trial's states

    def broken(x, **kw):
        raise RuntimeError("no stiffness")
    with pytest.raises(RuntimeError, match="no stiffness"):
        prestress._levenberg_marquardt(broken, np.zeros(2), describe, 50, 1e-12, 0.0, 1e-3, 1e-12)


def test_the_loop_without_rejection_propagates_a_trial_error_and_is_the_same_loop():
    """identify._levenberg_marquardt with reject_errors=False, as identify_nr(method="gauss-newton") runs it: the evaluation
    of the test above, which raises on its second call, propagates.  On the linear problem without that fault the two settings
    take the same path: the same x, stop, evaluations and history values; identify_nr's describe gives its entries no
    "prestress" key, and neither run has an "error" key."""
    from pinn_fem_amd.fem import identify, prestress
    assert prestress._levenberg_marquardt is identify._levenberg_marquardt
    target = np.array([1.0, 2.0])
    calls = []

    def evaluate(x, states=None, jacobian=True):
        calls.append(jacobian)
        if len(calls) == 2:
            raise RuntimeError("Tangent stiffness is not positive definite at the starting state: slack")
        return x - target, (np.eye(2) if jacobian else None), ["state"]

    factors = lambda x: {"factors": np.exp(x)}
    with pytest.raises(RuntimeError, match="slack"):
        identify._levenberg_marquardt(evaluate, np.zeros(2), factors, 50, 1e-12, 1e-20, 1e-3, 1e-12, reject_errors=False)
    assert calls == [True, False]                                   # it ended at the trial

    linear = lambda x, states=None, jacobian=True: (x - target, (np.eye(2) if jacobian else None), ["state"])
    both = lambda x: {"factors": np.exp(x), "prestress": x.copy()}
    plain = identify._levenberg_marquardt(linear, np.zeros(2), factors, 50, 1e-12, 1e-20, 1e-3, 1e-12, reject_errors=False)
    rejecting = identify._levenberg_marquardt(linear, np.zeros(2), both, 50, 1e-12, 1e-20, 1e-3, 1e-12, reject_errors=True)
    print(f"stop {plain[5]!r}, {plain[6]} evaluations, history {plain[4]}")
    assert plain[5] == rejecting[5] == "misfit" and plain[6] == rejecting[6] == len(plain[4]) == len(rejecting[4])
    for a, b in zip(plain[:3], rejecting[:3]):                      # x, rho, A
        assert np.array_equal(a, b)
    assert np.allclose(plain[0], target, atol=1e-9)
    for h, g in zip(plain[4], rejecting[4]):
        assert list(h) == ["misfit", "gradient_norm", "factors", "accepted", "damping"]
        assert list(g) == ["misfit", "gradient_norm", "factors", "prestress", "accepted", "damping"]
        assert all(np.array_equal(h[key], g[key]) for key in h) and h["accepted"] is True


# ---- 3. refusals ----------------------------------------------------------------------------------------------------
def _model():
    case = ir.warren_case(8)
    return case, case_model(case)


def test_every_refusal_is_a_value_error_before_an_engine_is_built(monkeypatch):
    from pinn_fem_amd.fem import prestress, solver
    from pinn_fem_amd.fem.properties import NNProperty
    from pinn_fem_amd.nets import SimpleNN
    monkeypatch.setattr(solver, "_engine_for", lambda *a, **k: pytest.fail("an engine was built"))
    case, model = _model()
    cfg = solver.SolverConfig(kinematics="green-lagrange", max_iterations=50, tolerance=1e-10)
    pg = case.groups

    def refused(match, levels=case.levels, pgroups=pg, config=cfg, mdl=model, **kw):
        with pytest.raises(ValueError, match=match):
            prestress.identify_prestress(mdl, config, levels, pgroups, **kw)
        with pytest.raises(ValueError, match=match):
            prestress.check_prestress(mdl, config, levels, pgroups, kw.get("t0"), kw.get("groups"), kw.get("q0"))

    refused("prestress group map has the wrong length", pgroups=pg[:-1])
    refused("must hold integer group ids", pgroups=pg.astype(float))
    refused("ids below -1", pgroups=np.where(np.arange(31) == 3, -2, pg))
    refused(r"prestress groups \[2\] have no element", pgroups=np.where(pg == 2, 4, pg))
    refused("identifies no element", pgroups=np.full(31, -1))
    refused("t0 has 3 entries for 4 prestress groups", t0=np.zeros(3))
    refused("t0 holds non-finite", t0=np.array([0.0, np.nan, 0.0, 0.0]))
    refused("t0 holds non-finite", t0=np.array([0.0, np.inf, 0.0, 0.0]))
    one_row = [(lam, dofs[:2], u[:2]) for lam, dofs, u in case.levels]
    refused("4 prestress groups and 4 stiffness groups for 6 measurement rows", levels=one_row, groups=case.groups)
    refused("4 prestress groups and 0 stiffness groups for 3 measurement rows", levels=[(l, d[:1], u[:1]) for l, d, u in case.levels])
    # what check_identify and check_strains refuse
    refused("needs kinematics 'green-lagrange'", config=solver.SolverConfig())
    refused("load control only", config=solver.SolverConfig(kinematics="green-lagrange", nr_control="displacement", nr_control_dof=33,
                                                            nr_control_displacement=-1.0))
    refused("levels is empty", levels=[])
    refused("negative group ids", groups=np.where(np.arange(31) == 3, -1, case.groups))
    refused("q0 has 3 entries", groups=case.groups, q0=np.zeros(3))
    refused("go together", levels=[dict(load_factor=1.0, dofs=[4], u=[0.0], strains=[0.0])])
    nn = NNProperty(net=SimpleNN(hidden_layers=1, neurons_per_layer=4, input_dim=3), input_dim=3, scale=2000.0)
    from pinn_fem_amd.fem.model import FEMModel, Material
    nn_model = FEMModel(nodes=case.nodes, elements=case.el, material=Material(nn, 0.5, 1.0), loads=case.loads,
                        fixed_dofs=case.fixed, dimension=2)
    refused("scalar materials", mdl=nn_model)
    monkeypatch.setattr(solver, "_world_size", lambda: 2)
    refused("sharded")
    monkeypatch.setattr(solver, "_world_size", lambda: 1)
    # identify_prestress's own: the scale, the damping, the cap, an empty stiffness group
    for kw, match in ((dict(prestress_scale=0.0), "prestress_scale"), (dict(prestress_scale=np.nan), "prestress_scale"),
                      (dict(damping=0.0), "damping must be positive"), (dict(max_evaluations=0), "max_evaluations"),
                      (dict(groups=np.where(case.groups == 2, 4, case.groups)), r"groups \[2\] have no element")):
        with pytest.raises(ValueError, match=match):
            prestress.identify_prestress(model, cfg, case.levels, pg, **kw)
    # what check_prestress passes
    levels, pgo, t, groups, q, rows = prestress.check_prestress(model, cfg, case.levels, np.where(pg == 3, -1, pg))
    assert len(levels) == 3 and pgo.dtype == np.int64 and t.shape == (3,) and groups is None and q.shape == (0,) and rows == 90
    assert prestress.check_prestress(model, cfg, case.levels, pg, groups=case.groups)[4].shape == (4,)


# ---- 4. surface -----------------------------------------------------------------------------------------------------
def test_exports_and_signatures():
    import pinn_fem_amd.fem as fem
    from pinn_fem_amd.fem import identify, prestress
    for name in ("PrestressResult", "check_prestress", "identify_prestress", "residuals_and_jacobian_prestress"):
        assert getattr(fem, name) is getattr(prestress, name) and name in fem.__all__
    assert list(prestress.PrestressResult.__dataclass_fields__) == [
        "prestress", "initial_strain", "factors", "ea", "misfit", "evaluations", "converged", "stop", "history", "displacements",
        "strains", "reactions", "axial_forces", "counters", "jacobian", "singular_values", "covariance", "prestress_std",
        "factor_std"]
    sig = inspect.signature(prestress.identify_prestress).parameters
    assert list(sig) == ["model", "config", "levels", "prestress_groups", "groups", "t0", "q0", "prestress_scale",
                         "max_evaluations", "gtol", "misfit_tolerance", "damping", "step_tolerance"]
    assert [sig[k].default for k in list(sig)[7:]] == [1e-3, 50, 1e-12, 0.0, 1e-3, 1e-12]
    sig = inspect.signature(prestress.residuals_and_jacobian_prestress).parameters
    assert list(sig) == ["model", "config", "levels", "prestress_groups", "t", "groups", "q", "states", "jacobian"]
    # the loops and the counters are identify.py's own, not copies
    assert prestress._newton_level is identify._newton_level and prestress._GN_COUNTERS is identify._GN_COUNTERS
    assert "fem/prestress.py identifies it" in identify.__doc__
    from pinn_fem_amd.engine import HipEngine
    assert list(inspect.signature(HipEngine.gl_prestress_rhs).parameters) == ["self", "u", "ea", "groups", "g0", "m"]


def test_json_blocks(tmp_path):
    from pinn_fem_amd.cli.generic import parse_problem
    path = os.path.join(HERE, "nl_inputs", "warren_identify_prestress.json")
    parsed = parse_problem(path)
    block = parsed["identify_prestress"]
    case = pr.warren_case(True, True)
    assert "identify_nr" not in parsed and set(block) == {"prestress_groups", "levels", "groups", "t0", "max_evaluations"}
    assert block["prestress_groups"] == case.pgroups.tolist() == block["groups"] and block["t0"] is None
    assert block["max_evaluations"] == 20 and len(block["levels"]) == 3
    assert np.array_equal(parsed["solver_config"].initial_strain, case.e0_base)
    assert np.array_equal(block["levels"][2]["u"], case.levels[2][2])
    cable = parse_problem(os.path.join(HERE, "nl_inputs", "cable_pretension.json"))["identify_prestress"]
    assert cable["t0"] == [-5e-3] and cable["groups"] is None and cable["prestress_scale"] == 1e-3 and cable["damping"] == 1e-3
    assert np.array_equal(cable["levels"][1]["u"], pr.cable_case().levels[1][2])
    with open(path) as f:
        data = json.load(f)
    good = data["accel"]["identify_prestress"]

    def refused(accel, match, **top):
        (tmp_path / "case.json").write_text(json.dumps(dict(data, accel=accel, **top)))
        with pytest.raises(ValueError, match=match):
            parse_problem(str(tmp_path / "case.json"))

    shape = r"identify_prestress must be \{\"prestress_groups\""
    for bad in (dict(good, extra=1), dict(good, method="gauss-newton"), {k: v for k, v in good.items() if k != "prestress_groups"},
                {k: v for k, v in good.items() if k != "levels"}, dict(good, prestress_groups=3),
                dict(good, levels=[dict(good["levels"][0], weight=1.0)])):
        refused(dict(data["accel"], identify_prestress=bad), shape)
    refused(dict(data["accel"], identify_nr={"groups": good["groups"], "levels": good["levels"]}), "both identify_nr and identify_prestress")
    refused(data["accel"], 'method "nr"', solver_config=dict(data["solver_config"], method="gd"))


def test_res_json_keys(monkeypatch):
    from pinn_fem_amd.cli import generic
    from pinn_fem_amd.fem import prestress
    seen = {}

    def fake(model, config, levels, prestress_groups, groups=None, t0=None, **kw):
        seen.update(kw, groups=groups, t0=t0, prestress_groups=prestress_groups)
        joint = groups is not None
        history = [{"misfit": 1.0, "gradient_norm": 2.0, "factors": np.ones(2) if joint else None, "prestress": np.zeros(1),
                    "accepted": True, "damping": 1e-3},
                   {"misfit": None, "gradient_norm": None, "factors": np.ones(2) if joint else None, "prestress": np.ones(1),
                    "accepted": False, "damping": 1e-3, "error": "slack"}]
        return prestress.PrestressResult(
            prestress=np.array([-1e-3]), initial_strain=np.full(3, -1e-3), factors=np.ones(2) if joint else None, ea=np.ones(3),
            misfit=1.0, evaluations=2, converged=False, stop="cap", history=history, displacements=[np.zeros(4)],
            strains=[np.zeros(3)], reactions=np.zeros(4), axial_forces=np.ones(3), counters={}, jacobian=np.ones((4, 3)),
            singular_values=np.ones(3), covariance=np.eye(3 if joint else 1), prestress_std=np.ones(1),
            factor_std=np.ones(2) if joint else None)
    monkeypatch.setattr(prestress, "identify_prestress", fake)
    keys = {"success", "converged", "iterations", "history", "identified_prestress", "prestress_std", "identified_initial_strain",
            "identified_ea", "misfit", "evaluations", "stop", "singular_values", "covariance", "displacements", "reactions",
            "strains", "axial_forces"}
    out = generic._identify_prestress_problem(None, None, {"prestress_groups": [0, 0, -1], "levels": [], "groups": None, "t0": [-5e-3],
                                                           "max_evaluations": 7, "prestress_scale": 1e-2})
    assert set(out) == keys and seen == {"max_evaluations": 7, "prestress_scale": 1e-2, "groups": None, "t0": [-5e-3],
                                         "prestress_groups": [0, 0, -1]}
    assert out["identified_prestress"] == [-1e-3] and out["axial_forces"] == [1.0, 1.0, 1.0] and out["stop"] == "cap"
    assert out["history"][1] == {"misfit": None, "gradient_norm": None, "factors": None, "prestress": [1.0], "accepted": False,
                                 "damping": 1e-3, "error": "slack"}
    assert "error" not in out["history"][0]
    out = generic._identify_prestress_problem(None, None, {"prestress_groups": [0, 0, -1], "levels": [], "groups": [0, 1, 1], "t0": None,
                                                           "damping": 0.5})
    assert set(out) == keys | {"identified_factors", "factor_std"} and seen["damping"] == 0.5 and seen["groups"] == [0, 1, 1]
    assert out["identified_factors"] == [1.0, 1.0] == out["factor_std"]
    json.dumps(out)


def test_abi_declares_pf_gl_prestress_rhs():
    from pinn_fem_amd import _capi
    header = open(os.path.join(os.path.dirname(HERE), "include", "pinnfem_hip.h")).read()
    assert _capi.PF_ABI_VERSION == 9 and re.search(r"#define PF_ABI_VERSION 9\b", header)
    assert _capi.PF_PCG_MAX_RHS == 2 and re.search(r"#define PF_PCG_MAX_RHS 2\b", header)
    decl = re.search(r"\bint pf_gl_prestress_rhs\(([^;]*)\);", header)
    assert decl
    params = [" ".join(a.split()) for a in decl.group(1).split(",")]
    assert params == ["const pf_problem* p", "const pf_gl* g", "const double* ea", "const double* u", "const int* elem_group",
                      "int g0", "int m", "double* out", "void* stream"]
    assert _capi.SYMBOLS["pf_gl_prestress_rhs"] == (C.c_int, [_capi._PP, _capi._PG, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                              C.c_int, C.c_void_p, C.c_void_p])
    assert [f[0] for f in _capi.PfGl._fields_] == ["d0", "kt", "fe", "strain"]           # no struct changed
    source = open(os.path.join(os.path.dirname(HERE), "pinn_fem_amd", "csrc", "pf_nl.hip")).read()
    assert "k_gl_prestress_rhs<2>" in source and "k_gl_prestress_rhs<1>" in source and "atomic" not in source.split(
        "void k_gl_prestress_rhs")[1].split("// out[dof] = sum over the node's incidences")[0]


def test_identify_scale_takes_the_parameters():
    tool = open(os.path.join(os.path.dirname(HERE), "tools", "identify_scale.py")).read()
    assert re.search(r'"--parameters",\s*choices=\("stiffness", "prestress", "both"\),\s*default="stiffness"', tool)
    assert re.search(r'"--method",\s*choices=\("lbfgs", "gauss-newton"\)', tool)          # as before
