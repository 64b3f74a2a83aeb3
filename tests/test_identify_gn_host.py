"""Gauss-Newton identification of E*A factors, host side: the restatement tests/identify_gn_reference.py against central
differences, against the adjoint gradient and against equilibrium, its Levenberg-Marquardt loop on four and eight span
groups and on noisy measurements, and the refusals, JSON, CLI and ABI surface of method "gauss-newton".  No GPU.

Every measured figure is printed in front of its assertion."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import gl_reference as gl
import identify_reference as ir
from device_driver import case_model

HERE = os.path.dirname(os.path.abspath(__file__))
U53 = 2.0 ** -53
POINTS = (np.zeros(4), np.array([0.1, -0.2, 0.05, 0.3]))


# ---- 1. the Jacobian ------------------------------------------------------------------------------------------------
def test_jacobian_against_central_differences():
    """A[:, g] against (rho(q + h e_g) - rho(q - h e_g)) / 2h, h = 1e-5, with states converged to 1e-12.  Bound 1e-8 of
    the largest entry, as test_identify_host.py bounds the adjoint gradient: the h^2 truncation term of the difference
    is h^2 = 1e-10 times rho''' / 6 rho' = O(10)."""
    case = ir.warren_case(8)
    h = 1e-5
    for q in POINTS:
        rho, A, _, _ = ir.case_residuals(case, q, tol=1e-12)
        fd = np.zeros_like(A)
        for g in range(4):
            e = np.zeros(4)
            e[g] = h
            fd[:, g] = (ir.case_residuals(case, q + e, jacobian=False, tol=1e-12)[0]
                        - ir.case_residuals(case, q - e, jacobian=False, tol=1e-12)[0]) / (2 * h)
        err = np.max(np.abs(A - fd)) / np.max(np.abs(A))
        print(f"q = {q}: A {A.shape}, max |A| = {np.max(np.abs(A)):.3e}, against differences {err:.2e}")
        assert A.shape == (3 * 30, 4) and rho.shape == (90,) and err <= 1e-8


def test_twice_a_transpose_rho_is_the_adjoint_gradient():
    """2 A^T rho against Case.objective's dJ/dq (one adjoint solve per level).  Both are sums over the levels of
    products with K_t,ff^-1, each solve exact to a few 2^-53 cond(K_t,ff); bound: 4 * 2^-53 * the largest condition
    number of the levels' tangents, computed here (two solves per path, a factor 2 each), relative to the largest
    component.  J itself: the same sum of squares in another order, 90 terms."""
    case = ir.warren_case(8)
    free = gl.free_mask(len(case.loads), case.fixed)
    for q in POINTS:
        rho, A, us, _ = ir.case_residuals(case, q)
        J, g = case.objective(q)
        cond = max(np.linalg.cond(gl.restrict(gl.k_t(case.nodes, case.el, u, case.ea(q), 2), free).toarray()) for u in us)
        err = np.max(np.abs(2.0 * A.T @ rho - g)) / np.max(np.abs(g))
        print(f"q = {q}: J - rho.rho = {J - rho @ rho:.2e}, 2 A^T rho against the adjoint {err:.2e} "
              f"(bound {4 * U53 * cond:.2e}, cond {cond:.3e})")
        assert abs(J - rho @ rho) <= 90 * U53 * J
        assert err <= 4 * U53 * cond


def test_group_right_hand_sides_sum_to_minus_the_load():
    """sum_g rhs_g = -f_int = -lam f on the free dofs of a converged state, within the Newton residual lam f - f_int(u)
    (recomputed here) plus the rounding of adding G group sums in another order: G * 2^-53 of the magnitude of f_int's
    terms (gl.f_int_scale).  On the fixed dofs every row is zero."""
    case = ir.warren_case(8)
    free = gl.free_mask(len(case.loads), case.fixed)
    q = POINTS[1]
    ea = case.ea(q)
    us = ir.case_residuals(case, q, jacobian=False)[2]
    for (lam, _, _), u in zip(case.levels, us):
        B = gl.group_rhs(case.nodes, case.el, u, ea, 2, case.groups, 4, case.fixed)
        residual = lam * case.loads - gl.f_int(case.nodes, case.el, u, ea, 2)
        gap = np.max(np.abs(B.sum(axis=0) + lam * case.loads - residual)[free])
        allowed = 4 * U53 * np.max(gl.f_int_scale(case.nodes, case.el, u, ea, 2))
        print(f"lam = {lam:.3f}: |sum_g rhs_g + lam f| = {np.max(np.abs(B.sum(axis=0) + lam * case.loads)[free]):.2e}, Newton "
              f"residual {np.max(np.abs(residual[free])):.2e}, apart by {gap:.2e} (allowed {allowed:.2e})")
        assert gap <= allowed and not B[:, ~free].any()
        assert np.max(np.abs(residual[free])) <= 1e-9 * abs(lam * case.loads[case.tip])


# ---- 2. the loop ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_groups", [4, 8])
def test_levenberg_marquardt_takes_five_evaluations(n_groups):
    """From all factors 1 with misfit_tolerance 1e-15: five evaluations, every step accepted, and the count does not
    hinge on round-off: the last misfit above 1e-15 is more than 150 times it and the first below more than 150 times
    under it."""
    case, run = ir.reference_run(n_groups)
    misfits = [h["misfit"] for h in run["history"]]
    err = np.max(np.abs(run["factors"] - case.factors))
    s = np.linalg.svd(run["jacobian"], compute_uv=False)
    print(f"{n_groups} groups: {run['evaluations']} evaluations, stop {run['stop']!r}, J per evaluation "
          f"{[f'{m:.1e}' for m in misfits]}, factor error {err:.2e}, sigma_min(A) {s[-1]:.2e}, cond(A) {s[0] / s[-1]:.0f}")
    assert run["evaluations"] == 5 == len(misfits) and run["stop"] == "misfit"
    assert all(h["accepted"] for h in run["history"])
    assert misfits[-2] > 150 * 1e-15 and misfits[-1] < 1e-15 / 150
    assert err <= 1e-6


def test_the_newton_tolerance_does_not_change_the_count():
    case = ir.case_with_groups(4)
    counts = [ir.identify_factors(case, misfit_tolerance=1e-15, tol=tol)["evaluations"] for tol in (1e-8, 1e-10)]
    print(f"evaluations with the Newton tolerance at 1e-8 and 1e-10: {counts}")
    assert counts == [5, 5]


def test_noisy_measurements_and_the_covariance():
    """Gaussian noise of 1e-4 on every measurement (seed 0): the loop stops on the gradient or the step; the estimated
    standard deviations of the log-factors are those of sigma^2 (A~^T A~)^-1 with the known sigma and the unweighted
    Jacobian A~ = sqrt|m| A to within three standard errors of a variance estimate, 3 / sqrt(2 (M - G)); and every
    log-factor lies within 4 estimated standard deviations of the truth."""
    case = ir.noisy_case()
    run = ir.identify_factors(case)
    A = run["jacobian"]
    M, G = A.shape
    std = np.sqrt(np.diag(ir.covariance(A, run["misfit"])))
    m = len(case.levels[0][1])
    known = ir.NOISE_SIGMA * np.sqrt(np.diag(np.linalg.inv((m * A).T @ A)))
    off = (run["q"] - np.log(case.factors)) / std
    print(f"noisy: {run['evaluations']} evaluations, stop {run['stop']!r}, J = {run['misfit']:.3e}, std of log-factors {std}, "
          f"std / known - 1 = {std / known - 1.0} (allowed {3 / np.sqrt(2 * (M - G)):.3f}), (q - q_true) / std = {off}")
    assert run["stop"] in ("gradient", "step")
    assert np.max(np.abs(std / known - 1.0)) <= 3.0 / np.sqrt(2.0 * (M - G))
    assert np.max(np.abs(off)) <= 4.0


# ---- 3. refusals ----------------------------------------------------------------------------------------------------
def _model(n_panels=8):
    case = ir.warren_case(n_panels)
    return case, case_model(case)


def test_every_refusal_is_a_value_error_before_an_engine_is_built(monkeypatch):
    from pinn_fem_amd.fem import identify, solver
    monkeypatch.setattr(solver, "_engine_for", lambda *a, **k: pytest.fail("an engine was built"))
    case, model = _model()
    cfg = solver.SolverConfig(kinematics="green-lagrange", max_iterations=50, tolerance=1e-10)

    def refused(match, levels=case.levels, groups=case.groups, **kw):
        kw.setdefault("method", "gauss-newton")
        with pytest.raises(ValueError, match=match):
            identify.identify_nr(model, cfg, levels, groups=groups, **kw)

    refused("unknown identification method", method="newton")
    refused("unknown identification method", method="Gauss-Newton")
    refused("needs an element -> group map", groups=None)
    refused(r"groups \[2\] have no element", groups=np.where(case.groups == 2, 4, case.groups))
    refused("4 groups for 3 measurement rows", levels=[(lam, dofs[:1], u[:1]) for lam, dofs, u in case.levels])
    for bad in (0.0, -1e-3, np.inf, np.nan):
        refused("damping must be positive and finite", damping=bad)
    refused("negative group ids", groups=np.where(np.arange(31) == 3, -1, case.groups))      # check_identify's still hold
    # what check_gauss_newton passes: G and M
    levels, groups, _ = identify.check_identify(model, cfg, case.levels, case.groups)
    assert identify.check_gauss_newton(levels, groups, 1e-3) == (4, 90)
    assert identify.check_gauss_newton([(lam, dofs[:2], u[:2]) for lam, dofs, u in levels][:2], groups, 1.0) == (4, 4)


# ---- 4. surface -----------------------------------------------------------------------------------------------------
def test_exports_and_the_result_fields():
    import inspect
    import pinn_fem_amd.fem as fem
    from pinn_fem_amd.fem import identify
    assert fem.residuals_and_jacobian is identify.residuals_and_jacobian and "residuals_and_jacobian" in fem.__all__
    fields = identify.IdentifyResult.__dataclass_fields__
    assert list(fields)[-5:] == ["jacobian", "singular_values", "covariance", "factor_std", "stop"]
    assert all(fields[name].default is None for name in list(fields)[-5:])
    sig = inspect.signature(identify.identify_nr).parameters
    assert (sig["method"].default, sig["damping"].default, sig["step_tolerance"].default) == ("lbfgs", 1e-3, 1e-12)
    assert list(sig)[:9] == ["model", "config", "levels", "groups", "q0", "max_evaluations", "gtol", "misfit_tolerance",
                             "history_size"]
    sig = inspect.signature(identify.residuals_and_jacobian).parameters
    assert list(sig) == ["model", "config", "levels", "ea", "groups", "states", "jacobian"]
    assert sig["states"].default is None and sig["jacobian"].default is True


def test_json_block(tmp_path):
    from pinn_fem_amd.cli.generic import parse_problem
    block = parse_problem(os.path.join(HERE, "nl_inputs", "warren_identify_gn.json"))["identify_nr"]
    lbfgs = parse_problem(os.path.join(HERE, "nl_inputs", "warren_identify.json"))["identify_nr"]
    assert set(lbfgs) == {"groups", "levels", "max_evaluations"} and lbfgs["max_evaluations"] == 78      # as before
    assert set(block) == set(lbfgs) | {"method", "damping"}
    assert block["method"] == "gauss-newton" and block["damping"] == 1e-3 and block["max_evaluations"] == 20
    assert block["groups"] == lbfgs["groups"] and block["levels"] == lbfgs["levels"]
    with open(os.path.join(HERE, "nl_inputs", "warren_identify_gn.json")) as f:
        data = json.load(f)
    good = data["accel"]["identify_nr"]
    for bad in (dict(good, extra=1), dict(good, step_tolerance=1e-12)):
        (tmp_path / "case.json").write_text(json.dumps(dict(data, accel=dict(data["accel"], identify_nr=bad))))
        with pytest.raises(ValueError, match="identify_nr"):
            parse_problem(str(tmp_path / "case.json"))


def test_res_json_keys(monkeypatch):
    """_identify_problem passes method and damping on; the L-BFGS output keeps its keys exactly, gauss-newton adds four."""
    from pinn_fem_amd.cli import generic
    from pinn_fem_amd.fem import identify
    seen = {}

    def fake(model, config, levels, groups=None, **kw):
        seen.update(kw)
        gauss = kw.get("method") == "gauss-newton"
        history = [{"misfit": 1.0, "gradient_norm": 2.0, "factors": np.ones(2)}]
        extra = {}
        if gauss:
            history = [dict(history[0], accepted=True, damping=1e-3),
                       {"misfit": 2.0, "gradient_norm": None, "factors": np.ones(2), "accepted": False, "damping": 1e-3}]
            extra = dict(jacobian=np.ones((3, 2)), singular_values=np.array([2.0, 1.0]), covariance=np.eye(2),
                         factor_std=np.ones(2), stop="cap")
        return identify.IdentifyResult(factors=np.ones(2), ea=np.ones(3), misfit=1.0, gradient=np.zeros(2), evaluations=1,
                                       converged=False, history=history, displacements=[np.zeros(4)], counters={},
                                       reactions=np.zeros(4), **extra)
    monkeypatch.setattr(identify, "identify_nr", fake)
    old_keys = {"success", "converged", "iterations", "history", "identified_factors", "identified_ea", "misfit",
                "evaluations", "displacements", "reactions"}
    out = generic._identify_problem(None, None, {"groups": [0, 0, 1], "levels": [], "max_evaluations": 7})
    assert set(out) == old_keys and seen == {"max_evaluations": 7}
    assert set(out["history"][0]) == {"misfit", "gradient_norm", "factors"}
    out = generic._identify_problem(None, None, {"groups": [0, 0, 1], "levels": [], "method": "gauss-newton", "damping": 0.5})
    assert seen == {"max_evaluations": 7, "method": "gauss-newton", "damping": 0.5}
    assert set(out) == old_keys | {"factor_std", "singular_values", "covariance", "stop"}
    assert out["stop"] == "cap" and out["covariance"] == [[1.0, 0.0], [0.0, 1.0]] and out["factor_std"] == [1.0, 1.0]
    assert out["history"][1] == {"misfit": 2.0, "gradient_norm": None, "factors": [1.0, 1.0], "accepted": False, "damping": 1e-3}
    json.dumps(out)


def test_abi_declares_pf_gl_group_rhs():
    from pinn_fem_amd import _capi
    header = open(os.path.join(os.path.dirname(HERE), "include", "pinnfem_hip.h")).read()
    assert _capi.PF_ABI_VERSION == 9 and re.search(r"#define PF_ABI_VERSION 9\b", header)
    assert _capi.PF_PCG_MAX_RHS == 2 and re.search(r"#define PF_PCG_MAX_RHS 2\b", header)
    decl = re.search(r"\bint pf_gl_group_rhs\(([^;]*)\);", header)
    assert decl
    params = [" ".join(a.split()) for a in decl.group(1).split(",")]
    assert params == ["const pf_problem* p", "const pf_gl* g", "const int* elem_group", "int g0", "int m", "double* out",
                      "void* stream"]
    assert _capi.SYMBOLS["pf_gl_group_rhs"] == (C.c_int, [_capi._PP, _capi._PG, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                                          C.c_void_p])
    assert [f[0] for f in _capi.PfGl._fields_] == ["d0", "kt", "fe", "strain"]           # no struct changed


def test_identify_scale_takes_a_method():
    tool = open(os.path.join(os.path.dirname(HERE), "tools", "identify_scale.py")).read()
    assert re.search(r'"--method",\s*choices=\("lbfgs", "gauss-newton"\)', tool)
