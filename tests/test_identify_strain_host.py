"""Identification from strain-gauge data, host side: the restatement tests/identify_strain_reference.py against central
differences, the adjoint identity, the adjoint gradient and the two-bar closed form, its Levenberg-Marquardt loop on four
and eight span groups with and without the tip dof, and the refusals, JSON, CLI and ABI surface of the strain keys.  No GPU.

Every measured figure is printed in front of its assertion."""
import ctypes as C
import inspect
import json
import os
import re

import numpy as np
import pytest

import gl_reference as gl
import identify_reference as ir
import identify_strain_reference as sr
from device_driver import case_model

HERE = os.path.dirname(os.path.abspath(__file__))
U53 = 2.0 ** -53
POINTS = (np.zeros(4), np.array([0.1, -0.2, 0.05, 0.3]))


# ---- 1. B = d e / d u ------------------------------------------------------------------------------------------------
def _dyadic_fields(case, rng):
    """u and v on the 2^-20 grid (the Warren nodes lie on the 1/2 grid): u +- 2^-8 v and every u_j - u_i are exact."""
    n = len(case.loads)
    return (np.round(0.3 * rng.standard_normal(n) * 2 ** 20) / 2 ** 20, np.round(rng.standard_normal(n) * 2 ** 12) / 2 ** 12)


def _e_abs(case, u):
    t = gl.element_state(case.nodes, case.el, u, 1.0, 2)[3]
    return (2.0 * np.sum(np.abs(t["d0"]) * np.abs(t["du"]), axis=1) + np.sum(t["du"] ** 2, axis=1)) / (2.0 * t["l02"])


def test_b_v_is_the_central_difference_of_the_strain():
    """e is quadratic in u, so (e(u + h v) - e(u - h v)) / 2h = B(u) v exactly; with a dyadic step h = 2^-8 on dyadic
    fields the only errors are the roundings of the two strains, 4 * 2^-53 e_abs each (half of the 8 e_abs that
    test_identify_f64.py allows device and reference together), over 2h, and those of B v itself: d is exact here, v_j - v_i
    is exact, so per gauge the products 1, their sum 1, l0^2 2 and the division 1: 5 * 2^-53 of gl.b_v_scale."""
    case = sr.strain_case(4)
    rng = np.random.default_rng(5)
    u, v = _dyadic_fields(case, rng)
    h = 2.0 ** -8
    elements = np.arange(len(case.el))
    fd = (gl.strains(case.nodes, case.el, u + h * v, 2) - gl.strains(case.nodes, case.el, u - h * v, 2)) / (2 * h)
    got = gl.b_v(case.nodes, case.el, u, elements, v, 2)
    bound = (4 * U53 * (_e_abs(case, u + h * v) + _e_abs(case, u - h * v)) / (2 * h)
             + 5 * U53 * gl.b_v_scale(case.nodes, case.el, u, elements, v, 2))
    err = np.abs(got - fd)
    print(f"B v against the central difference: worst error / bound {np.max(err / bound):.3f}, relative "
          f"{np.max(err) / np.max(np.abs(got)):.2e}")
    assert np.all(err <= bound) and np.max(np.abs(got)) > 0.1


def test_b_and_its_transpose_are_adjoint():
    """<c, B v> = <B^T c, v>: the same 2 * ne * dim products (c_e / l0^2) d_c v_c summed in two orders.  Each product
    carries at most 8 roundings on either side (d 2, l0^2 2, the division 1, the products 2, v_j - v_i 1) and each sum fewer
    than ne * dim + n_dofs additions: (16 + 2 (ne dim + n_dofs)) 2^-53 of sum_e |c_e| b_v_scale_e."""
    case = sr.strain_case(4)
    rng = np.random.default_rng(6)
    n, ne = len(case.loads), len(case.el)
    u, v, c = 0.3 * rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(ne)
    elements = np.arange(ne)
    lhs = float(c @ gl.b_v(case.nodes, case.el, u, elements, v, 2))
    rhs = float(gl.bt_c(case.nodes, case.el, u, c, 2) @ v)
    bound = (16 + 2 * (2 * ne + n)) * U53 * float(np.abs(c) @ gl.b_v_scale(case.nodes, case.el, u, elements, v, 2))
    print(f"<c, B v> = {lhs:.15e}, <B^T c, v> = {rhs:.15e}, apart by {abs(lhs - rhs):.2e} (bound {bound:.2e})")
    assert abs(lhs - rhs) <= bound and abs(lhs) > 1e-3
    # a coefficient vector that is zero but on two elements moves the dofs of their four nodes only
    c0 = np.zeros(ne)
    c0[[3, 20]] = 1.0
    out = gl.bt_c(case.nodes, case.el, u, c0, 2).reshape(-1, 2)
    touched = np.unique(case.el[[3, 20]])
    assert np.all(out[np.setdiff1d(np.arange(len(out)), touched)] == 0.0) and np.all(out[touched] != 0.0)


# ---- 2. the Jacobian and the gradient --------------------------------------------------------------------------------
@pytest.mark.parametrize("tip", [False, True])
def test_jacobian_and_gradient_against_central_differences(tip):
    """A[:, g] against (rho(q + h e_g) - rho(q - h e_g)) / 2h and the adjoint dJ/dq against (J(q + h e_g) - J(q - h e_g)) /
    2h, h = 1e-5, states converged to 1e-12.  Bound 1e-8 of the largest entry, as test_identify_gn_host.py allows the
    displacement Jacobian: the h^2 truncation term is h^2 = 1e-10 times rho''' / 6 rho' = O(10)."""
    case = sr.strain_case(4, tip=tip)
    h = 1e-5
    for q in POINTS:
        rho, A, _, _ = ir.case_residuals(case, q, tol=1e-12)
        _, g = case.objective(q, tol=1e-12)
        fd_A, fd_g = np.zeros_like(A), np.zeros(4)
        for k in range(4):
            e = np.zeros(4)
            e[k] = h
            rp = ir.case_residuals(case, q + e, jacobian=False, tol=1e-12)[0]
            rm = ir.case_residuals(case, q - e, jacobian=False, tol=1e-12)[0]
            fd_A[:, k] = (rp - rm) / (2 * h)
            fd_g[k] = (case.objective(q + e, tol=1e-12)[0] - case.objective(q - e, tol=1e-12)[0]) / (2 * h)
        err_A = np.max(np.abs(A - fd_A)) / np.max(np.abs(A))
        err_g = np.max(np.abs(g - fd_g)) / np.max(np.abs(g))
        print(f"tip {tip}, q = {q}: A {A.shape}, max |A| = {np.max(np.abs(A)):.3e}, against differences {err_A:.2e}; "
              f"dJ/dq against differences {err_g:.2e}")
        assert A.shape == (case.n_rows, 4) and rho.shape == (case.n_rows,) and case.n_rows == (15 if tip else 12)
        assert err_A <= 1e-8 and err_g <= 1e-8


@pytest.mark.parametrize("tip", [False, True])
def test_twice_a_transpose_rho_is_the_adjoint_gradient(tip):
    """test_identify_gn_host.py's bound: 4 * 2^-53 * the largest condition number of the levels' tangents, relative to the
    largest component; J is the same sum of squares in another order."""
    case = sr.strain_case(4, tip=tip)
    free = gl.free_mask(len(case.loads), case.fixed)
    for q in POINTS:
        rho, A, us, _ = ir.case_residuals(case, q)
        J, g = case.objective(q)
        cond = max(np.linalg.cond(gl.restrict(gl.k_t(case.nodes, case.el, u, case.ea(q), 2), free).toarray()) for u in us)
        err = np.max(np.abs(2.0 * A.T @ rho - g)) / np.max(np.abs(g))
        print(f"tip {tip}, q = {q}: J - rho.rho = {J - rho @ rho:.2e}, 2 A^T rho against the adjoint {err:.2e} "
              f"(bound {4 * U53 * cond:.2e}, cond {cond:.3e})")
        assert abs(J - rho @ rho) <= case.n_rows * U53 * J
        assert err <= 4 * U53 * cond


# ---- 3. the loop -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tip", [False, True])
def test_levenberg_marquardt_takes_five_evaluations(tip):
    """From all factors 1 with misfit_tolerance 1e-15, on strains only and with the tip dof added: the same count, five, on
    four and on eight groups, every step accepted, the factors to 1e-9."""
    counts = []
    for n_groups in (4, 8):
        case, run = sr.reference_run(n_groups, tip)
        misfits = [h["misfit"] for h in run["history"]]
        err = np.max(np.abs(run["factors"] - case.factors))
        s = np.linalg.svd(run["jacobian"], compute_uv=False)
        print(f"{n_groups} groups, tip {tip}: {run['evaluations']} evaluations, stop {run['stop']!r}, J per evaluation "
              f"{[f'{m:.1e}' for m in misfits]}, factor error {err:.2e}, sigma_min(A) {s[-1]:.2e}, largest strain "
              f"{max(np.max(np.abs(g[1])) for g in case.gauges):.3f}")
        assert run["stop"] == "misfit" and all(h["accepted"] for h in run["history"])
        assert err <= 1e-9
        counts.append(run["evaluations"])
    assert counts == [5, 5]


# ---- 4. the two-bar truss --------------------------------------------------------------------------------------------
def test_two_bar_closed_form():
    """dJ/d(ea) of J = L^2 (e(w) - e_bar)^2 with a gauge on both bars at half the limit load, against
    2 L^2 (e - e_bar) de/dw dw/d(ea), dw/d(ea) = -P / (ea tangent(w)); bound: sr.two_bar_bound (the Newton tolerance)."""
    tb = gl.TwoBar(ea=1000.0)
    p, tol, scale = 0.5 * tb.p_lim, 1e-10, tb.l0
    w_ref = -gl.newton(tb.nodes, tb.el, tb.loads(p), tb.fixed, tb.ea, 2, tol=tol)[0][5]
    e_bar = 0.9 * tb.strain(w_ref)
    levels, gauges = [(1.0, [], [])], [([0, 1], [e_bar, e_bar], scale)]
    J, g, us, _ = ir.misfit_and_gradient(tb.nodes, tb.el, tb.loads(p), tb.fixed, np.full(2, tb.ea), 2, levels, gauges, tol=tol)
    w = -us[0][5]
    want = sr.two_bar_closed_form(tb, p, w, e_bar, scale)
    rel, bound = abs(g.sum() - want) / abs(want), sr.two_bar_bound(tb, w, e_bar, tol)
    print(f"two-bar: w = {w:.12f}, e(w) = {tb.strain(w):.6e}, dJ/d(ea) = {g.sum():.12e} (closed form {want:.12e}), relative "
          f"{rel:.2e}, bound {bound:.2e}")
    assert abs(J - scale ** 2 * (tb.strain(w) - e_bar) ** 2) <= 1e-12 * J and abs(g[0] - g[1]) <= 1e-12 * abs(g[0])
    assert rel <= bound


# ---- 5. refusals -----------------------------------------------------------------------------------------------------
def test_every_refusal_of_check_strains(monkeypatch):
    from pinn_fem_amd.fem import identify, solver
    monkeypatch.setattr(solver, "_engine_for", lambda *a, **k: pytest.fail("an engine was built"))
    case = sr.strain_case(4, tip=True)
    model = case_model(case)
    cfg = solver.SolverConfig(kinematics="green-lagrange", max_iterations=50, tolerance=1e-10)
    good = case.dict_levels()

    def refused(match, **change):
        levels = [dict(lv) for lv in good]
        for key, val in change.items():
            if val is None:
                del levels[1][key]
            else:
                levels[1][key] = val
        with pytest.raises(ValueError, match=match):
            identify.check_strains(model, levels)
        for method in ("lbfgs", "gauss-newton"):                   # and through identify_nr, before an engine is built
            with pytest.raises(ValueError, match=match):
                identify.identify_nr(model, cfg, levels, groups=case.groups, method=method)

    refused("one is given without the other", strains=None)
    refused("one is given without the other", strain_elements=None)
    refused("mismatched lengths: 3 strain elements, 4 strains", strain_elements=[0, 7, 15])
    refused("strain elements must be integers", strain_elements=[0.0, 7.0, 15.0, 23.0])
    refused("strain elements out of range 0..30", strain_elements=[0, 7, 15, 31])
    refused("strain elements out of range 0..30", strain_elements=[-1, 7, 15, 23])
    refused("listed twice", strain_elements=[0, 7, 7, 23])
    for bad in (np.nan, np.inf):
        refused("strains are not all finite", strains=[0.0, bad, 0.0, 0.0])
    refused("no Green-Lagrange strain", strains=[0.0, -0.5, 0.0, 0.0])
    refused("no Green-Lagrange strain", strains=[0.0, -0.7, 0.0, 0.0])
    for bad in (0.0, -8.0, np.inf, np.nan):
        refused("strain_scale must be positive and finite", strain_scale=bad)
    # strain keys on a tuple level: only the dict form carries strains
    lv = good[1]
    with pytest.raises(ValueError, match="only the dict form carries strains"):
        identify.check_strains(model, [good[0], (lv["load_factor"], lv["dofs"], lv["u"], lv["strain_elements"], lv["strains"])])
    # a level with neither kind of data is the empty level it was; four groups need four rows
    with pytest.raises(ValueError, match=r"level 0: no measured dofs \(an empty level\)"):
        identify.identify_nr(model, cfg, [{"load_factor": 1.0, "dofs": [], "u": []}], groups=case.groups)
    one = dict(good[0], dofs=[], u=[], strain_elements=[0, 7, 15], strains=[0.0, 0.0, 0.0])
    with pytest.raises(ValueError, match="4 groups for 3 measurement rows"):
        identify.identify_nr(model, cfg, [one], groups=case.groups, method="gauss-newton")


def test_check_strains_and_check_identify_on_good_levels():
    from pinn_fem_amd.fem import identify, solver
    case = sr.strain_case(4, tip=True)
    model = case_model(case)
    cfg = solver.SolverConfig(kinematics="green-lagrange")
    good = case.dict_levels()
    mixed = [good[2], (good[0]["load_factor"], [33], [-0.4]), good[1]]           # unsorted, one tuple level without strains
    out = identify.check_strains(model, mixed)
    assert out[0] is None and [o[2] for o in out[1:]] == [8.0, 8.0]
    assert out[1][0].dtype == np.int64 and out[1][1].dtype == np.float64
    assert np.array_equal(out[1][1], good[1]["strains"]) and np.array_equal(out[2][1], good[2]["strains"])
    assert identify.check_strains(model, [{k: v for k, v in good[0].items() if k != "strain_scale"}])[0][2] == 1.0
    levels, groups, q0 = identify.check_identify(model, cfg, mixed, case.groups)
    assert [lv[0] for lv in levels] == sorted(lv[0] for lv in levels) and all(len(lv) == 3 for lv in levels)
    # strains only: empty dofs pass check_identify on a level that carries strains
    only = [dict(lv, dofs=[], u=[]) for lv in good]
    levels, _, _ = identify.check_identify(model, cfg, only, case.groups)
    assert all(len(lv) == 3 and lv[1].size == 0 and lv[1].dtype == np.int64 for lv in levels)
    # a level without strains is checked as before: the same tuples from the dict and the tuple form, the old messages
    base = ir.warren_case(8)
    a = identify.check_identify(model, cfg, base.levels, base.groups)[0]
    b = identify.check_identify(model, cfg, [{"load_factor": l, "dofs": d, "u": u} for l, d, u in base.levels], base.groups)[0]
    for (la, da, ua), (lb, db, ub), (l0, d0, u0) in zip(a, b, base.levels):
        assert la == lb == l0 and np.array_equal(da, db) and np.array_equal(da, d0) and np.array_equal(ua, ub)
        assert np.array_equal(ua, u0)
    assert identify.check_strains(model, base.levels) == [None, None, None]
    with pytest.raises(ValueError, match="measured dofs must be integers"):
        identify.check_identify(model, cfg, [(1.0, [4.0], [0.1])])
    with pytest.raises(ValueError, match=r"measured dofs \[0\] are fixed dofs"):
        identify.check_identify(model, cfg, [dict(good[0], dofs=[0], u=[0.0])])
    assert identify.check_gauss_newton(levels, case.groups, 1e-3, identify.check_strains(model, only)) == (4, 12)
    assert identify.check_gauss_newton(a, base.groups, 1e-3) == (4, 90)


# ---- 6. surface ------------------------------------------------------------------------------------------------------
def test_exports_signatures_and_the_result_fields():
    import pinn_fem_amd.fem as fem
    from pinn_fem_amd.fem import identify
    assert fem.check_strains is identify.check_strains and "check_strains" in fem.__all__
    fields = list(identify.IdentifyResult.__dataclass_fields__)
    assert fields[fields.index("reactions") + 1] == "strains" and identify.IdentifyResult.__dataclass_fields__["strains"].default is None
    assert fields[-5:] == ["jacobian", "singular_values", "covariance", "factor_std", "stop"]
    assert list(inspect.signature(identify.check_strains).parameters) == ["model", "levels"]
    assert list(inspect.signature(identify.identify_nr).parameters) == [
        "model", "config", "levels", "groups", "q0", "max_evaluations", "gtol", "misfit_tolerance", "history_size",
        "tolerance_change", "method", "damping", "step_tolerance"]
    assert list(inspect.signature(identify.residuals_and_jacobian).parameters) == [
        "model", "config", "levels", "ea", "groups", "states", "jacobian"]
    assert list(inspect.signature(identify.misfit_and_gradient).parameters) == ["model", "config", "levels", "ea"]
    sig = inspect.signature(identify.check_gauss_newton).parameters
    assert list(sig) == ["levels", "groups", "damping", "strains"] and sig["strains"].default is None
    for doc in (identify.identify_nr.__doc__, identify.check_strains.__doc__):
        assert "eps + eps^2 / 2" in doc                                # the engineering-strain conversion is stated


def test_json_block(tmp_path):
    from pinn_fem_amd.cli.generic import parse_problem
    path = os.path.join(HERE, "nl_inputs", "warren_identify_strain.json")
    block = parse_problem(path)["identify_nr"]
    gn_block = parse_problem(os.path.join(HERE, "nl_inputs", "warren_identify_gn.json"))["identify_nr"]
    assert set(block) == set(gn_block) and block["groups"] == gn_block["groups"] and max(block["groups"]) == 3
    assert (block["method"], block["damping"], block["max_evaluations"]) == ("gauss-newton", 1e-3, 20)
    case = sr.strain_case(4, tip=True)                       # the measurements are the restatement's
    assert len(block["levels"]) == 3
    for lv, want in zip(block["levels"], case.dict_levels()):
        assert set(lv) == {"load_factor", "dofs", "u", "strain_elements", "strains", "strain_scale"}
        assert lv["load_factor"] == want["load_factor"] and lv["dofs"] == [case.tip] and lv["strain_scale"] == 8.0
        assert lv["strain_elements"] == want["strain_elements"].tolist() and len(lv["strain_elements"]) == 4
        assert np.allclose(lv["strains"], want["strains"], rtol=1e-13, atol=0.0) and np.allclose(lv["u"], want["u"], rtol=1e-13)
    with open(path) as f:
        data = json.load(f)
    with open(os.path.join(HERE, "nl_inputs", "warren_identify_gn.json")) as f:
        gn_data = json.load(f)
    assert {k: v for k, v in data.items() if k != "accel"} == {k: v for k, v in gn_data.items() if k != "accel"}
    good = data["accel"]["identify_nr"]

    def parse(levels):
        bad = dict(good, levels=levels)
        (tmp_path / "case.json").write_text(json.dumps(dict(data, accel=dict(data["accel"], identify_nr=bad))))
        return parse_problem(str(tmp_path / "case.json"))["identify_nr"]

    lv = good["levels"][0]
    drop = lambda *keys: {k: v for k, v in lv.items() if k not in keys}
    assert set(parse([drop("strain_scale")])["levels"][0]) == set(lv) - {"strain_scale"}
    assert set(parse([drop("strain_scale", "strains", "strain_elements")])["levels"][0]) == {"load_factor", "dofs", "u"}
    for bad in (drop("strains"), drop("strain_elements"), drop("strains", "strain_elements"), dict(lv, gauge_factor=2.0),
                drop("dofs")):
        with pytest.raises(ValueError, match="strain_elements.*strains.*strain_scale"):
            parse([bad])


def test_res_json_keys(monkeypatch):
    """The .res.json gains "strains" (the last level's) only when the result has them; the old key sets are as they were."""
    from pinn_fem_amd.cli import generic
    from pinn_fem_amd.fem import identify

    def fake(with_strains, gauss):
        def run(model, config, levels, groups=None, **kw):
            extra = dict(jacobian=np.ones((3, 2)), singular_values=np.array([2.0, 1.0]), covariance=np.eye(2),
                         factor_std=np.ones(2), stop="cap") if gauss else {}
            history = [{"misfit": 1.0, "gradient_norm": 2.0, "factors": np.ones(2)}]
            return identify.IdentifyResult(factors=np.ones(2), ea=np.ones(3), misfit=1.0, gradient=np.zeros(2), evaluations=1,
                                           converged=False, history=history, displacements=[np.zeros(4)], counters={},
                                           reactions=np.zeros(4),
                                           strains=[np.zeros(3), np.array([0.1, 0.2, 0.3])] if with_strains else None, **extra)
        return run
    old_keys = {"success", "converged", "iterations", "history", "identified_factors", "identified_ea", "misfit",
                "evaluations", "displacements", "reactions"}
    gn_keys = {"factor_std", "singular_values", "covariance", "stop"}
    block = {"groups": [0, 0, 1], "levels": []}
    for with_strains in (False, True):
        for gauss in (False, True):
            monkeypatch.setattr(identify, "identify_nr", fake(with_strains, gauss))
            out = generic._identify_problem(None, None, block)
            assert set(out) == old_keys | (gn_keys if gauss else set()) | ({"strains"} if with_strains else set())
            if with_strains:
                assert out["strains"] == [0.1, 0.2, 0.3] and list(out)[-1] == "strains"
            json.dumps(out)


def test_abi_declares_the_two_strain_entry_points():
    from pinn_fem_amd import _capi
    header = open(os.path.join(os.path.dirname(HERE), "include", "pinnfem_hip.h")).read()
    assert _capi.PF_ABI_VERSION == 9 and re.search(r"#define PF_ABI_VERSION 9\b", header)
    assert _capi.PF_PCG_MAX_RHS == 2 and re.search(r"#define PF_PCG_MAX_RHS 2\b", header)
    want = {
        "pf_gl_strain_rhs": (["const pf_problem* p", "const pf_gl* g", "const double* u", "const double* coef", "int accumulate",
                              "double* out", "void* stream"],
                             [_capi._PP, _capi._PG, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
        "pf_gl_strain_jvp": (["const pf_problem* p", "const pf_gl* g", "const double* u", "const int* elems", "int n_meas",
                              "const double* v", "int m", "double* out", "void* stream"],
                             [_capi._PP, _capi._PG, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                              C.c_void_p]),
    }
    for name, (params, argtypes) in want.items():
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert decl, name
        assert [" ".join(a.split()) for a in decl.group(1).split(",")] == params, name
        assert _capi.SYMBOLS[name] == (C.c_int, argtypes), name
    assert [f[0] for f in _capi.PfGl._fields_] == ["d0", "kt", "fe", "strain"]           # no struct changed


def test_identify_scale_takes_the_kind_of_data():
    tool = open(os.path.join(os.path.dirname(HERE), "tools", "identify_scale.py")).read()
    assert re.search(r'"--data",\s*choices=\("displacements", "strains"\),\s*default="displacements"', tool)
