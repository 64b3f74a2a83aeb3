"""Identification through the Green-Lagrange Newton solve, host side: the restatement tests/identify_reference.py against
central differences and the two-bar closed form, its L-BFGS recovery of four span-group factors, and the refusals, JSON
and ABI surface of pinn_fem_amd.fem.identify.  No GPU."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import gl_reference as gl
import identify_reference as ir

HERE = os.path.dirname(os.path.abspath(__file__))
EA = 1000.0


# ---- 1. the adjoint gradient against central differences ------------------------------------------------------------
@pytest.mark.parametrize("n_panels", [8, 16])
def test_adjoint_gradient_against_central_differences(n_panels):
    """dJ/dq by the adjoint against (J(q + h) - J(q - h)) / 2h, h = 1e-5, at all factors 1 (where the optimisation
    starts) and at a point off it.  Bound 1e-8 of the largest component: the h^2 truncation term of the difference is of
    that size (h^2 = 1e-10 times J'''/6 J' = O(10)), and it is a 40-fold margin over the 2.6e-10 measured."""
    case = ir.warren_case(n_panels)
    u_tip = -case.levels[-1][2][list(case.levels[-1][1]).index(case.tip)] / n_panels
    assert 0.155 < u_tip < 0.165                                  # a tip deflection of 0.16 of the span
    h = 1e-5
    for q in (np.zeros(4), np.array([0.1, -0.2, 0.05, 0.3])):
        J, g = case.objective(q)
        fd = np.zeros(4)
        for k in range(4):
            e = np.zeros(4)
            e[k] = h
            fd[k] = (case.objective(q + e)[0] - case.objective(q - e)[0]) / (2 * h)
        err = np.max(np.abs(g - fd)) / np.max(np.abs(g))
        print(f"{n_panels} panels, q = {q}: J = {J:.6e}, dJ/dq = {g}, adjoint against differences {err:.2e}")
        assert J > 1e-4 and err <= 1e-8


def test_group_reduce_and_span_groups():
    case = ir.warren_case(8)
    assert np.bincount(case.groups).tolist() == [7, 8, 8, 8]
    v, w = np.arange(31.0), np.linspace(1.0, 2.0, 31)
    got = ir.group_reduce(v, w, case.groups, 4)
    assert np.allclose(got, [np.sum((v * w)[case.groups == g]) for g in range(4)], rtol=1e-15)
    assert np.array_equal(ir.group_reduce(v, None, np.zeros(31, dtype=int), 2), [v.sum(), 0.0])


# ---- 2. the two-bar closed form -------------------------------------------------------------------------------------
@pytest.mark.parametrize("fraction", [0.5, 0.9])
def test_two_bar_closed_form(fraction):
    tb = gl.TwoBar(ea=EA)
    p, tol = fraction * tb.p_lim, 1e-10
    u, _, ok = gl.newton(tb.nodes, tb.el, tb.loads(p), tb.fixed, EA, 2, tol=tol)
    w = -u[5]
    w_bar = 0.9 * w
    J, g, _, _ = ir.misfit_and_gradient(tb.nodes, tb.el, tb.loads(p), tb.fixed, np.full(2, EA), 2,
                                        [(1.0, [5], [-w_bar])], tol=tol)
    want = ir.two_bar_closed_form(tb, p, w, w_bar)
    rel, bound = abs(g.sum() - want) / abs(want), ir.two_bar_bound(tb, w, w_bar, tol)
    print(f"two-bar {fraction} P_lim: w = {w:.12f}, dJ/d(ea) = {g.sum():.12e} (closed form {want:.12e}), "
          f"relative {rel:.2e}, bound {bound:.2e}")
    assert ok and 0.0 < w < tb.w_lim and abs(J - (w - w_bar) ** 2) <= 1e-14 * J
    assert g[0] == pytest.approx(g[1], rel=1e-12)                   # symmetry: each bar carries half
    assert rel <= bound


# ---- 3. recovery ----------------------------------------------------------------------------------------------------
def test_lbfgs_recovers_four_span_group_factors():
    case, factors, evaluations = ir.reference_recovery(8)
    err = np.max(np.abs(factors - case.factors))
    print(f"8 panels: factors {factors}, error {err:.2e}, {evaluations} misfit evaluations")
    assert err <= 1e-6
    assert 10 <= evaluations <= 75                                  # LBFGS's own cap is max_iter * 5 / 4 = 75


# ---- 4. check_identify ----------------------------------------------------------------------------------------------
def _model(young=2000.0, n_panels=8):
    from pinn_fem_amd.fem.model import FEMModel, Material
    case = ir.warren_case(n_panels)
    return case, FEMModel(nodes=case.nodes, elements=case.el, material=Material(young, 0.5, 1.0), loads=case.loads,
                          fixed_dofs=case.fixed, dimension=2)


def test_every_refusal_is_a_value_error_before_an_engine_is_built(monkeypatch):
    from pinn_fem_amd.fem import identify, solver
    from pinn_fem_amd.fem.properties import NNProperty
    from pinn_fem_amd.nets import SimpleNN
    monkeypatch.setattr(solver, "_engine_for", lambda *a, **k: pytest.fail("an engine was built"))
    case, model = _model()
    levels = [{"load_factor": lam, "dofs": dofs, "u": u} for lam, dofs, u in case.levels]

    def cfg(**kw):
        base = dict(kinematics="green-lagrange", max_iterations=50, tolerance=1e-10)
        base.update(kw)
        return solver.SolverConfig(**base)

    def refused(match, m=model, c=None, lv=levels, groups=case.groups, q0=None):
        c = c or cfg()
        with pytest.raises(ValueError, match=match):
            identify.check_identify(m, c, lv, groups, q0)
        with pytest.raises(ValueError, match=match):
            identify.identify_nr(m, c, lv, groups=groups, q0=q0)

    def level(**kw):
        return [dict(levels[0], **kw)] + levels[1:]

    refused("linear operator has no per-element", c=cfg(kinematics="linear"))
    with pytest.raises(ValueError, match="linear operator has no per-element"):
        identify.misfit_and_gradient(model, cfg(kinematics="linear"), levels, np.full(31, EA))
    nn = NNProperty(net=SimpleNN(hidden_layers=1, neurons_per_layer=4, input_dim=3), input_dim=3,
                    enforce_positive=True, scale=2000.0)
    refused("scalar materials", m=_model(young=nn)[1])
    with monkeypatch.context() as mp:
        mp.setattr(solver, "_world_size", lambda: 2)
        refused("sharded")
    refused("load control only", c=cfg(nr_control="displacement", nr_control_dof=5, nr_control_displacement=-0.5))
    refused("levels is empty", lv=[])
    refused("empty level", lv=level(dofs=[], u=[]))
    refused("out of range", lv=level(dofs=[4, 34], u=[0.0, 0.0]))
    refused("out of range", lv=level(dofs=[-1], u=[0.0]))
    refused("fixed dofs", lv=level(dofs=[1, 4], u=[0.0, 0.0]))
    refused("mismatched lengths", lv=level(dofs=[4, 5], u=[0.0]))
    refused("wrong length", groups=case.groups[:-1])
    refused("negative group ids", groups=np.where(np.arange(31) == 3, -1, case.groups))
    refused("non-finite", q0=[0.0, np.nan, 0.0, 0.0])
    refused("non-finite", q0=[0.0, np.inf, 0.0, 0.0])
    refused("q0 has 3 entries", q0=[0.0, 0.0, 0.0])
    with pytest.raises(ValueError, match="31 elements"):
        identify.misfit_and_gradient(model, cfg(), levels, np.full(30, EA))
    with pytest.raises(ValueError, match="finite and positive"):
        identify.misfit_and_gradient(model, cfg(), levels, np.where(np.arange(31) == 3, 0.0, EA))
    # what passes: levels come back in ascending order of load factor, the defaults are one log-factor 0 per group
    lv, g, q = identify.check_identify(model, cfg(), levels[::-1], case.groups)
    assert [x[0] for x in lv] == sorted(x["load_factor"] for x in levels) and g.dtype == np.int64 and not q.any() and len(q) == 4
    assert len(identify.check_identify(model, cfg(), levels)[2]) == 31            # groups=None: one per element


# ---- 5. surface -----------------------------------------------------------------------------------------------------
def test_exports():
    import pinn_fem_amd.fem as fem
    from pinn_fem_amd.fem import identify
    for name in ("IdentifyResult", "check_identify", "identify_nr", "misfit_and_gradient"):
        assert getattr(fem, name) is getattr(identify, name) and name in fem.__all__
    fields = list(identify.IdentifyResult.__dataclass_fields__)
    assert fields[:9] == ["factors", "ea", "misfit", "gradient", "evaluations", "converged", "history", "displacements",
                          "counters"]


def test_json_block(tmp_path):
    from pinn_fem_amd.cli.generic import parse_problem
    path = os.path.join(HERE, "nl_inputs", "warren_identify.json")
    parsed = parse_problem(path)
    cfg, block = parsed["solver_config"], parsed["identify_nr"]
    assert cfg.kinematics == "green-lagrange" and cfg.method == "nr" and cfg.nr_control == "load"
    case = ir.warren_case(8)
    assert block["groups"] == case.groups.tolist() and block["max_evaluations"] == 78 and len(block["levels"]) == 3
    assert np.array_equal(parsed["model"].loads, case.loads)
    for lv, (lam, dofs, u) in zip(block["levels"], case.levels):
        # the committed measurements are what the restatement computes today
        assert lv["load_factor"] == lam and lv["dofs"] == dofs.tolist()
        assert np.max(np.abs(np.array(lv["u"]) - u)) <= 1e-12 * np.max(np.abs(u))
    with open(path) as f:
        data = json.load(f)

    def parse_with(accel, **top):
        p = tmp_path / "case.json"
        p.write_text(json.dumps(dict(data, accel=accel, **top)))
        return parse_problem(str(p))

    assert "identify_nr" not in parse_with({"kinematics": "green-lagrange"})
    good = data["accel"]["identify_nr"]
    assert parse_with({"kinematics": "green-lagrange", "identify_nr": dict(good, groups=None)})["identify_nr"]["groups"] is None
    for bad in ([1, 2], {"groups": None}, dict(good, extra=1), dict(good, levels={"load_factor": 1.0}),
                dict(good, levels=[{"load_factor": 1.0, "dofs": [4]}])):
        with pytest.raises(ValueError, match="identify_nr"):
            parse_with({"kinematics": "green-lagrange", "identify_nr": bad})
    with pytest.raises(ValueError, match='method "nr"'):
        parse_with(data["accel"], solver_config=dict(data["solver_config"], method="gd"))


C_TYPES = {"const pf_problem*": "_PP", "const pf_gl*": "_PG", "int": C.c_int, "const double*": C.c_void_p,
           "double*": C.c_void_p, "const int*": C.c_void_p, "void*": C.c_void_p}


def test_abi_declares_the_three_entry_points():
    from pinn_fem_amd import _capi
    header = open(os.path.join(os.path.dirname(HERE), "include", "pinnfem_hip.h")).read()
    assert _capi.PF_ABI_VERSION == 9 and re.search(r"#define PF_ABI_VERSION 9\b", header)
    names = {"pf_gl_state_ea": ["p", "g", "ea", "u", "stream"],
             "pf_gl_sens": ["p", "g", "u", "a", "accumulate", "out", "stream"],
             "pf_group_sum_f64": ["n_elems", "values", "weights", "group_ptr", "group_elems", "n_groups", "out", "stream"]}
    for name, args in names.items():
        assert name in _capi.SYMBOLS, name
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert decl, name
        params = [" ".join(a.split()) for a in decl.group(1).split(",")]
        assert [a.rsplit(" ", 1)[1] for a in params] == args, name
        want = [{"_PP": _capi._PP, "_PG": _capi._PG}.get(C_TYPES[a.rsplit(" ", 1)[0]], C_TYPES[a.rsplit(" ", 1)[0]])
                for a in params]
        assert _capi.SYMBOLS[name] == (C.c_int, want), name
    # the state entry point is pf_gl_state's with ea in front of u
    one, ea = _capi.SYMBOLS["pf_gl_state"][1], _capi.SYMBOLS["pf_gl_state_ea"][1]
    assert ea == one[:2] + [C.c_void_p] + one[2:]
    # no struct changed
    assert [f[0] for f in _capi.PfGl._fields_] == ["d0", "kt", "fe", "strain"]
