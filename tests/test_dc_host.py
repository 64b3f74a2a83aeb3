"""Displacement control of the Green-Lagrange Newton solve, host side: the restatement tests/dc_reference.py against the
two-bar closed form and on a shallow Warren arch, and the configuration, JSON and ABI surface.  No GPU."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import dc_reference as dc
import gl_reference as gl

HERE = os.path.dirname(os.path.abspath(__file__))
EA = 1000.0


def test_two_bar_through_the_limit_point_and_back():
    """Apex to w = 2.2 h in 11 equal steps, control dof 5: lam = P(w) / P_lim on the rising branch, the descending one,
    the negative loads between w = h and 2 h and beyond.  Bound 1e-12 (measured 8e-16: a 1 x 1 K')."""
    tb = gl.TwoBar(ea=EA)
    f = tb.loads(tb.p_lim)
    u, lams, its = dc.control_path(tb.nodes, tb.el, f, tb.fixed, EA, 2, 5, -2.2 * tb.h, 11)
    w = np.arange(1, 12) * (2.2 * tb.h / 11)
    err = np.abs(lams - tb.load(w) / tb.p_lim)
    print(f"two-bar: lam {lams}, worst |lam - P(w)/P_lim| {err.max():.2e}, iterations {its}")
    assert np.all(err <= 1e-12)
    signs = np.sign(np.where(np.abs(lams) <= 1e-12, 0.0, lams))
    signs = signs[signs != 0.0]
    assert np.count_nonzero(np.diff(signs)) == 2                      # + - +
    # at w = h the full tangent is indefinite, the one without the control dof is not
    u0 = np.zeros(6)
    u0[5] = -tb.h
    K = gl.k_t(tb.nodes, tb.el, u0, EA, 2)
    free = gl.free_mask(6, tb.fixed)
    fc = free.copy()
    fc[5] = False
    assert gl.min_eig_ff(K, free) < -0.98 and gl.min_eig_ff(K, fc) > 190.0


@pytest.fixture(scope="module")
def arch_b():
    nodes, el, loads, fixed, c = dc.arch_warren(8, 8.0, 0.5, 0.5)
    eig = []

    def watch(u, K, free, fc):
        eig.append(float(np.linalg.eigvalsh(gl.restrict(K, fc).toarray())[0]))
    u, lams, its = dc.control_path(nodes, el, loads, fixed, EA, 2, c, -1.1, 11, on_iterate=watch)
    return nodes, el, loads, fixed, c, u, lams, its, eig


def test_arch_geometry():
    nodes, el, loads, fixed, c = dc.arch_warren(8, 8.0, 0.5, 0.5)
    assert nodes.shape == (17, 2) and len(el) == 31 and c == 17
    assert np.allclose(nodes[8], [4.0, 0.5]) and np.allclose(nodes[0], 0.0) and np.allclose(nodes[16], [8.0, 0.0])
    assert np.allclose(nodes[1], [0.5, 4 * 0.5 * 0.5 * 7.5 / 64 + 0.5])
    assert list(fixed) == [0, 1, 32, 33] and np.flatnonzero(loads).tolist() == [5, 9, 13, 17, 21, 25, 29]
    assert np.all(loads[loads != 0.0] == -1.0)


def test_arch_passes_its_limit_point(arch_b):
    nodes, el, loads, fixed, c, u, lams, its, eig = arch_b
    free = gl.free_mask(len(loads), fixed)
    res = np.abs((gl.f_int(nodes, el, u, EA, 2) - lams[-1] * loads)[free]).max()
    print(f"arch B: lam {lams}, iterations {its}, residual {res:.2e}, min eig K' {min(eig):.3f}")
    assert res <= 1e-10 and u[c] == -1.1
    assert int(np.argmax(lams)) == 4 and lams[4] > lams[3] and lams[4] > lams[5]      # increment 5
    assert abs(lams[4] - 2.347) < 1e-3 and abs(lams[-1] - 1.182) < 1e-3
    assert min(eig) > 6.0
    assert gl.min_eig_ff(gl.k_t(nodes, el, u, EA, 2), free) < 0.0


def test_arch_with_jacobi_cg_agrees_with_the_direct_solve(arch_b):
    nodes, el, loads, fixed, c, u, lams, its, eig = arch_b
    u2, lams2, _ = dc.control_path(nodes, el, loads, fixed, EA, 2, c, -1.1, 11, linear_solve=gl.jacobi_cg())
    eu, el_ = np.abs(u2 - u).max() / np.abs(u).max(), np.abs(lams2 - lams).max() / np.abs(lams).max()
    print(f"arch B, Jacobi-CG against direct: u {eu:.2e}, lam {el_:.2e}")
    assert eu <= 1e-12 and el_ <= 1e-12


# ---- configuration, JSON and ABI surface ------------------------------------------------------------------------------
def _two_bar_model(loads=None, young=2000.0):
    from pinn_fem_amd.fem.model import FEMModel, Material
    tb = gl.TwoBar(ea=EA)
    return FEMModel(nodes=tb.nodes, elements=tb.el, material=Material(young, 0.5, 1.0),
                    loads=tb.loads(tb.p_lim) if loads is None else loads, fixed_dofs=tb.fixed, dimension=2)


def test_defaults():
    from pinn_fem_amd.fem.solver import SolverConfig, SolverResult
    cfg = SolverConfig()
    assert cfg.nr_control == "load" and cfg.nr_control_dof is None and cfg.nr_control_displacement == 0.0
    assert SolverResult(displacements=np.zeros(1), reactions=np.zeros(1), converged=True).path is None


def test_every_violation_is_a_value_error_before_an_engine_is_built(monkeypatch):
    from pinn_fem_amd.fem import solver
    from pinn_fem_amd.fem.properties import NNProperty
    from pinn_fem_amd.nets import SimpleNN
    monkeypatch.setattr(solver, "_engine_for", lambda *a, **k: pytest.fail("an engine was built"))

    def cfg(**kw):
        base = dict(kinematics="green-lagrange", nr_control="displacement", nr_control_dof=5, nr_control_displacement=-0.6,
                    method="nr", n_increments=1)
        base.update(kw)
        return solver.SolverConfig(**base)

    for run in (lambda m, c: solver.solve_nr(m, c), lambda m, c: solver.solve(m, c)):
        with pytest.raises(ValueError, match=r"unknown nr_control 'arc-length'.*'load'.*'displacement'"):
            run(_two_bar_model(), cfg(nr_control="arc-length"))
        with pytest.raises(ValueError, match="green-lagrange"):
            run(_two_bar_model(), cfg(kinematics="linear"))
        nn = NNProperty(net=SimpleNN(hidden_layers=1, neurons_per_layer=4, input_dim=3), input_dim=3,
                        enforce_positive=True, scale=2000.0)
        with pytest.raises(ValueError, match="scalar materials"):
            run(_two_bar_model(young=nn), cfg())
        for dof in (None, -1, 6, 2.5):
            with pytest.raises(ValueError, match="nr_control_dof"):
                run(_two_bar_model(), cfg(nr_control_dof=dof))
        with pytest.raises(ValueError, match="fixed dof"):
            run(_two_bar_model(), cfg(nr_control_dof=1))
        with pytest.raises(ValueError, match="non-zero nr_control_displacement"):
            run(_two_bar_model(), cfg(nr_control_displacement=0.0))
        fixed_only = np.array([1.0, 0.0, 0.0, 2.0, 0.0, 0.0])
        with pytest.raises(ValueError, match="not all zero on the free dofs"):
            run(_two_bar_model(loads=fixed_only), cfg())
    with monkeypatch.context() as mp:
        mp.setattr(solver, "_world_size", lambda: 2)
        with pytest.raises(ValueError, match="sharded"):
            solver.solve_nr(_two_bar_model(), cfg())
    # the other solvers refuse it the same way
    with pytest.raises(ValueError, match="displacement"):
        solver.solve_gd(_two_bar_model(), cfg())
    with pytest.raises(ValueError, match="displacement"):
        solver.solve_hybrid(_two_bar_model(), cfg())
    for method in ("gd", "hybrid", "full-nr"):
        with pytest.raises(ValueError, match="displacement"):
            solver.solve(_two_bar_model(), cfg(method=method))
    assert solver.check_control(cfg(), _two_bar_model()) == "displacement"
    assert solver.check_control(solver.SolverConfig()) == "load"


def test_json_key(tmp_path):
    from pinn_fem_amd.cli.generic import parse_problem
    path = os.path.join(HERE, "nl_inputs", "two_bar_displacement_control.json")
    cfg = parse_problem(path)["solver_config"]
    assert (cfg.nr_control, cfg.nr_control_dof, cfg.nr_control_displacement) == ("displacement", 5, -2.2)
    assert cfg.kinematics == "green-lagrange" and cfg.method == "nr" and cfg.n_increments == 11
    with open(path) as f:
        data = json.load(f)

    def parse_with(accel):
        p = tmp_path / "case.json"
        p.write_text(json.dumps(dict(data, accel=accel)))
        return parse_problem(str(p))["solver_config"]

    cfg = parse_with({"kinematics": "green-lagrange"})
    assert (cfg.nr_control, cfg.nr_control_dof, cfg.nr_control_displacement) == ("load", None, 0.0)
    for bad in ({"dof": 5}, {"displacement": 1.0}, [5, 1.0], {"dof": 5, "displacement": 1.0, "arc": 1}):
        with pytest.raises(ValueError, match="nr_control"):
            parse_with({"kinematics": "green-lagrange", "nr_control": bad})


def test_abi_declares_the_batched_entry_points():
    from pinn_fem_amd import _capi
    header = open(os.path.join(os.path.dirname(HERE), "include", "pinnfem_hip.h")).read()
    assert _capi.PF_ABI_VERSION == 9 and re.search(r"#define PF_ABI_VERSION 9\b", header)
    assert _capi.PF_PCG_MAX_RHS == 2 and re.search(r"#define PF_PCG_MAX_RHS 2\b", header)
    for fam, single in (("pf_pcgtm_", "pf_pcgt_"), ("pf_pcg2tm_", "pf_pcg2t_")):
        for tail in ("begin", "iterations", "graph_create", "state"):
            name = fam + tail
            assert name in _capi.SYMBOLS, name
            decl = re.search(r"\bint %s\(([^;]*)\);" % name, header)
            assert decl, name
            assert re.search(r"const double\* kt,\s+int m,", decl.group(1)), name       # m behind kt
            # one more int than the single family's signature, right behind kt
            one, many = _capi.SYMBOLS[single + tail][1], _capi.SYMBOLS[name][1]
            k = 3 if fam == "pf_pcg2tm_" and tail != "state" else 2
            assert many == one[:k] + [C.c_int] + one[k:], name
