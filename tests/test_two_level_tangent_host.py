"""The two-level preconditioner of the Green-Lagrange tangent solve on the host: the package's configuration, JSON and ABI
surface of preconditioner "two-level-updated", and, on the CPU restatements (tests/gl_reference.py,
tests/two_level_reference.py, pinn_fem_amd/coarse.py, scipy's CG at rtol 1e-13), why its columns are rebuilt on the
current configuration and what that gains.  No GPU."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import gl_reference as gl
import two_level_reference as tl
import two_level_tangent_reference as tt
from device_driver import truss_model

HERE = os.path.dirname(os.path.abspath(__file__))


def _two_bar_model():
    tb = gl.TwoBar()
    return truss_model(tb.nodes, tb.el, tb.loads(0.1), tb.fixed)


# ---- 1. configuration surface ---------------------------------------------------------------------------------------
def test_configuration_surface(monkeypatch, tmp_path):
    from pinn_fem_amd.cli.generic import parse_problem
    from pinn_fem_amd.coarse import PRECONDITIONERS
    from pinn_fem_amd.fem import solver

    class Stop(Exception):
        pass

    def no_engine(*a, **k):
        raise Stop()
    assert "two-level-updated" in PRECONDITIONERS
    cfg = solver.SolverConfig(kinematics="green-lagrange", nr_preconditioner="two-level-updated", nr_aggregates=5)
    assert solver.check_kinematics(cfg.kinematics, cfg.nr_preconditioner) == "green-lagrange"
    monkeypatch.setattr(solver, "_engine_for", no_engine)
    with pytest.raises(Stop):                       # every check passed: solve_nr got as far as building an engine
        solver.solve_nr(_two_bar_model(), cfg)
    with pytest.raises(Stop):
        solver.solve_hybrid(_two_bar_model(), cfg)
    for fn in (solver.solve_nr, solver.solve_hybrid):
        with pytest.raises(ValueError, match="nothing to update"):
            fn(_two_bar_model(), solver.SolverConfig(kinematics="linear", nr_preconditioner="two-level-updated"))
        with pytest.raises(ValueError, match=r"'two-level-updated'") as e:
            fn(_two_bar_model(), solver.SolverConfig(kinematics="green-lagrange", nr_preconditioner="two-level"))
        assert "two-level" in str(e.value).replace("two-level-updated", "")        # it still names what it refuses
    # the JSON keys parse to the same configuration
    with open(os.path.join(HERE, "nl_inputs", "two_bar_green_lagrange.json")) as f:
        data = json.load(f)

    def parse_with(accel):
        p = tmp_path / "case.json"
        p.write_text(json.dumps(dict(data, accel=accel)))
        return parse_problem(str(p))["solver_config"]

    sc = parse_with({"kinematics": "green-lagrange", "nr_preconditioner": "two-level-updated", "nr_aggregates": 5})
    assert (sc.kinematics, sc.nr_preconditioner, sc.nr_aggregates) == (cfg.kinematics, cfg.nr_preconditioner, 5)
    with pytest.raises(ValueError, match="nothing to update"):
        parse_with({"nr_preconditioner": "two-level-updated"})
    with pytest.raises(ValueError, match="two-level-updated"):
        parse_with({"kinematics": "green-lagrange", "nr_preconditioner": "two-level"})


# ---- 2. ABI surface -------------------------------------------------------------------------------------------------
def test_abi_declares_the_two_level_tangent_entry_points():
    from pinn_fem_amd import _capi
    header = open(os.path.join(os.path.dirname(HERE), "include", "pinnfem_hip.h")).read()
    assert _capi.PF_ABI_VERSION == 9 and re.search(r"#define PF_ABI_VERSION 9\b", header)
    for name in ("pf_coarse_setup_t", "pf_pcg2t_begin", "pf_pcg2t_iterations", "pf_pcg2t_graph_create", "pf_pcg2t_state"):
        assert name in _capi.SYMBOLS, name
        assert re.search(r"\bint %s\(" % name, header), name
    sym = _capi.SYMBOLS
    # kt follows the coarse space (argument 2) ...
    for tail in ("begin", "iterations", "graph_create"):
        two, tan = sym["pf_pcg2_" + tail][1], sym["pf_pcg2t_" + tail][1]
        assert tan == two[:2] + [C.c_void_p] + two[2:], tail
    assert sym["pf_coarse_setup_t"][1] == sym["pf_coarse_setup"][1][:2] + [C.c_void_p] + sym["pf_coarse_setup"][1][2:]
    # ... and p in _state, as in pf_pcgt_state
    assert sym["pf_pcg2t_state"][1] == sym["pf_pcg2_state"][1][:1] + [C.c_void_p] + sym["pf_pcg2_state"][1][1:]
    assert sym["pf_pcg2t_state"] == sym["pf_pcgt_state"]
    assert "no two-level form" not in header


# ---- 3. why the current configuration -------------------------------------------------------------------------------
def test_rigid_body_columns_of_the_current_configuration_are_the_tangents_null_space():
    """A free truss turned rigidly by 0.7 rad: the tangent's null space is the rigid motions of the TURNED body.  The
    measure is, per entry of K_t Z, its size over the same entry of |K_t||Z| (the sum of the magnitudes it is made of).
    Columns on X + u: 1.2e-15, the rounding of u.  Columns on X: 0.60 (the rotation column), no cancellation at all."""
    from pinn_fem_amd.coarse import update_coarse_space
    nodes, el = gl.irregular_truss(257, np.random.default_rng(257))
    u = gl.rigid_motion(nodes, 0.7, (0.3, -0.2))
    K, Kabs = gl.k_t(nodes, el, u, 1.0, 2), gl.k_t(nodes, el, u, 1.0, 2, absolute=True)
    free = np.zeros(nodes.size, dtype=bool)
    worst = {}
    for label, X in (("current", nodes + u.reshape(-1, 2)), ("reference", nodes)):
        cs = update_coarse_space(X, 2, free, np.zeros(len(nodes), dtype=np.int32))
        assert (cs.n_agg, cs.n_coarse) == (1, 3)
        Z = tl.z_matrix(cs).toarray()
        worst[label] = float(np.max(np.abs(K @ Z) / (Kabs @ np.abs(Z))))
    print(f"max |K_t Z| / |K_t||Z|: columns on X + u {worst['current']:.2e}, on X {worst['reference']:.2f}")
    assert worst["current"] <= 1e-12
    assert worst["reference"] >= 0.1


def test_update_coarse_space_keeps_the_aggregation():
    """The named entry point: the map is taken as given (whatever the coordinates would say), the columns follow them."""
    from pinn_fem_amd.coarse import build_coarse_space, update_coarse_space
    case = tt.warren_case()
    first = build_coarse_space(case.nodes, 2, case.mask, case.n_agg)
    assert np.array_equal(first.node_agg, case.node_agg)
    u = case.states[-1][0]
    cs = update_coarse_space(case.nodes + u.reshape(-1, 2), 2, case.mask, first.node_agg)
    for name in ("node_agg", "agg_ptr", "agg_nodes"):
        assert np.array_equal(getattr(cs, name), getattr(first, name)), name
    assert cs.zcoef.shape == first.zcoef.shape and not np.array_equal(cs.zcoef, first.zcoef)
    assert not cs.zcoef[case.mask].any()
    Z = tl.z_matrix(cs)
    assert np.allclose((Z.T @ Z).toarray(), np.eye(cs.n_coarse), rtol=0, atol=1e-13)       # orthonormal per aggregate


# ---- 4. the iteration gain ------------------------------------------------------------------------------------------
def test_current_configuration_columns_take_a_tenth_of_the_jacobi_iterations():
    """Warren cantilever, 100 panels, 32 strip aggregates, E*A = 1e6, linear tip deflection a tenth of the span, four
    increments.  Measured: Jacobi 23 220 iterations over the 23 tangent solves, two-level with columns on X 2 623 (growing
    with the load), with columns on X + u 1 577 (flat); worst ratio to Jacobi 0.090."""
    case = tt.warren_case()
    assert case.its == [5, 6, 6, 6] and len(case.states) == 23
    jac, ok_j = tt.cg_counts(kind="jacobi")
    ref, ok_r = tt.cg_counts(kind="reference")
    cur, ok_c = tt.cg_counts(kind="current")
    ratio = max(c / j for c, j in zip(cur, jac))
    print(f"CG iterations over {len(cur)} tangent solves: Jacobi {sum(jac)} ({min(jac)}-{max(jac)}), columns on X {sum(ref)} "
          f"({min(ref)}-{max(ref)}), on X + u {sum(cur)} ({min(cur)}-{max(cur)}); worst ratio to Jacobi {ratio:.3f}")
    assert ok_j and ok_r and ok_c                                      # info == 0 at every state
    assert all(10 * c <= j for c, j in zip(cur, jac))
    assert sum(cur) < sum(ref)
