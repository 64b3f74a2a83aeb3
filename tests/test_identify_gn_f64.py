"""Gauss-Newton identification on the device: pf_gl_group_rhs called through the C ABI and held, bit for bit, against a
sequential host sum of the device's own element forces; HipEngine.pcg_solve_many against single pcg_solve calls; then
residuals_and_jacobian / identify_nr(method="gauss-newton") / the CLI on the 8-panel Warren cantilever against the float64
restatement tests/identify_gn_reference.py, and the two-bar truss beyond its limit load.

The group right-hand sides are pure additions in a fixed order, so they are compared without a tolerance.  Every other
bound is a stated multiple of what the CPU restatement itself shows between its direct and its CG solves, or follows from
the stop rule; the measured figures are printed in front of every assertion.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import gl_reference as gl
import identify_reference as ir
from device_driver import (AREA, EA, RTOL, YOUNG, DeviceTruss, case_model, device_ids, gl_config, gl_field, gl_system,
                           group_maps, irregular_truss_with_supports, run_cli, system_cache, truss_model)

pytestmark = pytest.mark.gpu

MESHES = ["truss_1", "truss_255", "truss_257", "truss_1025", "chain_1", "chain_257"]
N_GROUPS = 5
RANGES = [(0, 5), (2, 2), (4, 1)]


@pytest.fixture(scope="module")
def systems():
    yield from system_cache(gl_system)


# ---------------------------------------------------------------------------------------------------------------------
# 1. pf_gl_group_rhs
# ---------------------------------------------------------------------------------------------------------------------
def _host_rhs(S, fe, groups, g):
    """Minus the sum of +-fe over the elements of group g, per node in ascending element id, one addition at a time;
    0.0 on the fixed dofs."""
    acc = np.zeros((S.n_nodes, S.dim))
    for e in np.flatnonzero(groups == g):
        i, j = S.el[e]
        acc[j] = acc[j] + fe[e]
        acc[i] = acc[i] + (-fe[e])
    out = -acc.reshape(-1)
    out[S.mask] = 0.0
    return out


@pytest.mark.parametrize("name", MESHES)
def test_group_rhs_is_the_sequential_host_sum_bit_for_bit(systems, name):
    S = systems(name)
    rng = np.random.default_rng(77)
    fe = S.state(gl_field(S, "large", rng))[1]
    assert np.all(np.isfinite(fe)) and np.any(fe != 0.0)
    for label, groups in group_maps(S, rng, N_GROUPS).items():
        ids = device_ids(S, groups)
        want = {g: _host_rhs(S, fe, groups, g) for g in range(N_GROUPS)}
        for g0, m in RANGES:
            got = S.group_rhs(ids, g0, m)
            again = S.group_rhs(ids, g0, m)
            differing = [g0 + k for k in range(m) if got[k].tobytes() != want[g0 + k].tobytes()]
            nonzero = [int(np.count_nonzero(got[k])) for k in range(m)]
            print(f"{name}, {label}, (g0, m) = ({g0}, {m}): rows that differ from the host sum {differing}, nonzero entries "
                  f"per row {nonzero}, repeat identical {got.tobytes() == again.tobytes()}")
            assert not differing
            assert got.tobytes() == again.tobytes()
            assert not got[:, S.mask].any()
        if label == "one empty group":
            assert not S.group_rhs(ids, 3, 1).any()


@pytest.mark.parametrize("name", MESHES)
def test_one_group_is_minus_the_internal_force(systems, name):
    S = systems(name)
    S.state(gl_field(S, "large", np.random.default_rng(78)))
    fint = S.fint()
    got = S.group_rhs(device_ids(S, np.zeros(S.ne, dtype=int)), 0, 1)[0]
    same = got[S.free].tobytes() == (-fint)[S.free].tobytes()
    print(f"{name}: every element in one group: -f_int on the {int(S.free.sum())} free dofs to the bit: {same}; "
          f"max |f_int| {np.max(np.abs(fint)):.3e}")
    assert same and not got[S.mask].any() and fint[S.mask].any()


def test_group_rhs_argument_errors(systems):
    S = systems("truss_257")
    eng, lib, capi = S.eng, S.lib, S.capi
    S.state(np.zeros(S.n))
    ids = device_ids(S, np.zeros(S.ne, dtype=int))
    out = torch.full((2, S.n), 7.0, dtype=torch.float64, device=eng.device)
    S.fe.fill_(7.0)
    s, P, G, ip, op = eng._stream(), eng._ref(), C.byref(S.rec), ids.data_ptr(), out.data_ptr()

    def problem(**mesh):
        Q = capi.PfProblem.from_buffer_copy(eng.P)
        for key, val in mesh.items():
            setattr(Q.mesh, key, val)
        return C.byref(Q)

    fe_null = capi.PfGl.from_buffer_copy(S.rec)
    fe_null.fe = None
    calls = [lambda: lib.pf_gl_group_rhs(None, G, ip, 0, 2, op, s), lambda: lib.pf_gl_group_rhs(P, None, ip, 0, 2, op, s),
             lambda: lib.pf_gl_group_rhs(P, G, None, 0, 2, op, s), lambda: lib.pf_gl_group_rhs(P, G, ip, 0, 2, None, s),
             lambda: lib.pf_gl_group_rhs(P, G, ip, 0, 0, op, s), lambda: lib.pf_gl_group_rhs(P, G, ip, 0, -1, op, s),
             lambda: lib.pf_gl_group_rhs(P, G, ip, -1, 2, op, s),
             lambda: lib.pf_gl_group_rhs(P, C.byref(fe_null), ip, 0, 2, op, s),
             lambda: lib.pf_gl_group_rhs(problem(dim=3), G, ip, 0, 2, op, s),
             lambda: lib.pf_gl_group_rhs(problem(n_elems=-1), G, ip, 0, 2, op, s),
             lambda: lib.pf_gl_group_rhs(problem(adj_ptr=None), G, ip, 0, 2, op, s),
             lambda: lib.pf_gl_group_rhs(problem(dof_flags=None), G, ip, 0, 2, op, s)]
    for i, call in enumerate(calls):
        assert call() == capi.PF_ERR_ARG, i
        assert lib.pf_last_error().decode().startswith("pf_gl_group_rhs:"), (i, lib.pf_last_error())
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((S.fe == 7.0).all()) and not bool(ids.any())        # nothing was enqueued
    # the engine: a group map of the wrong length, negative ids, an empty range, no state yet
    eng.gl_state(S.dev(np.zeros(S.n)))
    with pytest.raises(ValueError, match="gl_group_rhs"):
        eng.gl_group_rhs(np.zeros(S.ne - 1, dtype=int))
    with pytest.raises(ValueError, match="gl_group_rhs"):
        eng.gl_group_rhs(np.where(np.arange(S.ne) == 0, -1, 0))
    with pytest.raises(ValueError, match="gl_group_rhs"):
        eng.gl_group_rhs(np.zeros(S.ne, dtype=int), g0=1)
    assert eng.gl_group_rhs(np.arange(S.ne) % 3).shape == (3, S.n)
    assert eng.gl_group_rhs(np.arange(S.ne) % 3, g0=1).shape == (2, S.n)
    assert eng.gl_group_rhs(np.arange(S.ne) % 3, g0=1, m=1).shape == (1, S.n)


# ---------------------------------------------------------------------------------------------------------------------
# 2. pcg_solve_many
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def truss():
    """test_pcg_batch.py's system: a 1000-element irregular truss at a stretched state with a positive definite tangent."""
    nodes, el, fixed = irregular_truss_with_supports(1000, np.random.default_rng(2000))
    rng = np.random.default_rng(11)
    mean_l0 = float(np.mean(np.linalg.norm(nodes[el[:, 1]] - nodes[el[:, 0]], axis=1)))
    S = DeviceTruss(nodes, el, fixed, 2, YOUNG, AREA)
    S.u = 0.05 * nodes.reshape(-1) + 0.02 * (0.3 * mean_l0 / math.sqrt(4.0)) * rng.standard_normal(nodes.size)
    assert np.linalg.eigvalsh(gl.restrict(gl.k_t(S.nodes, S.el, S.u, EA, 2), S.free).toarray())[0] > 0.0
    S.groups = rng.integers(0, N_GROUPS, S.ne)
    yield S
    torch.cuda.empty_cache()


@pytest.mark.parametrize("pre", ["jacobi", "two-level-updated"])
def test_pcg_solve_many_equals_its_single_solves(truss, pre):
    """Five right-hand sides (the group right-hand sides of the state: two pairs and one alone): every row equals its own
    pcg_solve bit for bit, behind one coarse-space refresh."""
    S, eng = truss, truss.eng
    u = S.dev(S.u)
    eng.gl_state(u)
    B = eng.gl_group_rhs(S.groups)
    assert B.shape == (N_GROUPS, S.n)
    kw = dict(preconditioner=pre, n_aggregates=8, u=u, rtol=RTOL)
    singles = [eng.pcg_solve(B[k], tangent=True, **kw) for k in range(N_GROUPS)]
    refreshes, iterations = eng.coarse_refreshes, eng.pcg_iterations
    X, reports = eng.pcg_solve_many(B, **kw)
    torch.cuda.synchronize()
    grown = eng.coarse_refreshes - refreshes
    differing = [k for k in range(N_GROUPS) if X[k].cpu().numpy().tobytes() != singles[k][0].cpu().numpy().tobytes()]
    print(f"{pre}: iterations per row {[r[0] for r in reports]}, rows that differ from their own pcg_solve {differing}, "
          f"coarse refreshes {grown}")
    assert X.shape == (N_GROUPS, S.n) and len(reports) == N_GROUPS
    assert not differing
    for k in range(N_GROUPS):
        assert reports[k] == singles[k][1:] and reports[k][1] and reports[k][0] > 16, k
    assert eng.pcg_iterations - iterations == sum(r[0] for r in reports)
    assert grown == (1 if pre == "two-level-updated" else 0)
    with pytest.raises(ValueError, match="pcg_solve_many"):
        eng.pcg_solve_many(B[0], **kw)
    with pytest.raises(ValueError, match="no tangent form"):
        eng.pcg_solve_many(B, preconditioner="two-level")


# ---------------------------------------------------------------------------------------------------------------------
# 3. residuals_and_jacobian, identify_nr and the CLI on the 8-panel Warren cantilever
# ---------------------------------------------------------------------------------------------------------------------
def test_residuals_and_jacobian_against_the_reference():
    """rho, A and 2 A^T rho at all factors 1, with both preconditioners.  Allowed distance: ten times the distance the
    restatement itself shows between its direct-solve result and its own result with gl.jacobi_cg at rtol 1e-13, both
    computed here (test_misfit_and_gradient_against_the_reference's rule).  2 A^T rho is also held to the device's own
    adjoint gradient (misfit_and_gradient + group_sum) under the allowance of the gradient."""
    from pinn_fem_amd.fem.identify import misfit_and_gradient, residuals_and_jacobian
    case = ir.warren_case(8)
    q = np.zeros(4)
    rho_ref, A_ref, _, its_ref = ir.case_residuals(case, q)
    rho_cg, A_cg, _, _ = ir.case_residuals(case, q, linear_solve=gl.jacobi_cg(1e-13))
    g_ref, g_cg = 2.0 * A_ref.T @ rho_ref, 2.0 * A_cg.T @ rho_cg
    tol_rho, tol_A, tol_g = (10 * np.max(np.abs(rho_cg - rho_ref)), 10 * np.max(np.abs(A_cg - A_ref)),
                             10 * np.max(np.abs(g_cg - g_ref)))
    print(f"reference: J = {rho_ref @ rho_ref:.15e}, Newton iterations {its_ref}, ten times direct against CG: "
          f"{tol_rho:.2e} (rho), {tol_A:.2e} (A), {tol_g:.2e} (2 A^T rho)")
    model = case_model(case)
    ea = case.ea(q)
    got = {}
    for pre in ("jacobi", "two-level-updated"):
        cfg = gl_config(nr_preconditioner=pre)
        rho, A, states, counters = residuals_and_jacobian(model, cfg, case.levels, ea, case.groups)
        eng = model._pf_engine_cache[1]
        J_adj, g_ea, _, _ = misfit_and_gradient(model, cfg, case.levels, ea)
        g_adj = eng.group_sum(g_ea, torch.from_numpy(ea).to(eng.device), case.groups).cpu().numpy()
        g = 2.0 * A.T @ rho
        got[pre] = (rho, A, g_adj)
        print(f"{pre}: rho distance {np.max(np.abs(rho - rho_ref)):.2e} (allowed {tol_rho:.2e}), A distance "
              f"{np.max(np.abs(A - A_ref)):.2e} (allowed {tol_A:.2e}), 2 A^T rho against the reference "
              f"{np.max(np.abs(g - g_ref)):.2e} and against the device's adjoint gradient {np.max(np.abs(g - g_adj)):.2e} "
              f"(allowed {tol_g:.2e}), rho.rho - J = {rho @ rho - J_adj:.2e}, counters {counters}")
        assert rho.shape == (90,) and A.shape == (90, 4) and len(states) == 3 and states[0].is_cuda
        assert counters["newton_iterations"] == sum(its_ref) and counters["jacobians"] == 1
        assert counters["sensitivity_cg_iterations"] > 0 and counters["adjoint_cg_iterations"] == 0
        # states given: no Newton solves, the same rho; without a Jacobian: None and no sensitivity solves
        rho2, A2, _, c2 = residuals_and_jacobian(model, cfg, case.levels, ea, case.groups, states=states, jacobian=False)
        assert A2 is None and rho2.tobytes() == rho.tobytes()
        assert c2["newton_iterations"] == c2["sensitivity_cg_iterations"] == c2["jacobians"] == 0
    for pre, (rho, A, g_adj) in got.items():
        assert np.max(np.abs(rho - rho_ref)) <= tol_rho, pre
        assert np.max(np.abs(A - A_ref)) <= tol_A, pre
        assert np.max(np.abs(2.0 * A.T @ rho - g_ref)) <= tol_g, pre
        assert np.max(np.abs(2.0 * A.T @ rho - g_adj)) <= tol_g, pre


@pytest.mark.parametrize("n_groups", [4, 8])
def test_gauss_newton_recovers_the_factors(n_groups):
    """identify_nr(method="gauss-newton", misfit_tolerance=1e-15) from all factors 1: stop "misfit" in at most one
    evaluation more than the restatement takes (one more for a step that CG-solved states reject), and
    max |q - q_true| <= 2 (sqrt J + 1e-10 max_k |u_k|) / sigma_min(A): the first-order bound A dq = rho from the stop rule
    and the Newton tolerance (|du| <= 1e-10 |u_k| in the Euclidean norm), the factor 2 covering the linearisation."""
    from pinn_fem_amd.fem import identify_nr
    case, run = ir.reference_run(n_groups)
    model = case_model(case)
    res = identify_nr(model, gl_config(), case.levels, groups=case.groups, method="gauss-newton", misfit_tolerance=1e-15)
    A, M, G = res.jacobian, 90, n_groups
    q_err = np.max(np.abs(np.log(res.factors) - np.log(case.factors)))
    u_max = max(float(np.linalg.norm(u)) for u in res.displacements)
    bound = 2.0 * (math.sqrt(res.misfit) + 1e-10 * u_max) / res.singular_values[-1]
    print(f"{n_groups} groups: {res.evaluations} evaluations (restatement {run['evaluations']}), stop {res.stop!r}, J per "
          f"evaluation {[f'''{h['misfit']:.1e}''' for h in res.history]}, max |q - q_true| = {q_err:.2e} (bound {bound:.2e}), "
          f"singular values {res.singular_values[0]:.3e} .. {res.singular_values[-1]:.3e}, factor_std {res.factor_std}, "
          f"counters {res.counters}")
    assert res.stop == "misfit" and res.converged and res.misfit <= 1e-15
    assert res.evaluations <= run["evaluations"] + 1 and len(res.history) == res.evaluations
    assert q_err <= bound
    # the documented shapes and definitions, from `jacobian`
    assert A.shape == (M, G) and res.singular_values.shape == (G,) and res.covariance.shape == (G, G)
    assert res.factor_std.shape == (G,) and res.gradient.shape == (G,)
    assert np.array_equal(res.singular_values, np.linalg.svd(A, compute_uv=False))
    assert np.array_equal(res.covariance, res.misfit / (M - G) * np.linalg.inv(A.T @ A))
    assert np.array_equal(res.factor_std, res.factors * np.sqrt(np.diag(res.covariance)))
    rho = np.concatenate([(u[dofs] - ubar) / math.sqrt(len(dofs)) for u, (_, dofs, ubar) in zip(res.displacements, case.levels)])
    assert abs(rho @ rho - res.misfit) <= 1e-12 * res.misfit and np.allclose(res.gradient, 2.0 * A.T @ rho, rtol=1e-12, atol=0.0)
    assert all(h["accepted"] == (h["gradient_norm"] is not None) and h["damping"] > 0.0 for h in res.history)
    assert np.allclose(res.ea, 1000.0 * res.factors[case.groups], rtol=1e-15)
    assert len(res.displacements) == 3 and res.reactions.shape == (34,) and not res.reactions[4:].any()
    assert res.counters["jacobians"] == sum(h["accepted"] for h in res.history)
    if n_groups == 4:
        # L-BFGS on the same model is as before: none of the Gauss-Newton fields
        old = identify_nr(model, gl_config(), case.levels, groups=case.groups, max_evaluations=2)
        assert old.jacobian is None and old.singular_values is None and old.covariance is None
        assert old.factor_std is None and old.stop is None and old.evaluations == 2
        assert set(old.history[0]) == {"misfit", "gradient_norm", "factors"} and set(old.counters) == {
            "newton_iterations", "cg_iterations", "adjoint_cg_iterations"}


def test_evaluation_cap_and_a_group_that_moves_nothing():
    from pinn_fem_amd.fem import identify_nr
    case = ir.warren_case(8)
    model = case_model(case)
    res = identify_nr(model, gl_config(), case.levels, groups=case.groups, method="gauss-newton", max_evaluations=2)
    print(f"cap 2: stop {res.stop!r}, misfit {[h['misfit'] for h in res.history]}")
    assert res.stop == "cap" and not res.converged and res.evaluations == 2 and res.misfit < res.history[0]["misfit"]
    # element 1 joins the two clamped nodes: a group of its own moves no dof at all
    assert set(case.el[1]) == {0, 1} and set(case.fixed) == {0, 1, 2, 3}
    groups = np.where(np.arange(31) == 1, 4, case.groups)
    with pytest.raises(RuntimeError, match="group 4 moves no measured dof"):
        identify_nr(model, gl_config(), case.levels, groups=groups, method="gauss-newton")


def test_cli_identify_gauss_newton(tmp_path):
    case, run = ir.reference_run(4)
    out = run_cli(tmp_path, "warren_identify_gn", "warren")
    factors = np.array(out["identified_factors"])
    print(f"CLI: factors {factors}, {out['evaluations']} evaluations, misfit {out['misfit']:.2e}, stop {out['stop']!r}, "
          f"factor_std {out['factor_std']}, singular values {out['singular_values']}")
    # no misfit tolerance in the JSON: the run goes on to the gradient, the step or the cap of 20, past the restatement's 5
    assert out["stop"] in ("gradient", "step", "cap") and out["evaluations"] <= 20
    assert np.max(np.abs(factors - case.factors)) <= 1e-6 and out["misfit"] < 1e-15
    assert np.allclose(out["identified_ea"], 1000.0 * factors[case.groups], rtol=1e-15)
    assert len(out["displacements"]) == 34 and len(out["reactions"]) == 34
    assert len(out["history"]) == out["evaluations"] == out["iterations"]
    assert set(out["history"][-1]) == {"misfit", "gradient_norm", "factors", "accepted", "damping"}
    assert len(out["factor_std"]) == 4 == len(out["singular_values"]) and np.array(out["covariance"]).shape == (4, 4)
    assert np.allclose(out["factor_std"], factors * np.sqrt(np.diag(out["covariance"])), rtol=1e-12)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the two-bar truss
# ---------------------------------------------------------------------------------------------------------------------
def test_a_level_beyond_the_limit_point_is_refused():
    """test_identify_f64.py's levels at 0.5 and 2.0 of the limit load: the second level's Newton loop steps past the limit
    point, and gauss-newton propagates the existing error as L-BFGS does."""
    from pinn_fem_amd.fem import identify_nr
    from pinn_fem_amd.fem.identify import residuals_and_jacobian
    tb = gl.TwoBar(ea=EA)
    u0 = gl.newton(tb.nodes, tb.el, tb.loads(0.5 * tb.p_lim), tb.fixed, EA, 2)[0]
    model = truss_model(tb.nodes, tb.el, tb.loads(tb.p_lim), tb.fixed)
    levels = [(0.5, [5], [u0[5]]), (2.0, [5], [-0.5])]
    with pytest.raises(RuntimeError, match="not positive definite"):
        residuals_and_jacobian(model, gl_config(), levels, np.full(2, EA), [0, 0])
    with pytest.raises(RuntimeError, match="not positive definite"):
        identify_nr(model, gl_config(), levels, groups=[0, 0], method="gauss-newton")
