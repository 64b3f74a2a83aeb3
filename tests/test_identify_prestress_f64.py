"""Identification of a prestress on the device: pf_gl_prestress_rhs called through the C ABI and held against the float64
restatement tests/identify_prestress_reference.py and against the device's own internal forces, then
residuals_and_jacobian_prestress / identify_prestress / the CLI on the 8-panel Warren cantilever and the pretensioned cable,
and the two-bar truss beyond its limit load.

Every bound is derived next to its assertion from 2^-53, the operation count and the restatement's magnitude sums, or is a
stated multiple of what the CPU restatement itself shows; the measured figures are printed in front of every assertion.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import gl_reference as gl
import identify_prestress_reference as pr
import identify_reference as ir
from device_driver import (EA, U53, GlTruss, case_model, device_ids, gl_config, gl_field, gl_system, group_maps, run_cli,
                           system_cache, truss_model)

pytestmark = pytest.mark.gpu

MESHES = ["truss_1", "truss_2", "truss_257", "truss_1025", "chain_1", "chain_64"]
N_GROUPS = 5


def _system(name):
    """gl_system's meshes, but for the 1- and 2-element trusses: the irregular generator has none that small (or fixes
    every dof), so these are written out, each with free dofs at a node both elements meet."""
    if name == "truss_1":
        return GlTruss(np.array([[0.0, 0.0], [1.3, 0.7]]), np.array([[0, 1]]), np.array([0, 1]), 2)
    if name == "truss_2":
        return GlTruss(np.array([[0.0, 0.0], [1.3, 0.7], [2.1, -0.4]]), np.array([[0, 1], [2, 1]]), np.array([0, 1, 4]), 2)
    return gl_system(name)


@pytest.fixture(scope="module")
def systems():
    yield from system_cache(_system)


def _rhs_bound(S, u, ea, groups):
    """Per term +-(ea / l0) d_c: u_j - u_i 1 rounding and d0 + du 1 more, both of at most |d0_c| + |u_j,c| + |u_i,c|; l0 =
    sqrt(l0^2): the 2 relative roundings of l0^2 (the products, their sum) halve under the root to 1, the root's own 1; the
    quotient ea / l0 1; its product with d_c 1; the sign is exact: 6.  A dof's terms are added with at most deg - 1
    roundings (the first is added to 0.0, a term of another group is +0.0: both exact) of at most the sum of their
    magnitudes: (5 + deg) * 2^-53 of gl.prestress_rhs_scale per side, (10 + 2 deg) for device and restatement together (an
    FMA only takes roundings away)."""
    return (10 + 2 * S.degree)[None, :] * U53 * gl.prestress_rhs_scale(S.nodes, S.el, u, ea, groups, N_GROUPS, S.dim)


# ---------------------------------------------------------------------------------------------------------------------
# 1. pf_gl_prestress_rhs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MESHES)
def test_prestress_rhs_against_the_restatement(systems, name):
    S = systems(name)
    rng = np.random.default_rng(S.ne + 21)
    u = gl_field(S, "large", rng)
    ea = EA * np.exp2(rng.uniform(-3.0, 3.0, S.ne))
    for label, groups in group_maps(S, rng, N_GROUPS).items():
        ids = device_ids(S, groups)
        got, again = S.prestress_rhs(u, ea, ids, 0, N_GROUPS), S.prestress_rhs(u, ea, ids, 0, N_GROUPS)
        want = gl.prestress_rhs(S.nodes, S.el, u, ea, groups, N_GROUPS, S.dim)
        want[:, S.mask] = 0.0
        bound = _rhs_bound(S, u, ea, groups)
        err = np.abs(got - want)
        untouched = bound == 0.0                        # no element of the group at the node
        ratio = float(np.max(err[~untouched] / bound[~untouched], initial=0.0))
        singles = [S.prestress_rhs(u, ea, ids, k, 1)[0] for k in range(N_GROUPS)]
        differing = [k for k in range(N_GROUPS) if singles[k].tobytes() != got[k].tobytes()]
        tail = S.prestress_rhs(u, ea, ids, 2, 3)
        print(f"{name}, {label}: worst error / bound {ratio:.3f}, nonzero entries per row "
              f"{[int(np.count_nonzero(r)) for r in got]}, {int(S.mask.sum())} fixed dofs, repeat identical "
              f"{got.tobytes() == again.tobytes()}, rows that differ from their own (g0 = k, m = 1) call {differing}")
        assert np.all(np.isfinite(got)) and np.all(err <= bound)
        assert np.all(got[untouched] == 0.0) and np.all(got[:, S.mask] == 0.0)          # exact zeros
        assert got.tobytes() == again.tobytes()                                         # no atomics: the same bits
        assert not differing and tail.tobytes() == got[2:].tobytes()
        if label == "one empty group":
            assert not got[3].any()
        if label == "random":
            assert np.any(got != 0.0)


def _fint_bound(S, u, ea, e0):
    """pf_gl_fint after pf_gl_state_e0, per dof: test_gl_e0_f64.py's bound of fe_c, (8 e_abs + 16 (|e| + |e0|)) 2^-53 E A |d_c| /
    l0 per incidence (stated there for device and restatement together: an upper bound of the device's own), and deg - 1
    roundings of the node sum, each of at most the sum of the |fe_c| of the node's elements."""
    strain, fe, _, t = gl.element_state(S.nodes, S.el, u, ea, S.dim, e0=e0)
    b_fe = ((8 * t["e_abs"] + 16 * (np.abs(strain) + np.abs(t["e0"]))) * U53 * ea / t["l0"])[:, None] * np.abs(t["d"])
    per_dof, mag = np.zeros((S.n_nodes, S.dim)), np.zeros((S.n_nodes, S.dim))
    for end in (0, 1):
        np.add.at(per_dof, S.el[:, end], b_fe)
        np.add.at(mag, S.el[:, end], np.abs(fe))
    return per_dof.reshape(-1) + np.maximum(S.degree - 1, 0) * U53 * mag.reshape(-1)


@pytest.mark.parametrize("name", ["truss_257", "truss_1025", "chain_64"])
def test_prestress_rhs_is_the_difference_of_two_internal_forces(systems, name):
    """f_int is affine in e0, so f_int(e0) - f_int(e0 + tau 1_h) = tau * row h exactly; e0 (multiples of 2^-20) and tau = 2^-10
    make e0 + tau exact.  Allowed: the two pf_gl_fint calls' own derived bounds added, the rounding of their difference on the
    host (2^-53 of |f1| + |f2|), and tau times the row's own bound."""
    S = systems(name)
    rng = np.random.default_rng(S.ne + 22)
    u = gl_field(S, "large", rng)
    ea = EA * np.exp2(rng.uniform(-3.0, 3.0, S.ne))
    groups = rng.integers(0, N_GROUPS, S.ne)
    e0 = rng.integers(-1000, 1001, S.ne) * 2.0 ** -20
    tau = 2.0 ** -10
    rows = S.prestress_rhs(u, ea, device_ids(S, groups), 0, N_GROUPS)
    row_bound = _rhs_bound(S, u, ea, groups)
    S.state(u, e0, ea)
    f1 = S.fint()
    b1 = _fint_bound(S, u, ea, e0)
    for h in range(N_GROUPS):
        e0_h = e0 + tau * (groups == h)
        S.state(u, e0_h, ea)
        f2 = S.fint()
        diff = np.where(S.mask, 0.0, f1 - f2)
        allowed = b1 + _fint_bound(S, u, ea, e0_h) + U53 * (np.abs(f1) + np.abs(f2)) + tau * row_bound[h]
        err = np.abs(diff - tau * rows[h])
        print(f"{name} group {h}: |f_int(e0) - f_int(e0 + tau 1_h) - tau row| worst / allowed "
              f"{np.max(err / np.maximum(allowed, 1e-300)):.3f}, max |tau row| {np.max(np.abs(tau * rows[h])):.3e}")
        assert np.all(err <= allowed) and np.any(rows[h] != 0.0)


def test_bad_arguments_are_argument_errors(systems):
    S = systems("truss_257")
    eng, lib, capi = S.eng, S.lib, S.capi
    u, ea = S.dev(np.ones(S.n)), S.dev(np.ones(S.ne))
    ids = device_ids(S, np.zeros(S.ne, dtype=int))
    out = torch.full((2, S.n), 7.0, dtype=torch.float64, device=eng.device)
    s, P, G = eng._stream(), eng._ref(), C.byref(S.rec)
    up, ep, ip, op = u.data_ptr(), ea.data_ptr(), ids.data_ptr(), out.data_ptr()

    def problem(**mesh):
        Q = capi.PfProblem.from_buffer_copy(eng.P)
        for key, val in mesh.items():
            setattr(Q.mesh, key, val)
        return C.byref(Q)

    d0_null = capi.PfGl.from_buffer_copy(S.rec)
    d0_null.d0 = None
    f = lib.pf_gl_prestress_rhs
    calls = [lambda: f(None, G, ep, up, ip, 0, 2, op, s), lambda: f(P, None, ep, up, ip, 0, 2, op, s),
             lambda: f(P, G, None, up, ip, 0, 2, op, s), lambda: f(P, G, ep, None, ip, 0, 2, op, s),
             lambda: f(P, G, ep, up, None, 0, 2, op, s), lambda: f(P, G, ep, up, ip, 0, 2, None, s),
             lambda: f(P, G, ep, up, ip, 0, 0, op, s), lambda: f(P, G, ep, up, ip, 0, -1, op, s),
             lambda: f(P, G, ep, up, ip, 0, 65536, op, s), lambda: f(P, G, ep, up, ip, -1, 2, op, s),
             lambda: f(P, C.byref(d0_null), ep, up, ip, 0, 2, op, s),
             lambda: f(problem(dim=3), G, ep, up, ip, 0, 2, op, s), lambda: f(problem(n_elems=-1), G, ep, up, ip, 0, 2, op, s),
             lambda: f(problem(conn=None), G, ep, up, ip, 0, 2, op, s), lambda: f(problem(adj_ptr=None), G, ep, up, ip, 0, 2, op, s),
             lambda: f(problem(adj=None), G, ep, up, ip, 0, 2, op, s), lambda: f(problem(dof_flags=None), G, ep, up, ip, 0, 2, op, s),
             lambda: f(problem(n_dofs=S.n + 1), G, ep, up, ip, 0, 2, op, s)]
    for i, call in enumerate(calls):
        assert call() == capi.PF_ERR_ARG, i
        assert lib.pf_last_error().decode().startswith("pf_gl_prestress_rhs:"), (i, lib.pf_last_error())
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                                   # nothing was enqueued
    # the engine's method: the raw call's bits with no gl_state before it, ea=None, and its own checks
    rng = np.random.default_rng(5)
    uu, ee = gl_field(S, "large", rng), EA * np.exp2(rng.uniform(-1.0, 1.0, S.ne))
    groups = rng.integers(-1, 3, S.ne)
    got = eng.gl_prestress_rhs(S.dev(uu), S.dev(ee), groups)
    torch.cuda.synchronize()
    assert got.shape == (3, S.n) and got.cpu().numpy().tobytes() == S.prestress_rhs(uu, ee, device_ids(S, groups), 0, 3).tobytes()
    assert eng.gl_prestress_rhs(S.dev(uu), S.dev(ee), groups, g0=1).shape == (2, S.n)
    one = eng.gl_prestress_rhs(S.dev(uu), None, groups, g0=1, m=1)
    torch.cuda.synchronize()
    assert one.cpu().numpy().tobytes() == S.prestress_rhs(uu, np.full(S.ne, EA), device_ids(S, groups), 1, 1).tobytes()
    with pytest.raises(ValueError, match="gl_prestress_rhs: groups must hold"):
        eng.gl_prestress_rhs(S.dev(uu), None, groups[:-1])
    with pytest.raises(ValueError, match="gl_prestress_rhs: groups must hold"):
        eng.gl_prestress_rhs(S.dev(uu), None, np.where(np.arange(S.ne) == 0, -2, 0))
    with pytest.raises(ValueError, match="gl_prestress_rhs: no groups"):
        eng.gl_prestress_rhs(S.dev(uu), None, np.zeros(S.ne, dtype=int), g0=1)
    with pytest.raises(ValueError, match="gl_prestress_rhs: ea has"):
        eng.gl_prestress_rhs(S.dev(uu), S.dev(ee)[:-1], groups)


def test_the_two_group_map_slots_do_not_evict_each_other(systems):
    """The joint identification calls gl_group_rhs(groups) and gl_prestress_rhs(u, ea, pg) in turn with two maps.  On one
    engine, twice in turn: every result is, to the bit, what a fresh engine returns for that call alone, and after the first
    pair each method's cached device map stays the same tensor at the same address (the first pair's tensors are held here,
    so an upload in the second pair could not land on their addresses)."""
    from pinn_fem_amd.engine import HipEngine
    S = systems("truss_257")
    rng = np.random.default_rng(11)
    u, ea = S.dev(gl_field(S, "large", rng)), S.dev(EA * np.exp2(rng.uniform(-1.0, 1.0, S.ne)))
    groups, pg = rng.integers(0, 4, S.ne), rng.integers(-1, 3, S.ne)
    calls = (lambda eng: eng.gl_group_rhs(groups), lambda eng: eng.gl_prestress_rhs(u, ea, pg))

    def bits(eng, call):
        out = call(eng)
        torch.cuda.synchronize()
        return out.cpu().numpy().tobytes()

    want = []
    for call in calls:
        fresh = HipEngine(S.model)
        fresh.gl_state(u, ea)
        want.append(bits(fresh, call))
    eng = S.eng
    eng.gl_state(u, ea)
    assert [bits(eng, call) for call in calls] == want and want[0] != want[1]
    held = {who: slot[2] for who, slot in eng._group_maps.items()}
    ptrs = {who: t.data_ptr() for who, t in held.items()}
    assert sorted(held) == ["gl_group_rhs", "gl_prestress_rhs"] and ptrs["gl_group_rhs"] != ptrs["gl_prestress_rhs"]
    assert [bits(eng, call) for call in calls] == want
    for who, t in held.items():
        assert eng._group_maps[who][2] is t and t.data_ptr() == ptrs[who], who
    print(f"truss_257: both calls twice in turn, the bits of a fresh engine each time; device maps at {ptrs} throughout")


# ---------------------------------------------------------------------------------------------------------------------
# 2. residuals_and_jacobian_prestress, identify_prestress and the CLI
# ---------------------------------------------------------------------------------------------------------------------
def _config(case=None, **kw):
    if case is not None and np.any(case.e0_base != 0.0):
        kw["initial_strain"] = case.e0_base
    return gl_config(**kw)


def test_residuals_and_jacobian_against_the_reference():
    """rho and A = [A_q | A_t] at x = 0 on the joint Warren case, with both preconditioners.  Allowed distance: ten times
    the distance the restatement itself shows between its direct-solve result and its own result with gl.jacobi_cg at rtol
    1e-13, both computed here; the ten covers the device CG's different summation order."""
    from pinn_fem_amd.fem import residuals_and_jacobian_prestress
    case = pr.warren_case(True, True)
    q, t = np.zeros(4), np.zeros(4)
    rho_ref, A_ref, _, its_ref = ir.case_residuals(case, q, t=t)
    rho_cg, A_cg, _, _ = ir.case_residuals(case, q, linear_solve=gl.jacobi_cg(1e-13), t=t)
    tol_rho, tol_A = 10 * np.max(np.abs(rho_cg - rho_ref)), 10 * np.max(np.abs(A_cg - A_ref))
    print(f"reference: J = {rho_ref @ rho_ref:.15e}, Newton iterations {its_ref}, ten times direct against CG: {tol_rho:.2e} "
          f"(rho), {tol_A:.2e} (A); max |A_q| {np.max(np.abs(A_ref[:, :4])):.3e}, max |A_t| {np.max(np.abs(A_ref[:, 4:])):.3e}")
    model = case_model(case)
    got = {}
    for pre in ("jacobi", "two-level-updated"):
        cfg = _config(case, nr_preconditioner=pre)
        rho, A, states, counters = residuals_and_jacobian_prestress(model, cfg, case.levels, case.pgroups, t, groups=case.groups,
                                                                    q=q)
        got[pre] = (rho, A)
        print(f"{pre}: rho distance {np.max(np.abs(rho - rho_ref)):.2e} (allowed {tol_rho:.2e}), A distance "
              f"{np.max(np.abs(A - A_ref)):.2e} (allowed {tol_A:.2e}), counters {counters}")
        assert rho.shape == (90,) and A.shape == (90, 8) and len(states) == 3 and states[0].is_cuda
        assert counters["newton_iterations"] == sum(its_ref) and counters["jacobians"] == 1
        assert counters["sensitivity_cg_iterations"] > 0
        rho2, A2, _, c2 = residuals_and_jacobian_prestress(model, cfg, case.levels, case.pgroups, t, groups=case.groups, q=q,
                                                           states=states, jacobian=False)
        assert A2 is None and rho2.tobytes() == rho.tobytes()
        assert c2["newton_iterations"] == c2["sensitivity_cg_iterations"] == c2["jacobians"] == 0
        # the prestress columns alone (E*A known, the same base): the same A_t is not expected (another E*A), the shape is
        A_t = residuals_and_jacobian_prestress(model, cfg, case.levels, case.pgroups, t)[1]
        assert A_t.shape == (90, 4)
    for pre, (rho, A) in got.items():
        assert np.max(np.abs(rho - rho_ref)) <= tol_rho, pre
        assert np.max(np.abs(A - A_ref)) <= tol_A, pre


@pytest.mark.parametrize("name", ["warren-joint", "warren-prestress"])
def test_identify_prestress_recovers_the_parameters(name):
    """identify_prestress(misfit_tolerance=1e-15) from x = 0: stop "misfit" in the restatement's evaluation count, and the
    parameter errors within ten times the restatement's own (recomputed here)."""
    from pinn_fem_amd.fem import identify_prestress
    case, run = pr.reference_run(name)
    ref_t = np.max(np.abs(run["t"] - case.offsets))
    ref_q = np.max(np.abs(run["factors"] - case.factors)) if case.n_q else None
    res = identify_prestress(case_model(case), _config(case), case.levels, case.pgroups, groups=case.groups,
                             misfit_tolerance=1e-15)
    t_err = np.max(np.abs(res.prestress - case.offsets))
    q_err = np.max(np.abs(res.factors - case.factors)) if case.n_q else None
    print(f"{name}: {res.evaluations} evaluations (restatement {run['evaluations']}), stop {res.stop!r}, J per evaluation "
          f"{[h['misfit'] for h in res.history]}, t error {t_err:.2e} (restatement {ref_t:.2e}), q error {q_err} (restatement "
          f"{ref_q}), prestress_std {res.prestress_std}, factor_std {res.factor_std}, singular values {res.singular_values}, "
          f"counters {res.counters}")
    P, M = case.n_q + 4, 90
    assert res.stop == "misfit" and res.converged and res.misfit <= 1e-15
    assert res.evaluations == run["evaluations"] == (5 if case.n_q else 3) and len(res.history) == res.evaluations
    assert t_err <= 10 * ref_t
    if case.n_q:
        assert q_err <= 10 * ref_q
        assert np.allclose(res.ea, 1000.0 * res.factors[case.groups], rtol=1e-15) and res.factor_std.shape == (4,)
    else:
        assert res.factors is None and res.factor_std is None and np.all(res.ea == 1000.0)
    assert res.jacobian.shape == (M, P) and res.covariance.shape == (P, P) and res.prestress_std.shape == (4,)
    assert np.allclose(res.prestress_std, np.sqrt(np.diag(res.covariance))[case.n_q:], rtol=1e-12)
    assert np.array_equal(res.initial_strain, case.e0_base + res.prestress[case.pgroups])
    assert len(res.displacements) == 3 == len(res.strains) and res.reactions.shape == (34,) and not res.reactions[4:].any()
    assert np.allclose(res.axial_forces, res.ea * (res.strains[-1] - res.initial_strain), rtol=1e-15, atol=0.0)
    assert res.counters["jacobians"] == sum(h["accepted"] for h in res.history)


def test_cable_pretension_is_recovered():
    """The cable from the taut start t0 = -5e-3: the restatement's evaluation count (5) and -1e-2 to the 1e-9 the restatement
    itself reaches; from t0 = 0 the slack starting state is refused at the first evaluation."""
    from pinn_fem_amd.fem import identify_prestress
    case, run = pr.reference_run("cable")
    model = case_model(case)
    res = identify_prestress(model, _config(case), case.levels, case.pgroups, t0=case.t0, misfit_tolerance=1e-15)
    err = abs(res.prestress[0] + 1e-2)
    print(f"cable: {res.evaluations} evaluations (restatement {run['evaluations']}), stop {res.stop!r}, J per evaluation "
          f"{[h['misfit'] for h in res.history]}, t = {res.prestress[0]:.15e} (error {err:.2e}, restatement "
          f"{abs(run['t'][0] + 1e-2):.2e}), tension {res.axial_forces.min():.6f} .. {res.axial_forces.max():.6f}")
    assert abs(run["t"][0] + 1e-2) <= 1e-9
    assert res.stop == "misfit" and res.evaluations == run["evaluations"] == 5
    assert err <= 1e-9 and np.all(res.axial_forces > 0.0)
    with pytest.raises(RuntimeError, match="not positive definite at the starting state"):
        identify_prestress(model, _config(case), case.levels, case.pgroups)


def test_cli_identify_prestress(tmp_path):
    case = pr.warren_case(True, True)
    out = run_cli(tmp_path, "warren_identify_prestress", "warren")
    t, factors = np.array(out["identified_prestress"]), np.array(out["identified_factors"])
    print(f"CLI warren: prestress {t}, factors {factors}, {out['evaluations']} evaluations, misfit {out['misfit']:.2e}, stop "
          f"{out['stop']!r}, prestress_std {out['prestress_std']}, factor_std {out['factor_std']}")
    # no misfit tolerance in the JSON: the run goes on to the gradient, the step or the cap of 20
    assert out["stop"] in ("gradient", "step", "cap") and out["evaluations"] <= 20 and out["misfit"] < 1e-15
    assert np.max(np.abs(t - case.offsets)) <= 1e-8 and np.max(np.abs(factors - case.factors)) <= 1e-6
    assert np.allclose(out["identified_initial_strain"], case.e0_base + t[case.pgroups], rtol=0.0, atol=1e-18)
    assert len(out["displacements"]) == 34 == len(out["reactions"]) and len(out["axial_forces"]) == 31 == len(out["strains"])
    assert len(out["prestress_std"]) == 4 == len(out["factor_std"]) and np.array(out["covariance"]).shape == (8, 8)
    assert len(out["history"]) == out["evaluations"] == out["iterations"]
    cable = pr.cable_case()
    out = run_cli(tmp_path, "cable_pretension", "cable")
    print(f"CLI cable: prestress {out['identified_prestress']}, {out['evaluations']} evaluations, misfit {out['misfit']:.2e}, "
          f"stop {out['stop']!r}")
    assert abs(out["identified_prestress"][0] - cable.offsets[0]) <= 1e-8 and "identified_factors" not in out
    assert np.allclose(out["axial_forces"], 1000.0 * (np.array(out["strains"]) - out["identified_prestress"][0]), rtol=1e-12)


def test_a_level_beyond_the_limit_point_is_refused():
    """test_identify_gn_f64.py's levels at 0.5 and 2.0 of the two-bar truss's limit load: the second level's Newton loop steps
    past the limit point at the FIRST evaluation, whose error propagates."""
    from pinn_fem_amd.fem import identify_prestress, residuals_and_jacobian_prestress
    tb = gl.TwoBar(ea=EA)
    u0 = gl.newton(tb.nodes, tb.el, tb.loads(0.5 * tb.p_lim), tb.fixed, EA, 2)[0]
    model = truss_model(tb.nodes, tb.el, tb.loads(tb.p_lim), tb.fixed)
    levels = [(0.5, [5], [u0[5]]), (2.0, [5], [-0.5])]
    with pytest.raises(RuntimeError, match="not positive definite"):
        residuals_and_jacobian_prestress(model, _config(), levels, [0, 0], [0.0])
    with pytest.raises(RuntimeError, match="not positive definite"):
        identify_prestress(model, _config(), levels, [0, 0])
