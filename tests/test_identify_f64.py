"""Identification through the Green-Lagrange Newton solve on the device: pf_gl_state_ea, pf_gl_sens and pf_group_sum_f64
called through the C ABI and held against the float64 restatements (tests/gl_reference.py, tests/identify_reference.py),
then misfit_and_gradient / identify_nr / the CLI on the 8-panel Warren cantilever and the two-bar truss.

Every bound is derived next to its assertion from 2^-53 and operation counts, or is a stated multiple of what the CPU
restatement itself shows between its direct and its CG solves.  The measured figures are printed in front of every
assertion.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import gl_reference as gl
import identify_reference as ir
from device_driver import EA, U53, case_model, check_state, gl_config, gl_field, gl_system, run_cli, system_cache, truss_model

pytestmark = pytest.mark.gpu

MESHES = ["truss_1", "truss_255", "truss_256", "truss_257", "truss_1025", "chain_1", "chain_257"]


@pytest.fixture(scope="module")
def systems():
    yield from system_cache(gl_system)


# ---------------------------------------------------------------------------------------------------------------------
# 1. pf_gl_state_ea
# ---------------------------------------------------------------------------------------------------------------------
def _state_bounds(S, u, ea):
    """tests/test_gl_f64.py's _state_bounds with E*A per element: the same operation counts (ea enters every product
    where the scalar did), in units of 2^-53:
      e:   8 e_abs for device and reference together, e_abs = (2 |d0|.|du| + |du|.|du|) / (2 l0^2)
      fe_c = (ea e / l0) d_c: e's error, then 14 relative to |fe_c|
      B_rc = (ea / l0^3) d_r d_c + delta_rc ea e / l0: 25 on the first term, fe's chain without d_c on the second."""
    strain, fe, B, t = gl.element_state(S.nodes, S.el, u, ea, S.dim)
    ea = np.broadcast_to(np.asarray(ea, dtype=np.float64), strain.shape)
    e_abs = (2.0 * np.sum(np.abs(t["d0"]) * np.abs(t["du"]), axis=1) + np.sum(t["du"] ** 2, axis=1)) / (2.0 * t["l02"])
    b_e = 8 * U53 * e_abs
    n_l0 = (b_e + 14 * U53 * np.abs(strain)) * ea / t["l0"]
    b_fe = n_l0[:, None] * np.abs(t["d"])
    k = ea / (t["l02"] * t["l0"])
    dd = np.abs(t["d"][:, :, None] * t["d"][:, None, :])
    b_B = 25 * U53 * k[:, None, None] * dd + n_l0[:, None, None] * np.eye(S.dim)
    if S.dim == 2:
        pick = lambda M: np.stack([M[:, 0, 0], M[:, 0, 1], M[:, 1, 1]], axis=1)
    else:
        pick = lambda M: M[:, 0, 0][:, None]
    return (strain, b_e), (fe, b_fe), (pick(B), pick(b_B))


@pytest.mark.parametrize("kind", ["large", "tiny"])
@pytest.mark.parametrize("name", MESHES)
def test_gl_state_ea_against_the_restatement(systems, name, kind):
    """Element counts 1, on both sides of the block (255, 256, 257) and on several blocks (1025), 1-D chains of 1 and
    257; E*A drawn per element from [500, 2000]."""
    S = systems(name)
    rng = np.random.default_rng(S.ne + 5)
    u, ea = gl_field(S, kind, rng), rng.uniform(500.0, 2000.0, S.ne)
    check_state(S.state(u, ea=ea), _state_bounds(S, u, ea), f"{name} {kind} per-element ea")
    # pf_gl_state itself: the restatement bound of tests/test_gl_f64.py with the model's scalar E*A ...
    scalar = S.state(u)
    check_state(scalar, _state_bounds(S, u, EA), f"{name} {kind} pf_gl_state")
    # ... and pf_gl_state_ea with ea filled with that scalar gives its bits
    filled = S.state(u, ea=np.full(S.ne, EA))
    for what, a, b in zip(("strain", "fe", "kt"), filled, scalar):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), what


# ---------------------------------------------------------------------------------------------------------------------
# 2. pf_gl_sens
# ---------------------------------------------------------------------------------------------------------------------
def _sens_bound(S, u, a):
    """s = -(e / l0) sum_c d_c (a_j,c - a_i,c).  Per side, in units of 2^-53 of (e_abs / l0) sum_c |d_c| (|a_j,c| + |a_i,c|)
    (gl.sensitivity_scale): e 4 (half of the 8 e_abs of the state bounds), l0 = sqrt(l0^2) 2.5 (l0^2: 3, halved by the
    root, + 1), the division 1, d_c 1, a_j - a_i 1, their product 1, the sum over c 1, the last product 1: 12.5; 25 for
    device and reference together."""
    return 25 * U53 * gl.sensitivity_scale(S.nodes, S.el, u, a, S.dim)


@pytest.mark.parametrize("name", MESHES)
def test_gl_sens_against_the_restatement(systems, name):
    S = systems(name)
    rng = np.random.default_rng(S.ne + 6)
    for kind in ("large", "tiny"):
        u = gl_field(S, kind, rng)
        a1, a2 = rng.standard_normal(S.n), rng.standard_normal(S.n) * np.exp2(rng.uniform(-8.0, 8.0, S.n))
        one = S.sens(u, a1).cpu().numpy()
        want, bound = gl.element_sensitivity(S.nodes, S.el, u, a1, S.dim), _sens_bound(S, u, a1)
        err = np.abs(one - want)
        print(f"{name} {kind}: sensitivity worst error / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}, "
              f"relative {np.max(err) / np.max(np.abs(want)):.2e}")
        assert np.all(np.isfinite(one)) and np.all(err <= bound)
        # a rigid translation of the adjoint: a_j - a_i is exactly zero in every element
        shift = np.tile([3.0, -2.5][: S.dim], S.n_nodes)
        rigid = S.sens(u, shift).cpu().numpy()
        assert np.all(rigid == 0.0)
        # accumulate: out + s with s rounded first, so the sum of two single calls to one rounding per element
        two = S.sens(u, a2).cpu().numpy()
        acc = S.sens(u, a1)
        acc = S.sens(u, a2, accumulate=1, out=acc).cpu().numpy()
        err = np.abs(acc - (one + two))
        print(f"{name} {kind}: accumulated against the sum of two calls, worst {np.max(err / np.maximum(np.abs(one + two), 1e-300)) / U53:.2f} * 2^-53")
        assert np.all(err <= U53 * np.abs(one + two))


# ---------------------------------------------------------------------------------------------------------------------
# 3. pf_group_sum_f64
# ---------------------------------------------------------------------------------------------------------------------
def _group_sum(lib, capi, values, weights, groups, n_groups, device="cuda"):
    """pf_group_sum_f64 with a CSR built here (group -> elements in ascending element id); out pre-filled with 7.0."""
    groups = np.asarray(groups, dtype=np.int64)
    ptr = np.zeros(n_groups + 1, dtype=np.int32)
    np.cumsum(np.bincount(groups, minlength=n_groups), out=ptr[1:])
    order = np.argsort(groups, kind="stable").astype(np.int32)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    v, p, o = dev(values), dev(ptr), dev(order)
    w = None if weights is None else dev(weights)
    out = torch.full((n_groups,), 7.0, dtype=torch.float64, device=device)
    capi.check(lib.pf_group_sum_f64(len(groups), v.data_ptr(), None if w is None else w.data_ptr(), p.data_ptr(),
                                    o.data_ptr(), n_groups, out.data_ptr(), torch.cuda.current_stream().cuda_stream),
               "pf_group_sum_f64")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check_group_sum(lib, capi, values, weights, groups, n_groups, label):
    """|out_g - fsum| <= (n_g + 1) 2^-53 sum|terms|: one rounding for each product and fewer than n_g for the additions
    (a thread's strided partial sum, six shuffle steps, four wave sums)."""
    got = _group_sum(lib, capi, values, weights, groups, n_groups)
    again = _group_sum(lib, capi, values, weights, groups, n_groups)
    terms = values * (1.0 if weights is None else weights)
    worst = 0.0
    for g in range(n_groups):
        t = terms[groups == g]
        want, unit = math.fsum(t), (len(t) + 1) * U53 * math.fsum(np.abs(t))
        assert abs(got[g] - want) <= unit, (label, g, len(t))
        worst = max(worst, abs(got[g] - want) / unit if unit else 0.0)
        if len(t) == 0:
            assert got[g] == 0.0 and not np.signbit(got[g])
    print(f"{label}: {n_groups} groups, worst error / bound {worst:.3f}")
    assert np.array_equal(got.view(np.uint64), again.view(np.uint64))          # no atomics: the same bits
    return got


def test_group_sum_against_fsum(systems):
    S = systems("truss_257")
    lib, capi = S.lib, S.capi
    rng = np.random.default_rng(42)
    sizes = [0, 1, 255, 256, 257, 1000]                     # empty, one, both sides of the block, several strides
    groups = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))
    n = len(groups)
    values = rng.standard_normal(n) * np.exp2(rng.uniform(-20.0, 20.0, n))
    weights = rng.uniform(500.0, 2000.0, n)
    _check_group_sum(lib, capi, values, weights, groups, len(sizes), "mixed sizes")
    _check_group_sum(lib, capi, values, None, groups, len(sizes), "mixed sizes, null weights")
    _check_group_sum(lib, capi, values, weights, np.zeros(n, dtype=np.int64), 1, "one group")
    perm = rng.permutation(n)
    each = _check_group_sum(lib, capi, values, weights, perm, n, "a group per element")
    assert np.array_equal(each[perm], values * weights)                      # one term: the rounded product itself
    # the engine's group_sum: the same kernel behind a cached CSR
    T = systems("truss_1025")
    gm = rng.integers(0, 7, T.ne)
    v, w = rng.standard_normal(T.ne), rng.uniform(500.0, 2000.0, T.ne)
    want = _group_sum(lib, capi, v, w, gm, 7)
    for _ in range(2):                                       # the second call takes the CSR from the cache
        got = T.eng.group_sum(T.dev(v), T.dev(w), gm)
        torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy().view(np.uint64), want.view(np.uint64))
    assert T.eng._group_csr[1] == 7
    with pytest.raises(ValueError, match="group_sum"):
        T.eng.group_sum(T.dev(v), None, gm[:-1])
    with pytest.raises(ValueError, match="group_sum"):
        T.eng.group_sum(T.dev(v), None, np.where(np.arange(T.ne) == 0, -1, gm))


# ---------------------------------------------------------------------------------------------------------------------
# 4. argument errors
# ---------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_argument_errors(systems):
    S = systems("truss_257")
    eng, lib, capi = S.eng, S.lib, S.capi
    S.state(np.zeros(S.n))
    u, a, ea = S.dev(np.ones(S.n)), S.dev(np.ones(S.n)), S.dev(np.full(S.ne, EA))
    out = torch.full((S.ne,), 7.0, dtype=torch.float64, device=eng.device)
    S.refill()
    s, P, G = eng._stream(), eng._ref(), C.byref(S.rec)
    up, ap, ep, op = u.data_ptr(), a.data_ptr(), ea.data_ptr(), out.data_ptr()

    def problem(**mesh):
        Q = capi.PfProblem.from_buffer_copy(eng.P)
        for key, val in mesh.items():
            setattr(Q.mesh, key, val)
        return C.byref(Q)

    def record(**kw):
        R = capi.PfGl.from_buffer_copy(S.rec)
        for key, val in kw.items():
            setattr(R, key, val)
        return C.byref(R)

    ptr = torch.zeros(3, dtype=torch.int32, device=eng.device)
    ids = torch.zeros(S.ne, dtype=torch.int32, device=eng.device)
    gout = torch.full((2,), 7.0, dtype=torch.float64, device=eng.device)
    pp, ip, gp = ptr.data_ptr(), ids.data_ptr(), gout.data_ptr()
    calls = {
        "pf_gl_state_ea": [lambda: lib.pf_gl_state_ea(None, G, ep, up, s), lambda: lib.pf_gl_state_ea(P, None, ep, up, s),
                           lambda: lib.pf_gl_state_ea(P, G, None, up, s), lambda: lib.pf_gl_state_ea(P, G, ep, None, s),
                           lambda: lib.pf_gl_state_ea(problem(dim=3), G, ep, up, s),
                           lambda: lib.pf_gl_state_ea(problem(n_elems=-1), G, ep, up, s),
                           lambda: lib.pf_gl_state_ea(P, record(d0=None), ep, up, s),
                           lambda: lib.pf_gl_state_ea(P, record(kt=None), ep, up, s)],
        "pf_gl_sens": [lambda: lib.pf_gl_sens(None, G, up, ap, 0, op, s), lambda: lib.pf_gl_sens(P, None, up, ap, 0, op, s),
                       lambda: lib.pf_gl_sens(P, G, None, ap, 0, op, s), lambda: lib.pf_gl_sens(P, G, up, None, 0, op, s),
                       lambda: lib.pf_gl_sens(P, G, up, ap, 0, None, s), lambda: lib.pf_gl_sens(P, G, up, ap, 2, op, s),
                       lambda: lib.pf_gl_sens(P, G, up, ap, -1, op, s),
                       lambda: lib.pf_gl_sens(problem(dim=3), G, up, ap, 0, op, s),
                       lambda: lib.pf_gl_sens(problem(n_elems=-1), G, up, ap, 0, op, s),
                       lambda: lib.pf_gl_sens(P, record(d0=None), up, ap, 0, op, s)],
        "pf_group_sum_f64": [lambda: lib.pf_group_sum_f64(-1, op, ep, pp, ip, 2, gp, s),
                             lambda: lib.pf_group_sum_f64(S.ne, None, ep, pp, ip, 2, gp, s),
                             lambda: lib.pf_group_sum_f64(S.ne, op, ep, None, ip, 2, gp, s),
                             lambda: lib.pf_group_sum_f64(S.ne, op, ep, pp, None, 2, gp, s),
                             lambda: lib.pf_group_sum_f64(S.ne, op, ep, pp, ip, -1, gp, s),
                             lambda: lib.pf_group_sum_f64(S.ne, op, ep, pp, ip, 2, None, s)],
    }
    for name, group in calls.items():
        for i, call in enumerate(group):
            assert call() == capi.PF_ERR_ARG, (name, i)
            assert lib.pf_last_error().decode().startswith(name + ":"), (name, i, lib.pf_last_error())
    torch.cuda.synchronize()
    for t in (S.kt, S.fe, S.strain, out, gout):                          # nothing was enqueued
        assert bool((t == 7.0).all())
    # the engine never makes the scalar call when it is given an ea, and checks its length
    with pytest.raises(ValueError, match="ea has"):
        eng.gl_state(u, ea[:-1])
    with pytest.raises(ValueError, match="gl_sensitivity"):
        eng.gl_sensitivity(u, a, out=out[:-1])
    assert lib.pf_group_sum_f64(S.ne, op, None, pp, ip, 0, gp, s) == capi.PF_OK      # no groups: nothing to do


# ---------------------------------------------------------------------------------------------------------------------
# 5, 6. misfit_and_gradient, identify_nr and the CLI on the 8-panel Warren cantilever
# ---------------------------------------------------------------------------------------------------------------------
def test_misfit_and_gradient_against_the_reference():
    """J and dJ/dq at all factors 1, with both preconditioners.  Allowed distance: ten times the distance the restatement
    itself shows between its direct-solve result and its own result with gl.jacobi_cg at rtol 1e-13, both computed here."""
    from pinn_fem_amd.engine import HipEngine
    from pinn_fem_amd.fem.identify import misfit_and_gradient
    case = ir.warren_case(8)
    q = np.zeros(4)
    J_ref, g_ref = case.objective(q)
    its_ref = ir.misfit_and_gradient(case.nodes, case.el, case.loads, case.fixed, case.ea(q), 2, case.levels)[3]
    J_cg, g_cg = case.objective(q, linear_solve=gl.jacobi_cg(1e-13))
    tol_J, tol_g = 10 * abs(J_cg - J_ref), 10 * np.max(np.abs(g_cg - g_ref))
    print(f"reference: J = {J_ref:.15e}, Newton iterations {its_ref}, direct against CG {abs(J_cg - J_ref):.2e} (J), {np.max(np.abs(g_cg - g_ref)):.2e} (dJ/dq)")
    model = case_model(case)
    ea = case.ea(q)
    got = {}
    for pre in ("jacobi", "two-level-updated"):
        J, g_ea, states, counters = misfit_and_gradient(model, gl_config(nr_preconditioner=pre), case.levels, ea)
        eng = model._pf_engine_cache[1]
        assert isinstance(eng, HipEngine) and g_ea.is_cuda and g_ea.dtype == torch.float64 and len(states) == 3
        g = eng.group_sum(g_ea, torch.from_numpy(ea).to(eng.device), case.groups).cpu().numpy()
        got[pre] = (J, g)
        print(f"{pre}: J - J_ref = {J - J_ref:.2e} (allowed {tol_J:.2e}), dJ/dq distance {np.max(np.abs(g - g_ref)):.2e} "
              f"(allowed {tol_g:.2e}), counters {counters}")
        assert counters["newton_iterations"] == sum(its_ref) and counters["adjoint_cg_iterations"] > 0   # the CPU loop's
    for pre, (J, g) in got.items():
        assert abs(J - J_ref) <= tol_J, pre
        assert np.max(np.abs(g - g_ref)) <= tol_g, pre
    (Ja, ga), (Jb, gb) = got.values()
    print(f"jacobi against two-level-updated: {abs(Ja - Jb):.2e} (J), {np.max(np.abs(ga - gb)):.2e} (dJ/dq)")
    assert abs(Ja - Jb) <= tol_J and np.max(np.abs(ga - gb)) <= tol_g


def test_identify_nr_recovers_the_four_factors():
    """From all factors 1 to within 1e-5 of (1.0, 0.7, 1.3, 0.85) in at most 1.5 times the evaluations the restatement's
    own optimisation takes (recomputed here; the half allows for CG-solved states steering the line search differently)."""
    from pinn_fem_amd.fem import identify_nr
    case, ref_factors, ref_evaluations = ir.reference_recovery(8)
    cap = int(1.5 * ref_evaluations)
    res = identify_nr(case_model(case), gl_config(), case.levels, groups=case.groups, max_evaluations=cap, gtol=1e-14)
    err = np.max(np.abs(res.factors - case.factors))
    print(f"identify_nr: factors {res.factors}, error {err:.2e}, {res.evaluations} evaluations (reference {ref_evaluations}, "
          f"cap {cap}), misfit {res.misfit:.2e}, converged {res.converged}, counters {res.counters}")
    assert err <= 1e-5 and res.evaluations <= cap
    assert len(res.history) == res.evaluations and res.history[0]["misfit"] > 1e-4 > res.misfit
    assert np.allclose(res.ea, 1000.0 * res.factors[case.groups], rtol=1e-15)
    assert len(res.displacements) == 3 and res.reactions.shape == (34,) and not res.reactions[4:].any()
    # the last level's displacements at the identified factors are the measured ones
    dofs, u_meas = case.levels[-1][1], case.levels[-1][2]
    assert np.max(np.abs(res.displacements[-1][dofs] - u_meas)) <= 1e-5 * np.max(np.abs(u_meas))
    assert abs(res.reactions[1] + res.reactions[3] + case.loads[case.tip]) <= 1e-9 * abs(case.loads[case.tip])


def test_identify_nr_evaluation_cap_and_per_element_parameters():
    from pinn_fem_amd.fem import identify_nr
    case = ir.warren_case(8)
    res = identify_nr(case_model(case), gl_config(), case.levels, groups=None, max_evaluations=3)
    print(f"per element, 3 evaluations: misfit {[h['misfit'] for h in res.history]}")
    assert res.evaluations == 3 and not res.converged and res.factors.shape == (31,) and res.gradient.shape == (31,)
    assert res.misfit == min(h["misfit"] for h in res.history) < res.history[0]["misfit"]


def test_cli_identify(tmp_path):
    case, _, ref_evaluations = ir.reference_recovery(8)
    out = run_cli(tmp_path, "warren_identify", "warren")
    factors = np.array(out["identified_factors"])
    print(f"CLI: factors {factors}, {out['evaluations']} evaluations, misfit {out['misfit']:.2e}")
    assert np.max(np.abs(factors - case.factors)) <= 1e-5 and out["evaluations"] <= int(1.5 * ref_evaluations)
    assert np.allclose(out["identified_ea"], 1000.0 * factors[case.groups], rtol=1e-15)
    assert len(out["displacements"]) == 34 and len(out["reactions"]) == 34 and out["misfit"] < 1e-10
    assert len(out["history"]) == out["evaluations"] == out["iterations"]


# ---------------------------------------------------------------------------------------------------------------------
# 7, 8. the two-bar truss
# ---------------------------------------------------------------------------------------------------------------------
def test_two_bar_closed_form_on_the_device():
    """dJ/d(ea) = 2 (w - w_bar) (-P / (ea tangent(w))) at half the limit load.  Bound: ir.two_bar_bound (the Newton
    tolerance) plus 1e-9 for the CG solves, as tests/test_gl_f64.py allows them on this truss (rtol 1e-13 times the
    condition number of these states, 150 .. 360, times ~30)."""
    from pinn_fem_amd.fem.identify import misfit_and_gradient
    tb = gl.TwoBar(ea=EA)
    p, tol = 0.5 * tb.p_lim, 1e-10
    w_ref = -gl.newton(tb.nodes, tb.el, tb.loads(p), tb.fixed, EA, 2, tol=tol)[0][5]
    w_bar = 0.9 * w_ref
    model = truss_model(tb.nodes, tb.el, tb.loads(p), tb.fixed)
    J, g, states, _ = misfit_and_gradient(model, gl_config(), [(1.0, [5], [-w_bar])], np.full(2, EA))
    w = -float(states[0][5])
    g = g.cpu().numpy()
    want = ir.two_bar_closed_form(tb, p, w, w_bar)
    rel, bound = abs(g.sum() - want) / abs(want), ir.two_bar_bound(tb, w, w_bar, tol) + 1e-9
    print(f"two-bar on the device: w = {w:.12f} (CPU {w_ref:.12f}), dJ/d(ea) = {g.sum():.12e} (closed form {want:.12e}), "
          f"relative {rel:.2e}, bound {bound:.2e}")
    assert abs(J - (w - w_bar) ** 2) <= 1e-14 * J and abs(g[0] - g[1]) <= 1e-12 * abs(g[0])
    assert rel <= bound


def test_a_level_beyond_the_limit_point_is_refused():
    """Levels at 0.5 and 2.0 of the limit load: from the first level's state (w = 0.115) the first Newton step of the
    second lands at w = 0.544, past the limit point (0.423), where the vertical tangent is -0.37: the CPU loop sees it
    in its second iterate (checked here), and the device's rule rhs.du > 0 refuses it."""
    from pinn_fem_amd.fem import identify_nr
    from pinn_fem_amd.fem.identify import misfit_and_gradient
    tb = gl.TwoBar(ea=EA)
    u0 = gl.newton(tb.nodes, tb.el, tb.loads(0.5 * tb.p_lim), tb.fixed, EA, 2)[0]
    eigs = []
    gl.newton(tb.nodes, tb.el, tb.loads(2.0 * tb.p_lim), tb.fixed, EA, 2, u0=u0, max_iter=2,
              on_iterate=lambda u, K, free, rhs: eigs.append(gl.min_eig_ff(K, free)))
    assert eigs[0] > 1.0 and eigs[1] < -0.3
    model = truss_model(tb.nodes, tb.el, tb.loads(tb.p_lim), tb.fixed)
    levels = [(0.5, [5], [u0[5]]), (2.0, [5], [-0.5])]
    with pytest.raises(RuntimeError, match="not positive definite"):
        misfit_and_gradient(model, gl_config(), levels, np.full(2, EA))
    with pytest.raises(RuntimeError, match="not positive definite"):
        identify_nr(model, gl_config(), levels, groups=[0, 0])
