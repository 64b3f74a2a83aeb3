"""Several right-hand sides per launch in the tangent CG solve: pf_pcgtm_* and pf_pcg2tm_* against the single families
pf_pcgt_* and pf_pcg2t_*, bit for bit, and the engine's extra_fixed view.

The system is a 1000-element irregular planar truss (400 nodes: two node blocks, four vector blocks per right-hand side)
at a stretched state whose tangent is positive definite (eigenvalues of K_ff in [21.4, 7831] on the CPU), with a dense
right-hand side and a unit one: scipy's Jacobi-CG takes 152 and 161 iterations for them, so one stops while the other
goes on.  A 5-element chain covers DIM = 1."""
import ctypes as C
import math

import numpy as np
import pytest
import scipy.sparse.linalg as spla
import torch

import gl_reference as gl
from device_driver import AREA, EA, RTOL, YOUNG, CgRun, DeviceTruss, irregular_truss_with_supports, same_bits, system_cache

pytestmark = pytest.mark.gpu


class System(DeviceTruss):
    """One truss on the device at a Green-Lagrange state u: the tangent blocks are the engine's (eng.gl_state)."""

    def __init__(self, nodes, el, fixed, dim, u):
        super().__init__(nodes, el, fixed, dim, YOUNG, AREA)
        self.u = np.asarray(u, dtype=np.float64)
        self.K = gl.k_t(self.nodes, self.el, self.u, EA, dim)
        self.eng.gl_state(self.dev(self.u))
        torch.cuda.synchronize()
        self.kt = self.eng._gl[1]

    def coarse(self, n_agg):
        return self.eng.updated_coarse_space(self.dev(self.u), n_agg)


def _truss_1000():
    nodes, el, fixed = irregular_truss_with_supports(1000, np.random.default_rng(2000))
    rng = np.random.default_rng(11)
    mean_l0 = float(np.mean(np.linalg.norm(nodes[el[:, 1]] - nodes[el[:, 0]], axis=1)))
    u = 0.05 * nodes.reshape(-1) + 0.02 * (0.3 * mean_l0 / math.sqrt(4.0)) * rng.standard_normal(nodes.size)
    S = System(nodes, el, fixed, 2, u)
    assert len(S.nodes) == 400
    lam = np.linalg.eigvalsh(gl.restrict(S.K, S.free).toarray())
    print(f"truss: eigenvalues of K_t,ff in [{lam[0]:.3e}, {lam[-1]:.3e}]")
    assert lam[0] > 0.0
    xs = np.where(S.free, rng.standard_normal(S.n), 0.0)
    S.b_dense = np.where(S.free, S.K @ xs, 0.0)
    S.b_unit = np.zeros(S.n)
    S.b_unit[np.flatnonzero(S.free)[3]] = 1.0
    S.n_agg = 8
    return S


def _chain_5():
    x = np.array([0.0, 0.7, 1.6, 2.1, 3.0, 3.8])
    el = np.array([[0, 1], [2, 1], [2, 3], [4, 3], [4, 5]])
    u = 0.05 * x + 0.01 * np.array([0.0, 0.3, -0.2, 0.5, 0.1, -0.4])
    S = System(x, el, np.array([0]), 1, u)
    assert np.linalg.eigvalsh(gl.restrict(S.K, S.free).toarray())[0] > 0.0
    S.b_dense = np.where(S.free, S.K @ np.array([0.0, 1.0, -2.0, 0.5, 3.0, -1.0]), 0.0)
    # the second right-hand side is mu D v for an eigenpair of D^-1 K_ff: Jacobi-CG ends after one iteration
    idx = np.flatnonzero(S.free)
    Kff = gl.restrict(S.K, S.free).toarray()
    d = np.sqrt(np.diag(Kff))
    w = np.linalg.eigh(Kff / np.outer(d, d))[1][:, 0]
    S.b_unit = np.zeros(S.n)
    S.b_unit[idx] = Kff @ (w / d)
    S.n_agg = 2
    return S


@pytest.fixture(scope="module")
def systems():
    yield from system_cache(lambda name: {"truss": _truss_1000, "chain": _chain_5}[name]())


def _run(S, B, dc=None, batched=True):
    """a tangent family on the engine's kt: pf_pcgtm_* / pf_pcg2tm_* with m = len(B), or the single family (B one row)"""
    return CgRun(S, B, kt=S.kt.data_ptr(), dc=dc, batched=batched)


def _dc(S, two_level):
    return S.coarse(S.n_agg) if two_level else None


# ---- 4. m = 1 is the single family --------------------------------------------------------------------------------------
@pytest.mark.parametrize("two_level", [False, True], ids=["jacobi", "two-level"])
def test_one_right_hand_side_equals_the_single_family_bitwise(systems, two_level):
    S = systems("truss")
    dc = _dc(S, two_level)
    assert dc is not None or not two_level
    one, many = _run(S, S.b_dense, dc, batched=False), _run(S, S.b_dense, dc, batched=True)
    assert one.stride == many.stride
    done = 0
    for upto in (0, 7, 200):
        st1, stm = one.iterate(upto - done), many.iterate(upto - done)
        done = upto
        assert [st1] == stm, upto
        assert same_bits(one.read(), many.read()[0]), upto
    assert st1[1] == 1.0 and 16 < st1[0] < 200                        # it stopped on its own, inside the last call
    assert [one.state()] == many.state() == [st1]


# ---- 5. m = 2 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("two_level", [False, True], ids=["jacobi", "two-level"])
@pytest.mark.parametrize("name", ["truss", "chain"])
def test_two_right_hand_sides_equal_their_single_solves_bitwise(systems, name, two_level):
    S = systems(name)
    dc = _dc(S, two_level)
    assert dc is not None or not two_level
    B = np.stack([S.b_dense, S.b_unit])
    singles = [_run(S, B[k], dc, batched=False) for k in range(2)]
    pair = _run(S, B, dc)

    def check(label):
        st = pair.state()
        got = pair.read()
        for k in range(2):
            assert singles[k].state() == st[k], (label, k)
            assert same_bits(singles[k].read(), got[k]), (label, k)
        return st, got

    check("begin")
    # the iteration counts, from a probe of each
    T = []
    for k in range(2):
        probe = _run(S, B[k], dc, batched=False)
        st = probe.iterate(4000)
        assert st[1] == 1.0
        T.append(int(st[0]))
    print(f"{name}, {'two-level' if two_level else 'jacobi'}: iterations {T}")
    if name == "truss":
        assert T[0] != T[1], T                                          # 152 and 161 on the CPU
    first, last = (0, 1) if T[0] <= T[1] else (1, 0)
    # polls of 8 iterations up to the last one before the first stop, then exactly to it
    done, per = 0, 8 if name == "truss" else 1
    while done + per < T[first]:
        for r in singles + [pair]:
            r.iterate(per)
        done += per
        check(f"after {done}")
    for r in singles + [pair]:
        r.iterate(T[first] - done)
    st, got = check("first stop")
    assert st[first][:2] == (float(T[first]), 1.0)
    assert st[last][:2] == (float(T[first]), 1.0 if T[last] == T[first] else 0.0)
    # the second goes on; the part of the first no longer changes
    for r in singles + [pair]:
        r.iterate(T[last] - T[first])
    st2, got2 = check("second stop")
    assert st2[first] == st[first] and same_bits(got2[first], got[first])
    assert st2[last][:2] == (float(T[last]), 1.0) and (T[last] == T[first] or not same_bits(got2[last], got[last]))
    # both stopped: further launches change nothing
    assert pair.iterate(10) == st2
    assert all(same_bits(a, b) for a, b in zip(pair.read(), got2))


@pytest.mark.parametrize("two_level", [False, True], ids=["jacobi", "two-level"])
@pytest.mark.parametrize("name", ["truss", "chain"])
def test_batched_graph_of_64_equals_eager_bitwise(systems, name, two_level):
    S = systems(name)
    dc = _dc(S, two_level)
    B = np.stack([S.b_dense, S.b_unit])
    eager, graphed = _run(S, B, dc), _run(S, B, dc)
    g = graphed.graph(64)
    try:
        for i in range(4):
            st_g, st_e = graphed.replay(g), eager.iterate(64)
            assert st_g == st_e, i
            assert all(same_bits(a, b) for a, b in zip(graphed.read(), eager.read())), i
            if all(s[1] == 1.0 for s in st_g):
                break
        assert all(s[1] == 1.0 for s in st_g), st_g
        after = graphed.read()
        assert graphed.replay(g) == st_g                                # after the stop a replay is a no-op
        assert all(same_bits(a, b) for a, b in zip(graphed.read(), after))
    finally:
        S.lib.pf_graph_destroy(g)


@pytest.mark.parametrize("two_level", [False, True], ids=["jacobi", "two-level"])
@pytest.mark.parametrize("name", ["truss", "chain"])
def test_zero_right_hand_side_is_done_at_begin(systems, name, two_level):
    S = systems(name)
    dc = _dc(S, two_level)
    B = np.stack([S.b_dense, np.zeros(S.n)])
    single, pair = _run(S, B[0], dc, batched=False), _run(S, B, dc)
    assert pair.state()[1] == (0.0, 1.0, 0.0, 0.0) and pair.state()[0][:2] == (0.0, 0.0)
    st1, st = single.iterate(4000), pair.iterate(4000)
    assert st[0] == st1 and st1[1] == 1.0 and st[1] == (0.0, 1.0, 0.0, 0.0)
    got = pair.read()
    assert same_bits(single.read(), got[0]) and not got[1][0].any()


# ---- 6. argument errors -------------------------------------------------------------------------------------------------
def test_argument_errors(systems):
    S = systems("truss")
    eng, lib, capi = S.eng, S.lib, S.capi
    dc = S.coarse(S.n_agg)
    n2 = int(lib.pf_pcg2_workspace_count(eng._ref()))
    b = S.dev(np.concatenate([S.b_dense, S.b_unit, S.b_unit]))
    x = torch.full((3 * S.n,), 7.0, dtype=torch.float64, device=eng.device)
    ws = torch.full((3 * n2,), 7.0, dtype=torch.float64, device=eng.device)
    st, g, s, P = (C.c_double * 12)(), C.c_void_p(), eng._stream(), eng._ref()
    kt, bp, xp, wp, cc = S.kt.data_ptr(), b.data_ptr(), x.data_ptr(), ws.data_ptr(), C.byref(dc.record)
    jac = {
        "pf_pcgtm_begin": lambda k, m: lib.pf_pcgtm_begin(P, k, m, bp, xp, wp, RTOL, s),
        "pf_pcgtm_iterations": lambda k, m: lib.pf_pcgtm_iterations(P, k, m, xp, wp, 1, st, s),
        "pf_pcgtm_graph_create": lambda k, m: lib.pf_pcgtm_graph_create(P, k, m, xp, wp, 4, s, C.byref(g)),
        "pf_pcgtm_state": lambda k, m: lib.pf_pcgtm_state(P, k, m, wp, st, s),
    }
    two = {
        "pf_pcg2tm_begin": lambda c, k, m: lib.pf_pcg2tm_begin(P, c, k, m, bp, xp, wp, RTOL, s),
        "pf_pcg2tm_iterations": lambda c, k, m: lib.pf_pcg2tm_iterations(P, c, k, m, xp, wp, 1, st, s),
        "pf_pcg2tm_graph_create": lambda c, k, m: lib.pf_pcg2tm_graph_create(P, c, k, m, xp, wp, 4, s, C.byref(g)),
    }
    with eng.on_stream():
        for name, call in jac.items():
            for args in ((kt, 0), (kt, 3), (None, 2)):
                assert call(*args) == capi.PF_ERR_ARG, (name, args)
                assert lib.pf_last_error().decode().startswith(name + ":"), name
        for name, call in two.items():
            for args in ((cc, kt, 0), (cc, kt, 3), (cc, None, 2), (None, kt, 2)):
                assert call(*args) == capi.PF_ERR_ARG, (name, args)
                assert lib.pf_last_error().decode().startswith(name + ":"), name
        for args in ((kt, 0), (kt, 3), (None, 2)):
            assert lib.pf_pcg2tm_state(P, *args, wp, st, s) == capi.PF_ERR_ARG
            assert lib.pf_last_error().decode().startswith("pf_pcg2tm_state:")
    assert not g.value
    torch.cuda.synchronize()
    assert bool((x == 7.0).all()) and bool((ws == 7.0).all())          # nothing was enqueued
    with pytest.raises(ValueError, match="pcg_solve_batch"):
        eng.pcg_solve_batch(b.reshape(3, -1))
    with pytest.raises(ValueError, match="tangent"):
        eng.pcg_solve_batch(b.reshape(3, -1)[:2], tangent=False)


# ---- the engine's batched solve ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pre", ["jacobi", "two-level-updated"])
def test_pcg_solve_batch_equals_two_pcg_solves(systems, pre):
    S = systems("truss")
    eng = S.eng
    kw = dict(tangent=True, preconditioner=pre, n_aggregates=S.n_agg, u=S.dev(S.u), rtol=RTOL)
    singles = [eng.pcg_solve(S.dev(b), **kw) for b in (S.b_dense, S.b_unit)]
    before, batches = eng.pcg_iterations, eng.pcg_batch_solves
    X, reports = eng.pcg_solve_batch(S.dev(np.stack([S.b_dense, S.b_unit])), **kw)
    torch.cuda.synchronize()
    assert eng.pcg_batch_solves == batches + 1
    assert eng.pcg_iterations - before == sum(r[0] for r in reports)
    for k in range(2):
        assert reports[k] == singles[k][1:], k
        assert reports[k][1] and reports[k][0] > 16
        assert X[k].cpu().numpy().tobytes() == singles[k][0].cpu().numpy().tobytes(), k
    assert reports[0][0] != reports[1][0]


# ---- 7. extra_fixed -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pre", ["jacobi", "two-level-updated"])
def test_extra_fixed_solves_the_smaller_system(systems, pre):
    """pcg_solve(tangent=True, extra_fixed=[c]) against a sparse direct solve with K' = K_t without row and column c.
    Tolerance as in test_pcgt_solves_the_tangent_system: the distance at which scipy's Jacobi-CG (same rtol) ends, times
    its margin 10."""
    S = systems("truss")
    eng = S.eng
    c = int(np.flatnonzero(S.free)[100])
    fc = S.free.copy()
    fc[c] = False
    idx = np.flatnonzero(fc)
    Kp = gl.restrict(S.K, fc)
    b = np.where(S.free, S.b_dense, 0.0)                                # non-zero at c: the solve must ignore it
    assert b[c] != 0.0
    direct = np.zeros(S.n)
    direct[idx] = spla.spsolve(Kp, b[idx])
    y = np.zeros(S.n)
    y[idx] = gl.jacobi_cg(RTOL)(Kp, b[idx])
    scale = np.max(np.abs(direct))
    err_ref = np.max(np.abs(y - direct)) / scale
    flags_before = eng.dof_flags.cpu().numpy().copy()
    ptr_before = eng.P.mesh.dof_flags
    kw = dict(tangent=True, preconditioner=pre, n_aggregates=S.n_agg, u=S.dev(S.u), rtol=RTOL)
    plain_before = eng.pcg_solve(S.dev(b), **kw)
    x, it, ok, rr, bb = eng.pcg_solve(S.dev(b), extra_fixed=[c], **kw)
    plain_after = eng.pcg_solve(S.dev(b), **kw)
    torch.cuda.synchronize()
    x = x.cpu().numpy()
    err = np.max(np.abs(x - direct)) / scale
    print(f"extra_fixed, {pre}: scipy CG error {err_ref:.2e} | device {it} iterations, error {err:.2e}")
    assert ok and x[c] == 0.0 and np.all(x[~S.free] == 0.0)
    assert abs(bb - float(b[idx] @ b[idx])) <= 1e-12 * bb              # |b|^2 without the entry at c
    assert err <= 10 * err_ref
    assert np.array_equal(eng.dof_flags.cpu().numpy(), flags_before) and eng.P.mesh.dof_flags == ptr_before
    assert np.array_equal(eng.plan.dof_flags, flags_before)
    assert plain_after[1:] == plain_before[1:]
    assert plain_after[0].cpu().numpy().tobytes() == plain_before[0].cpu().numpy().tobytes()
    assert plain_before[0].cpu().numpy()[c] != 0.0
    # K_t v with the same view: the row of c is zeroed as well
    v = S.dev(S.b_dense)
    kv = eng.kt_v_f64(v, zero_fixed=True, extra_fixed=[c]).cpu().numpy()
    kv_plain = eng.kt_v_f64(v, zero_fixed=True).cpu().numpy()
    assert kv[c] == 0.0 and kv_plain[c] != 0.0 and np.array_equal(np.delete(kv, c), np.delete(kv_plain, c))
