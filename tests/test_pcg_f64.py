"""The float64 K v and Jacobi-PCG kernels (pinn_fem_amd/csrc/pf_pcg.hip) called directly through the C ABI and
held against the CPU float64 reference of tests/f64_reference.py (itself verified by tests/test_f64_reference.py),
at the sizes where both grid-stride loops run (node kernels from 262 145 nodes, vector kernels from 1 048 577 dofs).

Every bound below is either derived from 2^-53 / 2^-24 and operation counts in a comment at the assertion, or a
stated multiple of what the CPU reference alone achieves on the same system; the measured figures are printed.
"""
import ctypes as C
import math

import numpy as np
import pytest
import scipy.sparse.linalg as spla
import torch

import f64_reference as ref
from device_driver import RTOL, U24, U53, CgRun, bar1d, hub_truss, manufactured, same_bits, system_cache, wide_vector
from device_driver import LinearTruss as System

pytestmark = pytest.mark.gpu



def _mask_of(n, fixed):
    m = np.zeros(n, dtype=bool)
    m[np.asarray(fixed, dtype=int)] = True
    return m


def _chain2d(n_nodes, rng):
    """2-D chain of n_nodes with jittered (inclined) members, random orientation; node 0 and some other dofs fixed."""
    x = np.concatenate([[0.0], np.cumsum(0.5 + rng.random(n_nodes - 1))])
    nodes = np.stack([x, rng.uniform(-0.5, 0.5, n_nodes)], axis=1)
    e = np.arange(n_nodes - 1)
    el = np.stack([e, e + 1], axis=1)
    flip = rng.random(len(el)) < 0.5
    el[flip] = el[flip][:, ::-1]
    fixed = np.unique(np.concatenate([[0, 1], rng.choice(2 * n_nodes, size=max(1, n_nodes // 9), replace=False)]))
    return nodes, el, fixed


def _make(name):
    if name.startswith("grid"):
        side = int(name.split("_")[0][4:])
        nets = {"scalar": (None, None), "EA": (20, 15), "E": (20, None)}[name.split("_")[1]]
        nodes, el, fixed = ref.pinned_grid_truss(side, np.random.default_rng(side))
        return System(nodes, el, fixed, 2, 2.0, 0.5, nets)
    if name.startswith("hub"):
        nets = {"scalar": (None, None), "E": (20, None)}[name.split("_")[1]]
        return System(*hub_truss(np.random.default_rng(2500)), 2, 2.0, 0.5, nets)
    if name == "bar300k":
        x, el, fixed = ref.pinned_bar(300_000, np.random.default_rng(64))
        return System(x, el, fixed, 1, 3.0, 0.25)
    raise KeyError(name)


@pytest.fixture(scope="module")
def systems():
    """Every larger system is built once per module (the CPU matrices at side 750 cost some 20 s each)."""
    yield from system_cache(_make)


# ---------------------------------------------------------------------------------------------------------------------
# A. pf_kv_f64 against the CSR product
# ---------------------------------------------------------------------------------------------------------------------
def _check_kv(S, rng, symmetry=False):
    v = wide_vector(rng, S.n)
    got, got_zf = S.kv(v, False), S.kv(v, True)
    assert np.all(np.isfinite(got))
    want, scale = S.K @ v, S.Kabs @ np.abs(v)
    # float64 round-off per incidence, in units of 2^-53 of |ke||v_e|: s = (E*A)/l0 two roundings, dx and dy one
    # each, the bracket c2*dx + cs*dy three, the product with s one; one more per accumulated incidence -> 8 + degree;
    # doubled because the CPU product rounds as well.  A float32 slip anywhere is 2^29 times larger.
    bound = (16 + 2 * S.max_degree) * U53 * scale
    err = np.abs(got - want)
    worst = float(np.max(err / np.maximum(scale, 1e-300))) / U53
    print(f"kv f64: n_dofs {S.n}, max degree {S.max_degree}, worst error {worst:.2f} * 2^-53 |K||v| "
          f"(bound {16 + 2 * S.max_degree})")
    assert np.all(err <= bound)
    # against the float64 coordinates: c2, cs (or cs, s2) and l0 are float32 roundings of the float64 values, three
    # relative errors of 2^-24 per term (four allowed), plus the float64 round-off above
    K64, Kabs64 = S.from_f64_coordinates()
    scale64 = Kabs64 @ np.abs(v)
    err64 = np.abs(got - K64 @ v)
    print(f"        vs float64 coordinates: worst {float(np.max(err64 / np.maximum(scale64, 1e-300))) / U24:.3f} * 2^-24 |K||v|")
    assert np.all(err64 <= 4 * U24 * scale64 + bound)
    # zero_fixed: fixed rows exactly 0.0, every other row the same bits
    assert np.all(got_zf[S.mask] == 0.0) and not np.any(np.signbit(got_zf[S.mask]))
    assert np.array_equal(got_zf[~S.mask].view(np.uint64), got[~S.mask].view(np.uint64))
    if symmetry:
        w = wide_vector(rng, S.n)
        kw = S.kv(w, False)
        lhs, rhs = math.fsum(w * got), math.fsum(v * kw)                  # one rounding per product, exact sums
        unit = math.fsum(np.abs(w) * scale)
        # each (K v)_i is off by <= (8 + degree) 2^-53 (|K||v|)_i, degree 8 here: 16 per side, 32 for both, one more
        # per side for the products of the dot
        print(f"        symmetry: |<w,Kv> - <v,Kw>| = {abs(lhs - rhs) / unit / U53:.3e} * 2^-53 <|w|,|K||v|> (bound 64)")
        assert abs(lhs - rhs) <= 64 * U53 * unit


@pytest.mark.parametrize("n_nodes", [2, 255, 256, 257, 262_144, 262_145, 600_000])
def test_kv_f64_chain_2d(n_nodes):
    """Chains across the wave / block edges and both sides of the node kernels' grid-stride threshold
    (1024 blocks * 256 threads = 262 144 nodes)."""
    rng = np.random.default_rng(n_nodes)
    _check_kv(System(*_chain2d(n_nodes, rng), 2), rng)


@pytest.mark.parametrize("n_nodes", [2, 257, 262_145])
def test_kv_f64_bar_1d(n_nodes):
    rng = np.random.default_rng(n_nodes + 1)
    _check_kv(System(*bar1d(n_nodes, rng), 1), rng)


def test_kv_f64_hub_truss(systems):
    """Node degree 300, shuffled element order, random element orientation."""
    S = systems("hub_scalar")
    assert S.max_degree >= 300
    _check_kv(S, np.random.default_rng(1))


def test_kv_f64_pinned_grid_750(systems):
    """562 500 nodes: the node kernels stride (2.15 nodes per thread); symmetry of the operator."""
    S = systems("grid750_scalar")
    assert S.n_nodes > 262_144 * 2 and S.n > 1_048_576
    _check_kv(S, np.random.default_rng(2), symmetry=True)


@pytest.mark.parametrize("name", ["grid750_EA", "hub_E"])
def test_kv_f64_net_properties(systems, name):
    """The net-enabled branch of elem_s64: E (and A) per element from prop_e / prop_a."""
    S = systems(name)
    assert np.ptp(S.E) > 0.01 * np.mean(S.E)                      # the property really varies over the mesh
    _check_kv(S, np.random.default_rng(3))


# ---------------------------------------------------------------------------------------------------------------------
# B. state of a running solve
# ---------------------------------------------------------------------------------------------------------------------
def _check_invariants(S, run, b, asked, st):
    x, w = run.read()[0], run.parts()
    free, fixed = ~S.mask, S.mask
    bf = np.where(fixed, 0.0, b)
    # dinv = 1 / diag(K_ff): the diagonal is the same sum of the same products in the same (element) order, and the
    # division rounds once: 4 ulp (the issue's figure) leaves room for a contracted multiply-add
    want = S.dinv
    assert np.all(np.abs(w["dinv"][free] - want[free]) <= 4 * np.spacing(want[free]))
    assert np.all(w["dinv"][fixed] == 0.0)
    names = ("r", "z", "p") + (("ap",) if asked > 0 else ())         # ap is first written by iteration 1
    for name in names:
        assert np.all(w[name][fixed] == 0.0), name
        assert np.all(np.isfinite(w[name])), name
    assert np.all(x[fixed] == 0.0) and np.all(np.isfinite(x))
    assert np.array_equal(w["z"], w["dinv"] * w["r"])                # z == dinv * r, bit for bit
    # the |r|^2 and |b|^2 the host reads: block sums in another order than fsum, 1e-13 relative
    rr, bb = math.fsum(w["r"] * w["r"]), math.fsum(bf * bf)
    assert abs(st[2] - rr) <= 1e-13 * rr and abs(st[3] - bb) <= 1e-13 * bb
    assert (st[2], st[3]) == (w["state"][2], w["state"][3]) == run.state()[2:]      # ST_RR, ST_BB
    # recurrence residual against the true one
    drift = np.linalg.norm(w["r"] - (bf - S.Kff @ x)) / np.linalg.norm(bf)
    assert drift <= 1e-12
    if not st[1]:
        assert st[0] == asked
    else:
        assert st[0] <= asked
    return x, st[2], drift


@pytest.mark.parametrize("name", ["grid100_scalar", "hub_scalar", "grid750_scalar"])
def test_pcg_running_state(systems, name):
    """Workspace invariants after pf_pcg_begin and after 1, 2, 5, 20 and 64 iterations, and the trajectory
    against pcg_reference.  CG amplifies rounding differences, so the trajectory's unit is measured on the
    reference alone: the same recurrence with the dofs permuted (another summation order).  The device must stay
    within 10 units + 1e-14.  Measured at k = 64, where the spread is largest (unit of x, of |r|^2 | device x, |r|^2):
      grid100_scalar  2.11e-13  5.51e-12 | 5.82e-13  1.52e-11
      hub_scalar      3.32e-15  4.53e-14 | 2.56e-14  4.58e-13   (|r|^2: 10.1 units, inside only with the floor)
      grid750_scalar  1.13e-12  1.05e-12 | 1.72e-12  1.61e-12
    At k <= 20 everything is below 4e-15; the residual drift |r - (b - K x)| / |b| stays below 5e-16."""
    S = systems(name)
    rng = np.random.default_rng(5)
    xs, b = manufactured(S, rng)
    b_dirty = b + np.where(S.mask, 3.0, 0.0)                          # entries on fixed dofs are ignored
    ks = (1, 2, 5, 20, 64)
    _, _, _, _, _, snaps = ref.pcg_reference(S.Kff, S.dinv, b, RTOL, 64, snapshots=ks)
    perm = rng.permutation(S.n)
    Kp = S.Kff[perm][:, perm].tocsr()
    _, _, _, _, _, snaps_p = ref.pcg_reference(Kp, S.dinv[perm], b[perm], RTOL, 64, snapshots=ks)
    run = CgRun(S, b_dirty)
    _check_invariants(S, run, b_dirty, 0, run.state())
    x0, w0 = run.read()[0], run.parts()
    assert not x0.any() and np.array_equal(w0["r"], b) and np.array_equal(w0["p"], w0["z"])
    assert tuple(w0["state"][[7, 6]]) == (0.0, 0.0) and w0["state"][8] == RTOL * RTOL   # ITERS, DONE, RTOL2
    done = 0
    for k in ks:
        st = run.iterate(k - done)
        done = k
        x, rr, drift = _check_invariants(S, run, b_dirty, k, st)
        xr, rr_r = snaps[k]
        xp, rr_p = snaps_p[k]
        back = np.empty_like(xp)
        back[perm] = xp
        unit_x = np.max(np.abs(xr - back)) / np.max(np.abs(xr))
        unit_r = abs(rr_r - rr_p) / rr_r
        dev_x = np.max(np.abs(x - xr)) / np.max(np.abs(xr))
        dev_r = abs(rr - rr_r) / rr_r
        print(f"{name} k={k:2d}: reference unit x {unit_x:.2e} rr {unit_r:.2e} | device x {dev_x:.2e} rr {dev_r:.2e}"
              f" | residual drift {drift:.2e}")
        assert dev_x <= 10 * unit_x + 1e-14
        assert dev_r <= 10 * unit_r + 1e-14


# ---------------------------------------------------------------------------------------------------------------------
# C. solve to convergence, both stride paths
# ---------------------------------------------------------------------------------------------------------------------
def _scipy_cg(S, b, maxiter):
    n_it = [0]
    dinv = S.dinv
    M = spla.LinearOperator((S.n, S.n), matvec=lambda v: dinv * v, dtype=np.float64)
    y, info = spla.cg(S.Kff, b, rtol=RTOL, atol=0.0, maxiter=maxiter, M=M,
                      callback=lambda _: n_it.__setitem__(0, n_it[0] + 1))
    return y, n_it[0], info


@pytest.mark.parametrize("name", ["grid750_EA", "grid100_scalar", "bar300k"])
def test_pcg_solve_to_convergence(systems, name):
    """Manufactured solution, eng.pcg_solve at rtol 1e-13 against scipy's CG with the same preconditioner and rtol:
    device error <= 10 * scipy's, device iterations <= 1.25 * scipy's, true residual <= 4 rtol |b| (the reference
    reaches 1.0 rtol).  grid750_EA (1 125 000 dofs, s per element from the nets) runs both grid-stride loops.
    Measured (scipy iterations, error | device iterations, error, true residual / |b|):
      grid750_EA      216  6.77e-12 | 216  6.77e-12  9.79e-14
      grid100_scalar  194  3.25e-12 | 194  3.19e-12  9.83e-14
      bar300k         490  1.40e-10 | 490  1.40e-10  9.98e-14"""
    S = systems(name)
    xs, b = manufactured(S, np.random.default_rng(9))
    y, it_ref, info = _scipy_cg(S, b, 5000)
    assert info == 0
    err_ref = np.max(np.abs(y - xs)) / np.max(np.abs(xs))
    x, it, ok, rr, bb = S.eng.pcg_solve(S.dev(b), rtol=RTOL)
    torch.cuda.synchronize()
    x = x.cpu().numpy()
    err = np.max(np.abs(x - xs)) / np.max(np.abs(xs))
    res = np.linalg.norm(b - S.Kff @ x) / np.linalg.norm(b)
    res_ref = np.linalg.norm(b - S.Kff @ y) / np.linalg.norm(b)
    print(f"{name}: scipy {it_ref} iterations, error {err_ref:.2e}, residual {res_ref:.2e} | device {it} iterations, "
          f"error {err:.2e}, true residual {res:.2e}")
    assert ok and rr <= RTOL ** 2 * bb
    assert np.all(x[S.mask] == 0.0)
    assert err <= 10 * err_ref
    assert it <= 1.25 * it_ref
    assert res <= 4 * RTOL


# ---------------------------------------------------------------------------------------------------------------------
# D. graph replay equals eager launches, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
def test_pcg_graph_replay_equals_eager_bitwise(systems, monkeypatch):
    S = systems("grid200_scalar")
    for seed in range(13, 20):                         # a right-hand side whose stop is not at a replay's very end
        _, b = manufactured(S, np.random.default_rng(seed))
        probe = CgRun(S, b)
        T = int(probe.iterate(4000)[0])                # the stopping iteration
        if 2 <= T % 64 <= 62:
            break
    assert probe.state()[1] == 1.0 and 2 <= T % 64 <= 62 and 64 < T < 400, T
    k = -(-T // 64)                                    # the stop test fires inside the k-th replay
    eager = CgRun(S, b)
    st_e = eager.iterate(64 * k)
    graphed = CgRun(S, b)
    g = graphed.graph(64)
    try:
        for i in range(k):
            st_g = graphed.replay(g)
            assert st_g[:2] == ((i + 1) * 64.0, 0.0) if i < k - 1 else st_g[:2] == (float(T), 1.0)
        assert st_g == st_e and st_e[0] == T
        a, e = graphed.read(), eager.read()
        assert same_bits(a, e) and same_bits(e, probe.read())
        # after the stop every launch is a no-op: x, the whole workspace and the counter stay
        assert graphed.replay(g) == st_g and eager.iterate(10) == st_e
        assert same_bits(graphed.read(), a) and same_bits(eager.read(), e)
    finally:
        S.eng.lib.pf_graph_destroy(g)

    def plain(n_iter):
        r = CgRun(S, b)
        st = r.iterate(n_iter)
        return r.read()[0], st

    def solve(**kw):
        x, it, ok, rr, bb = S.eng.pcg_solve(S.dev(b), rtol=RTOL, **kw)
        torch.cuda.synchronize()
        return x.cpu().numpy(), it, ok, rr, bb

    for max_iter in (40, 100, 64 * (k - 1) + 1, None):      # below poll | graph + eager remainder | ... | to the stop
        for graph_env in ("1", "0"):
            monkeypatch.setenv("PINNFEM_GRAPH", graph_env)
            x, it, ok, rr, bb = solve() if max_iter is None else solve(max_iter=max_iter)
            n_it = T if max_iter is None else min(max_iter, T)
            xp, stp = plain(n_it)
            assert it == n_it == stp[0], (max_iter, graph_env, it)
            assert np.array_equal(x, xp) and (rr, bb) == stp[2:]
            if n_it == T:
                assert ok
            elif max_iter in (40, 100):
                assert not ok                                  # cut short far from the stop


# ---------------------------------------------------------------------------------------------------------------------
# E. edge semantics
# ---------------------------------------------------------------------------------------------------------------------
def _finite_run(run):
    x, w = run.read()[0], run.parts()
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(w["state"]))
    for name in ("r", "z", "p", "dinv"):
        assert np.all(np.isfinite(w[name])), name
    return x, w


def test_pcg_zero_and_fixed_only_rhs(systems):
    S = systems("grid100_scalar")
    for b in (np.zeros(S.n), np.where(S.mask, 5.0, 0.0)):
        run = CgRun(S, b)
        assert run.state() == (0.0, 1.0, 0.0, 0.0)
        assert run.iterate(7) == (0.0, 1.0, 0.0, 0.0)
        x, w = _finite_run(run)
        assert not x.any() and not w["r"].any()
        x, it, ok, rr, bb = S.eng.pcg_solve(S.dev(b), rtol=RTOL)
        assert it == 0 and ok and not x.cpu().numpy().any()


def test_pcg_ignores_rhs_on_fixed_dofs(systems):
    S = systems("grid100_scalar")
    rng = np.random.default_rng(17)
    _, b = manufactured(S, rng)
    b2 = b + np.where(S.mask, rng.standard_normal(S.n) * 1e6, 0.0)
    outs = []
    for rhs in (b, b2):
        x, it, ok, rr, bb = S.eng.pcg_solve(S.dev(rhs), rtol=RTOL)
        outs.append((x.cpu().numpy(), it, ok, rr, bb))
    assert np.array_equal(outs[0][0], outs[1][0]) and outs[0][1:] == outs[1][1:] and outs[0][2]


def test_pcg_one_element_mesh():
    """One inclined element, one free dof (ux of its far node): K_ff is the 1 x 1 matrix s*c2, so the first step lands
    on b / (s*c2) and the stop test fires there."""
    nodes = np.array([[0.0, 0.0], [0.75, 0.5]])
    S = System(nodes, np.array([[1, 0]]), np.array([0, 1, 3]), 2)
    b = np.array([9.0, 9.0, 0.3, 9.0])                 # entries on fixed dofs are ignored
    run = CgRun(S, b)
    assert run.state() == (0.0, 0.0, 0.3 * 0.3, 0.3 * 0.3)
    st = run.iterate(5)
    x, w = _finite_run(run)
    # alpha = r.z / p.Ap, x = alpha * p, r = b - alpha * Ap: a handful of roundings each, so |r| <= 8 * 2^-53 |b| << rtol |b|
    assert st[:2] == (1.0, 1.0) and st[2] <= (8 * U53 * 0.3) ** 2
    want = 0.3 / (S.s[0] * S.geo[0, 0])
    assert abs(x[2] - want) <= 8 * U53 * want and not x[[0, 1, 3]].any()
    x2, it, ok, rr, bb = S.eng.pcg_solve(S.dev(b), rtol=RTOL)
    assert it == 1 and ok and np.array_equal(x2.cpu().numpy(), x)


def test_pcg_free_dof_without_stiffness():
    """A free dof no element stiffens (uy of the middle node of a collinear chain): dinv = 0 there, x stays 0, and
    nothing turns inf or NaN, with and without load on it.  solve_nr refuses such a model; this is the kernel's own
    behaviour."""
    nodes = np.array([[0.0, 0.0], [1.0, 0.0], [2.5, 0.0]])
    S = System(nodes, np.array([[0, 1], [2, 1]]), np.array([0, 1, 5]), 2)
    assert S.K.diagonal()[3] == 0.0
    for b3 in (0.0, 0.25):
        b = np.array([0.0, 0.0, 0.4, b3, -1.1, 0.0])
        run = CgRun(S, b)
        st = run.iterate(50)
        x, w = _finite_run(run)
        assert w["dinv"][3] == 0.0 and x[3] == 0.0 and np.all(x[S.mask] == 0.0)
        assert np.all(np.isfinite(st))
        free_stiff = np.array([2, 4])
        want = np.linalg.solve(S.K.toarray()[np.ix_(free_stiff, free_stiff)], b[free_stiff])
        assert np.allclose(x[free_stiff], want, rtol=1e-12, atol=0.0)      # 2 x 2, cond < 10
        if b3 == 0.0:
            assert st[1] == 1.0 and st[0] <= 2
        x2, it, ok, rr, bb = S.eng.pcg_solve(S.dev(b), rtol=RTOL, max_iter=50)
        assert np.all(np.isfinite(x2.cpu().numpy())) and math.isfinite(rr) and ok == (b3 == 0.0)


def test_pcg_rtol_zero_runs_to_max_iter(systems):
    S = systems("grid100_scalar")
    _, b = manufactured(S, np.random.default_rng(19))
    x, it, ok, rr, bb = S.eng.pcg_solve(S.dev(b), rtol=0.0, max_iter=200)
    x = x.cpu().numpy()
    assert np.all(np.isfinite(x)) and math.isfinite(rr) and bb > 0
    run = CgRun(S, b, rtol=0.0)
    st = run.iterate(200)
    assert st[0] == it <= 200 and (st[2], st[3]) == (rr, bb)
    if it < 200:                                       # only an exact zero of |r|^2 or r.z ends it early
        assert st[1] == 1.0 and (rr == 0.0 or run.parts()["state"][0] == 0.0)
    else:
        assert st[1] == 0.0 or rr == 0.0 or run.parts()["state"][0] == 0.0
    assert not ok or rr == 0.0
    assert rr < 1e-12 * bb                             # it did iterate: 200 steps take |r| far below 1e-6 |b|


def test_pcg_bad_arguments(systems):
    from pinn_fem_amd import _capi
    S = systems("grid100_scalar")
    eng, lib = S.eng, S.eng.lib
    b, x = S.dev(np.ones(S.n)), S.dev(np.zeros(S.n))
    ws = torch.zeros(int(lib.pf_pcg_workspace_count(eng._ref())), dtype=torch.float64, device=eng.device)
    st = (C.c_double * 4)()
    g = C.c_void_p()
    s = eng._stream()
    P, bp, xp, wp = eng._ref(), b.data_ptr(), x.data_ptr(), ws.data_ptr()
    calls = [
        lambda: lib.pf_pcg_begin(P, bp, xp, wp, -1e-3, s),
        lambda: lib.pf_pcg_begin(P, bp, xp, wp, float("nan"), s),
        lambda: lib.pf_pcg_begin(P, None, xp, wp, RTOL, s),
        lambda: lib.pf_pcg_begin(P, bp, None, wp, RTOL, s),
        lambda: lib.pf_pcg_begin(P, bp, xp, None, RTOL, s),
        lambda: lib.pf_pcg_begin(None, bp, xp, wp, RTOL, s),
        lambda: lib.pf_pcg_iterations(P, None, wp, 1, st, s),
        lambda: lib.pf_pcg_iterations(P, xp, None, 1, st, s),
        lambda: lib.pf_pcg_iterations(P, xp, wp, -1, st, s),
        lambda: lib.pf_pcg_graph_create(P, xp, wp, 0, s, C.byref(g)),
        lambda: lib.pf_pcg_graph_create(P, xp, None, 8, s, C.byref(g)),
        lambda: lib.pf_pcg_state(P, None, st, s),
        lambda: lib.pf_pcg_state(P, wp, None, s),
        lambda: lib.pf_kv_f64(P, None, xp, 0, s),
        lambda: lib.pf_kv_f64(P, bp, None, 0, s),
    ]
    for i, call in enumerate(calls):
        assert call() == _capi.PF_ERR_ARG, i
        msg = lib.pf_last_error()
        assert msg and msg.decode().startswith("pf_"), (i, msg)
    assert not g.value
    assert lib.pf_pcg_workspace_count(None) == _capi.PF_ERR_ARG
    with pytest.raises(ValueError, match="pf_pcg_begin"):
        eng.pcg_solve(b, rtol=-1.0)


# ---------------------------------------------------------------------------------------------------------------------
# F. solve_nr at scale
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("panels", [100, 1000])
def test_solve_nr_warren_girder_at_scale(panels):
    """Newton-Raphson on Warren girders (slender, beam-like: the hard case for a Jacobi preconditioner) against a
    sparse direct solve.  Yardstick: scipy's CG (same preconditioner, rtol 1e-13, same iteration allowance) against the
    same direct solve; the device may be 10 times worse.  Measured (relative to max |u|; scipy | device | device vs float64
    coordinates): 100 panels 2.53e-11 | 2.69e-11 | 2.00e-11; 1000 panels 9.98e-08 | 9.99e-08 | 1.27e-07 (57 199 CG
    iterations in scipy: at this condition number the direct solve and CG part ways at 1e-7)."""
    from pinn_fem_amd.fem.model import FEMModel, Material
    from pinn_fem_amd.fem.solver import SolverConfig, solve_nr
    from pinn_fem_amd.plan import build_host_plan, warren_mesh
    nodes, el, loads, fixed, _, _ = warren_mesh(panels)
    young, area = 2.0, 0.5
    model = FEMModel(nodes=nodes, elements=el, material=Material(young, area, 1.0), loads=loads, fixed_dofs=fixed,
                     dimension=2)
    res = solve_nr(model, SolverConfig(max_iterations=10, tolerance=1e-10), 1.0)
    assert res.converged
    u = res.displacements.reshape(-1)
    n = u.size
    mask = _mask_of(n, fixed)
    free = np.flatnonzero(~mask)
    b = np.where(mask, 0.0, loads)

    def direct(geo):
        K = ref.k_csr(geo, el, (young * area) / geo[:, 3], 2, len(nodes))
        out = np.zeros(n)
        out[free] = spla.spsolve(K[free][:, free].tocsc(), b[free])
        return K, out

    K, u_plan = direct(build_host_plan(nodes, el, loads, fixed, 2).egeo.astype(np.float64))
    Kff, dinv = ref.restrict_ff(K, mask), ref.jacobi_dinv(K, mask)
    n_it = [0]
    y, info = spla.cg(Kff, b, rtol=RTOL, atol=0.0, maxiter=40 * n + 2000,
                      M=spla.LinearOperator((n, n), matvec=lambda v: dinv * v, dtype=np.float64),
                      callback=lambda _: n_it.__setitem__(0, n_it[0] + 1))
    scale = np.max(np.abs(u_plan))
    err_ref = np.max(np.abs(y - u_plan)) / scale
    err = np.max(np.abs(u - u_plan)) / scale
    _, u_f64 = direct(ref.geo_f64(nodes, el, 2))
    err64 = np.max(np.abs(u - u_f64)) / np.max(np.abs(u_f64))
    print(f"warren {panels}: scipy CG {n_it[0]} iterations (info {info}) error {err_ref:.2e} | solve_nr "
          f"{res.history[-1]['iterations']:.0f} Newton steps, error {err:.2e} | vs float64 coordinates {err64:.2e}")
    assert err <= 10 * err_ref
    assert err64 <= 1e-6                       # float32 geometry in the plan: the bound of the fixture tests
    # equilibrium: the reactions carry the applied load
    R = res.reactions.reshape(-1, 2)
    total = np.sum(loads.reshape(-1, 2), axis=0)
    load = np.linalg.norm(total)
    assert np.all(R.reshape(-1)[free] == 0.0)
    assert np.all(np.abs(R.sum(axis=0) + total) <= 1e-9 * load)
