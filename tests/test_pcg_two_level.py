"""The two-level preconditioner of the float64 CG solve on the device (pf_coarse_setup, pf_pcg2_* in
pinn_fem_amd/csrc/pf_pcg.hip; HipEngine.pcg_solve(preconditioner="two-level"); SolverConfig.nr_preconditioner) against
the scipy restatement of tests/two_level_reference.py.

Bounds are float64 round-off bounds derived from operation counts at the assertion (unit 2^-53 of the sum of the
absolute terms), or the margins of tests/test_pcg_f64.py against scipy's CG with the same preconditioner."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import two_level_reference as tl
from device_driver import RTOL, U53, CgRun, bar1d, hub_truss, manufactured, same_bits, system_cache, wide_vector
from device_driver import LinearTruss as System
from helpers import _random_truss, load_run, product_example, rel_err

pytestmark = pytest.mark.gpu


def _warren(panels):
    from pinn_fem_amd.plan import warren_mesh
    nodes, el, loads, fixed, _, _ = warren_mesh(panels)
    return nodes, el, fixed


def _warren_dead_aggregate():
    """Warren girder of 40 panels, 9 strips, every dof of strip 4 fixed."""
    from pinn_fem_amd.coarse import strip_aggregates
    nodes, el, fixed = _warren(40)
    dead = np.flatnonzero(strip_aggregates(nodes, 2, 9) == 4)
    return nodes, el, np.unique(np.concatenate([fixed, 2 * dead, 2 * dead + 1]))


def _chain(n):
    from pinn_fem_amd.plan import chain_mesh
    nodes, el, loads, fixed, _, _ = chain_mesh(n)
    return nodes, el, fixed


SYSTEMS = {
    "warren100": lambda: (System(*_warren(100), 2, 2.0, 0.5), 32),
    "warren300": lambda: (System(*_warren(300), 2, 2.0, 0.5), 64),
    "warren1000": lambda: (System(*_warren(1000), 2, 2.0, 0.5), 256),
    "hub": lambda: (System(*hub_truss(np.random.default_rng(2500)), 2, 2.0, 0.5), None),
    "hub_E": lambda: (System(*hub_truss(np.random.default_rng(2500)), 2, 2.0, 0.5, (20, None)), None),
    "random": lambda: (System(*_random_truss(611, np.random.default_rng(611)), np.array([0, 1, 41, 700, 1221]), 2), 37),
    "bar": lambda: (System(*bar1d(2000, np.random.default_rng(7)), 1, 3.0, 0.25), 100),
    "dead": lambda: (System(*_warren_dead_aggregate(), 2, 2.0, 0.5), 9),
    "chain": lambda: (System(*_chain(200), 2, 2.0, 0.5), 16),
}


@pytest.fixture(scope="module")
def systems():
    yield from system_cache(lambda name: SYSTEMS[name]())


def _coarse(S, n_agg):
    dc = S.eng.coarse_space(n_agg)
    assert dc is not None
    cs = dc.space
    return dc, cs, int(np.max(np.diff(cs.agg_ptr)))


def _run(S, n_agg, b):
    return CgRun(S, b, dc=S.eng.coarse_space(n_agg))


# ---------------------------------------------------------------------------------------------------------------------
# A. A_c = Z^T K Z from the device
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["warren100", "hub", "random", "bar", "hub_E", "dead", "chain"])
def test_coarse_matrix_from_device(systems, name):
    S, n_agg = systems(name)
    dc, cs, m = _coarse(S, n_agg)
    if name == "hub_E":
        assert np.ptp(S.E) > 0.01 * np.mean(S.E)                  # net properties: E really varies over the mesh
    Z = tl.z_matrix(cs)
    want = (Z.T @ (S.K @ Z)).toarray()
    Za = abs(Z)
    scale = (Za.T @ (S.Kabs @ Za)).toarray()
    # per entry, in units of 2^-53 of sum |z_i||ke||z_j|: a row of K z_j costs 8 + degree roundings (the count of
    # test_pcg_f64.py for K v; the difference of two coefficients stands for dx), the product with z_i one, the sum
    # over the aggregate's dim * m node dofs one per term; the CSR restatement rounds once per product and per
    # addition: 4 * degree for K Z, dim * m for Z^T (K Z).  Both sides together, rounded up:
    terms = 2 * (16 + 4 * S.max_degree + S.dim * m)
    err = np.abs(dc.a_c - want)
    worst = float(np.max(err / np.maximum(scale, 1e-300))) / U53
    print(f"{name}: {cs.n_agg} aggregates of <= {m} nodes, {cs.n_coarse} columns, max degree {S.max_degree}: worst error "
          f"{worst:.2f} * 2^-53 |Z|^T|K||Z| (bound {terms})")
    assert dc.a_c.shape == (cs.n_coarse, cs.n_coarse) and np.all(np.isfinite(dc.a_c))
    assert np.all(err <= terms * U53 * scale)                      # exact zeros where no element joins two aggregates
    assert np.allclose(dc.a_inv_host, dc.a_inv_host.T, rtol=0, atol=0)


# ---------------------------------------------------------------------------------------------------------------------
# B. one application of M^-1
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["warren100", "hub", "bar", "dead", "chain"])
def test_one_application(systems, name):
    """pf_pcg2_begin leaves w = Z^T r, y = A^-1 w, z = M^-1 r (r = b on free dofs) and p = z in the workspace."""
    S, n_agg = systems(name)
    dc, cs, m = _coarse(S, n_agg)
    rng = np.random.default_rng(21)
    b = wide_vector(rng, S.n)
    run = _run(S, n_agg, b)
    x, w = run.read()[0], run.parts()
    P = tl.TwoLevel(S.K, S.mask, cs, a_inv=dc.a_inv_host)         # the inverse the device reads: A^-1 is not under test
    r = np.where(S.mask, 0.0, b)
    assert not x.any() and np.array_equal(w["r"], r) and np.array_equal(w["p"], w["z"])
    # w = Z^T r: dim * m products and additions per column, on both sides
    Za = abs(P.Z)
    t_w = 2 * S.dim * m + 2
    assert np.all(np.abs(w["w"][:cs.n_coarse] - P.Z.T @ r) <= 2 * t_w * U53 * (Za.T @ np.abs(r)))
    assert not w["w"][cs.n_coarse:].any() and not w["y"][cs.n_coarse:].any()
    # z: the error of w passes through |A^-1| and |Z|; y adds n_coarse products and additions per row, z three
    # coefficient products, the dinv product (dinv itself within 4 ulp, test_pcg_f64.py) and three additions
    t_z = t_w + (2 * cs.n_coarse + 2) + 12
    want, scale = P.apply(b), P.apply_abs(b)
    err = np.abs(w["z"] - want)
    worst = float(np.max(err / np.maximum(scale, 1e-300))) / U53
    print(f"{name}: M^-1 r worst error {worst:.2f} * 2^-53 (|D^-1||r| + |Z||A^-1||Z|^T|r|) (bound {2 * t_z})")
    assert np.all(err <= 2 * t_z * U53 * scale)
    # fixed dofs, and with them every dropped column, contribute exactly nothing
    assert np.all(w["z"][S.mask] == 0.0) and np.all(np.isfinite(w["z"]))
    if name == "chain":
        assert cs.n_coarse == cs.n_agg and not w["z"][1::2].any()
    if name == "dead":
        dead = np.flatnonzero(cs.node_agg == 4)
        assert cs.columns_of(4) == 0 and not w["z"][2 * dead].any() and not w["z"][2 * dead + 1].any()
    # r.z and |b|^2 as the state holds them
    rz, bb = math.fsum(w["r"] * w["z"]), math.fsum(r * r)
    assert abs(w["state"][0] - rz) <= 1e-12 * math.fsum(np.abs(w["r"] * w["z"])) and abs(w["state"][3] - bb) <= 1e-13 * bb


# ---------------------------------------------------------------------------------------------------------------------
# C. solve to convergence
# ---------------------------------------------------------------------------------------------------------------------
def _solve_both(S, n_agg, b):
    dc, cs, _ = _coarse(S, n_agg)
    P = tl.TwoLevel(S.K, S.mask, cs)                               # the host pipeline's own inverse
    y, it_ref, info = tl.cg(S.Kff, b, P.operator(), 40 * S.n + 2000)
    assert info == 0
    x, it, ok, rr, bb = S.eng.pcg_solve(S.dev(b), rtol=RTOL, preconditioner="two-level", n_aggregates=n_agg)
    torch.cuda.synchronize()
    return y, it_ref, x.cpu().numpy(), it, ok, rr, bb


@pytest.mark.parametrize("name", ["warren100", "hub", "bar"])
def test_two_level_solve_to_convergence(systems, name):
    """Manufactured solution at rtol 1e-13; scipy's CG with the restated preconditioner is the yardstick."""
    S, n_agg = systems(name)
    xs, b = manufactured(S, np.random.default_rng(9))
    y, it_ref, x, it, ok, rr, bb = _solve_both(S, n_agg, b)
    err_ref = np.max(np.abs(y - xs)) / np.max(np.abs(xs))
    err = np.max(np.abs(x - xs)) / np.max(np.abs(xs))
    res = np.linalg.norm(b - S.Kff @ x) / np.linalg.norm(b)
    print(f"{name}: scipy {it_ref} iterations, error {err_ref:.2e} | device {it} iterations, error {err:.2e}, "
          f"true residual {res:.2e}")
    assert ok and rr <= RTOL ** 2 * bb
    assert np.all(x[S.mask] == 0.0)
    assert it <= 1.25 * it_ref
    assert err <= 10 * err_ref
    assert res <= 4 * RTOL


def test_two_level_solve_warren_1000(systems):
    """4 002 dofs, 256 aggregates: the recursive and the true residual part ways (as for Jacobi), so only the error
    against the direct solve is held against scipy's."""
    S, n_agg = systems("warren1000")
    xs, b = manufactured(S, np.random.default_rng(9))
    u = tl.direct_solve(S.K, S.mask, b)
    y, it_ref, x, it, ok, rr, bb = _solve_both(S, n_agg, b)
    scale = np.max(np.abs(u))
    err_ref, err = np.max(np.abs(y - u)) / scale, np.max(np.abs(x - u)) / scale
    print(f"warren1000/256: scipy {it_ref} iterations, error {err_ref:.2e} | device {it} iterations, error {err:.2e}")
    assert ok and np.all(x[S.mask] == 0.0)
    assert err <= 10 * err_ref


def test_two_level_takes_a_tenth_of_the_jacobi_iterations(systems):
    S, n_agg = systems("warren300")
    from pinn_fem_amd.plan import warren_mesh
    b = np.where(S.mask, 0.0, warren_mesh(300)[2])
    x1, it1, ok1, _, _ = S.eng.pcg_solve(S.dev(b), rtol=RTOL)
    x2, it2, ok2, _, _ = S.eng.pcg_solve(S.dev(b), rtol=RTOL, preconditioner="two-level", n_aggregates=n_agg)
    print(f"warren300: Jacobi {it1} iterations | two-level/64 {it2} iterations")
    assert ok1 and ok2
    assert it2 <= it1 / 10
    u = tl.direct_solve(S.K, S.mask, b)
    assert np.max(np.abs(x2.cpu().numpy() - u)) <= 10 * np.max(np.abs(x1.cpu().numpy() - u)) + 1e-12 * np.max(np.abs(u))


# ---------------------------------------------------------------------------------------------------------------------
# D. graph replay equals eager launches, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
def test_two_level_graph_replay_equals_eager_bitwise(systems):
    S, n_agg = systems("warren300")
    _, b = manufactured(S, np.random.default_rng(13))
    probe = _run(S, n_agg, b)
    T = int(probe.iterate(2000)[0])                                 # the stopping iteration
    assert probe.state()[1] == 1.0
    poll = next(q for q in (16, 15, 14, 13) if 2 <= T % q <= q - 2)
    assert T > 4 * poll, T
    k = -(-T // poll)
    eager, graphed = _run(S, n_agg, b), _run(S, n_agg, b)
    g = graphed.graph(poll)
    try:
        for i in range(3):
            st_g = graphed.replay(g)
        st_e = eager.iterate(3 * poll)
        assert st_g == st_e == (3.0 * poll, 0.0, st_e[2], st_e[3])
        assert same_bits(graphed.read(), eager.read())             # after 3 polls: x, r, z, p, ap, dinv, partials, state, w, y
        for i in range(3, k):
            st_g = graphed.replay(g)
        st_e = eager.iterate((k - 3) * poll)
        assert st_g == st_e and st_e[:2] == (float(T), 1.0)         # stopped in mid-replay
        a, e = graphed.read(), eager.read()
        assert same_bits(a, e) and same_bits(e, probe.read())
        assert graphed.replay(g) == st_g and eager.iterate(5) == st_e           # after the stop every launch is a no-op
        assert same_bits(graphed.read(), a) and same_bits(eager.read(), e)
    finally:
        S.eng.lib.pf_graph_destroy(g)
    outs = []
    for _ in range(2):
        x, it, ok, rr, bb = S.eng.pcg_solve(S.dev(b), rtol=RTOL, preconditioner="two-level", n_aggregates=n_agg)
        outs.append((x.cpu().numpy(), it, ok, rr, bb))
    assert np.array_equal(outs[0][0], outs[1][0]) and outs[0][1:] == outs[1][1:]
    assert np.array_equal(outs[0][0], a[0]) and outs[0][1] == T


# ---------------------------------------------------------------------------------------------------------------------
# E. edge semantics
# ---------------------------------------------------------------------------------------------------------------------
def test_two_level_zero_and_fixed_only_rhs(systems):
    S, n_agg = systems("warren100")
    for b in (np.zeros(S.n), np.where(S.mask, 5.0, 0.0)):
        run = _run(S, n_agg, b)
        assert run.state() == (0.0, 1.0, 0.0, 0.0)
        assert run.iterate(7) == (0.0, 1.0, 0.0, 0.0)
        x, w = run.read()[0], run.parts()
        assert not x.any() and not w["r"].any() and not w["z"].any() and not w["p"].any()
        assert np.all(np.isfinite(w["state"])) and np.all(np.isfinite(w["dinv"]))
        x, it, ok, rr, bb = S.eng.pcg_solve(S.dev(b), rtol=RTOL, preconditioner="two-level", n_aggregates=n_agg)
        assert it == 0 and ok and not x.cpu().numpy().any()


def test_two_level_one_element_mesh():
    """One inclined element, one free dof: one aggregate with one column, A_c = K_ff = s*c2, M^-1 = 2 / (s*c2); the
    first step lands on b / (s*c2)."""
    S = System(np.array([[0.0, 0.0], [0.75, 0.5]]), np.array([[1, 0]]), np.array([0, 1, 3]), 2)
    dc, cs, _ = _coarse(S, None)
    assert (cs.n_agg, cs.n_coarse) == (1, 1)
    k = S.s[0] * S.geo[0, 0]
    assert abs(dc.a_c[0, 0] - k) <= 4 * U53 * k
    b = np.array([9.0, 9.0, 0.3, 9.0])
    x, it, ok, rr, bb = S.eng.pcg_solve(S.dev(b), rtol=RTOL, preconditioner="two-level")
    x = x.cpu().numpy()
    assert it == 1 and ok and abs(x[2] - 0.3 / k) <= 8 * U53 * 0.3 / k and not x[[0, 1, 3]].any()


def test_two_level_aggregate_counts(systems):
    S, _ = systems("warren100")
    xs, b = manufactured(S, np.random.default_rng(3))
    for n_agg, expect in ((1, 1), (250, 201)):                       # above the node count: clamped to it
        x, it, ok, rr, bb = S.eng.pcg_solve(S.dev(b), rtol=RTOL, preconditioner="two-level", n_aggregates=n_agg)
        assert ok and S.eng.coarse_space(n_agg).space.n_agg == expect
        assert np.max(np.abs(x.cpu().numpy() - xs)) <= 1e-6 * np.max(np.abs(xs))
    small = System(*_warren(20), 2, 2.0, 0.5)                        # 41 nodes
    xs, b = manufactured(small, np.random.default_rng(4))
    x, it, ok, rr, bb = small.eng.pcg_solve(small.dev(b), rtol=RTOL, preconditioner="two-level", n_aggregates=200)
    assert ok and small.eng.coarse_space(200).space.n_agg == 41
    assert np.max(np.abs(x.cpu().numpy() - xs)) <= 1e-8 * np.max(np.abs(xs))
    with pytest.raises(ValueError):
        small.eng.pcg_solve(small.dev(b), preconditioner="two-level", n_aggregates=257)
    with pytest.raises(ValueError):
        small.eng.pcg_solve(small.dev(b), preconditioner="ilu")
    # the caller's own map, and the cache: same request -> same object; another stiffness -> rebuilt
    own = np.arange(41) // 6
    x2, it2, ok2, _, _ = small.eng.pcg_solve(small.dev(b), rtol=RTOL, preconditioner="two-level", aggregates=own)
    assert ok2 and np.max(np.abs(x2.cpu().numpy() - xs)) <= 1e-8 * np.max(np.abs(xs))
    first = small.eng.coarse_space(aggregates=own)
    assert first is small.eng.coarse_space(aggregates=own) and np.array_equal(first.space.node_agg, own)
    small.eng.specs[0].scale *= 2.0
    small.eng.configure(lam=1.0)
    second = small.eng.coarse_space(aggregates=own)
    assert second is not first and np.allclose(second.a_c, 2.0 * first.a_c, rtol=1e-15, atol=0.0)


def test_two_level_falls_back_to_jacobi_with_a_warning():
    """A free dof no element stiffens inside an aggregate's translation makes Z^T K Z singular: the solve warns and
    runs the Jacobi path."""
    nodes = np.array([[0.0, 0.0], [1.0, 0.0], [2.5, 0.0]])
    S = System(nodes, np.array([[0, 1], [2, 1]]), np.array([0, 1, 5]), 2)
    b = np.array([0.0, 0.0, 0.4, 0.0, -1.1, 0.0])
    with pytest.warns(RuntimeWarning, match="Jacobi"):
        x, it, ok, rr, bb = S.eng.pcg_solve(S.dev(b), rtol=RTOL, max_iter=50, preconditioner="two-level")
    xj, itj, okj, rrj, bbj = S.eng.pcg_solve(S.dev(b), rtol=RTOL, max_iter=50)
    assert np.array_equal(x.cpu().numpy(), xj.cpu().numpy()) and (it, ok, rr, bb) == (itj, okj, rrj, bbj)


def test_two_level_bad_arguments(systems):
    from pinn_fem_amd import _capi
    S, n_agg = systems("warren100")
    eng, lib = S.eng, S.eng.lib
    dc = eng.coarse_space(n_agg)
    b, x = S.dev(np.ones(S.n)), S.dev(np.zeros(S.n))
    ws = torch.zeros(int(lib.pf_pcg2_workspace_count(eng._ref())), dtype=torch.float64, device=eng.device)
    ac = torch.zeros(dc.space.n_coarse ** 2, dtype=torch.float64, device=eng.device)
    st, g, s = (C.c_double * 4)(), C.c_void_p(), eng._stream()
    P, cc, bp, xp, wp, ap = eng._ref(), C.byref(dc.record), b.data_ptr(), x.data_ptr(), ws.data_ptr(), ac.data_ptr()

    def broken(**kw):
        rec = _capi.PfCoarse.from_buffer_copy(dc.record)
        for k, v in kw.items():
            setattr(rec, k, v)
        return C.byref(rec)

    bad = [broken(n_agg=0), broken(n_agg=-1), broken(n_agg=257), broken(n_coarse=-1), broken(n_coarse=3 * n_agg + 1),
           broken(node_agg=None), broken(agg_off=None), broken(zcoef=None), broken(agg_ptr=None), broken(agg_nodes=None)]
    calls = [lambda: lib.pf_coarse_setup(None, cc, ap, s), lambda: lib.pf_coarse_setup(P, None, ap, s),
             lambda: lib.pf_coarse_setup(P, cc, None, s)]
    calls += [lambda c=c: lib.pf_coarse_setup(P, c, ap, s) for c in bad]
    calls += [lambda c=c: lib.pf_pcg2_begin(P, c, bp, xp, wp, RTOL, s) for c in bad + [broken(a_inv=None)]]
    calls += [
        lambda: lib.pf_pcg2_begin(None, cc, bp, xp, wp, RTOL, s),
        lambda: lib.pf_pcg2_begin(P, None, bp, xp, wp, RTOL, s),
        lambda: lib.pf_pcg2_begin(P, cc, None, xp, wp, RTOL, s),
        lambda: lib.pf_pcg2_begin(P, cc, bp, None, wp, RTOL, s),
        lambda: lib.pf_pcg2_begin(P, cc, bp, xp, None, RTOL, s),
        lambda: lib.pf_pcg2_begin(P, cc, bp, xp, wp, -1e-3, s),
        lambda: lib.pf_pcg2_begin(P, cc, bp, xp, wp, float("nan"), s),
        lambda: lib.pf_pcg2_iterations(None, cc, xp, wp, 1, st, s),
        lambda: lib.pf_pcg2_iterations(P, None, xp, wp, 1, st, s),
        lambda: lib.pf_pcg2_iterations(P, broken(a_inv=None), xp, wp, 1, st, s),
        lambda: lib.pf_pcg2_iterations(P, cc, None, wp, 1, st, s),
        lambda: lib.pf_pcg2_iterations(P, cc, xp, None, 1, st, s),
        lambda: lib.pf_pcg2_iterations(P, cc, xp, wp, -1, st, s),
        lambda: lib.pf_pcg2_graph_create(None, cc, xp, wp, 8, s, C.byref(g)),
        lambda: lib.pf_pcg2_graph_create(P, None, xp, wp, 8, s, C.byref(g)),
        lambda: lib.pf_pcg2_graph_create(P, cc, None, wp, 8, s, C.byref(g)),
        lambda: lib.pf_pcg2_graph_create(P, cc, xp, None, 8, s, C.byref(g)),
        lambda: lib.pf_pcg2_graph_create(P, cc, xp, wp, 0, s, C.byref(g)),
        lambda: lib.pf_pcg2_graph_create(P, cc, xp, wp, -3, s, C.byref(g)),
        lambda: lib.pf_pcg2_graph_create(P, cc, xp, wp, 8, s, None),
        lambda: lib.pf_pcg2_state(None, wp, st, s),
        lambda: lib.pf_pcg2_state(P, None, st, s),
        lambda: lib.pf_pcg2_state(P, wp, None, s),
    ]
    for i, call in enumerate(calls):
        assert call() == _capi.PF_ERR_ARG, i
        msg = lib.pf_last_error()
        assert msg and msg.decode().startswith("pf_"), (i, msg)
    assert not g.value
    assert lib.pf_pcg2_workspace_count(None) == _capi.PF_ERR_ARG
    assert lib.pf_pcg2_workspace_count(P) == lib.pf_pcg_workspace_count(P) + 2 * _capi.PF_COARSE_MAX
    with pytest.raises(ValueError, match="pf_pcg2_begin"):
        eng.pcg_solve(b, rtol=-1.0, preconditioner="two-level", n_aggregates=n_agg)


# ---------------------------------------------------------------------------------------------------------------------
# F. solve_nr with nr_preconditioner = "two-level"
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("panels", [100, 1000])
def test_solve_nr_two_level_warren_girder(panels):
    """The yardstick of test_pcg_f64.py::test_solve_nr_warren_girder_at_scale: error against the sparse direct solve on
    the plan's geometry, at most 10 times that of scipy's CG (here with the restated two-level preconditioner, default
    aggregate count, rtol 1e-13) on the same system."""
    import f64_reference as ref
    from pinn_fem_amd.coarse import build_coarse_space
    from pinn_fem_amd.fem.model import FEMModel, Material
    from pinn_fem_amd.fem.solver import SolverConfig, solve_nr
    from pinn_fem_amd.plan import build_host_plan, warren_mesh
    nodes, el, loads, fixed, _, _ = warren_mesh(panels)
    young, area = 2.0, 0.5
    model = FEMModel(nodes=nodes, elements=el, material=Material(young, area, 1.0), loads=loads, fixed_dofs=fixed,
                     dimension=2)
    res = solve_nr(model, SolverConfig(max_iterations=10, tolerance=1e-10, nr_preconditioner="two-level"), 1.0)
    assert res.converged
    u = res.displacements.reshape(-1)
    n = u.size
    mask = np.zeros(n, dtype=bool)
    mask[fixed] = True
    b = np.where(mask, 0.0, loads)
    geo = build_host_plan(nodes, el, loads, fixed, 2).egeo.astype(np.float64)
    K = ref.k_csr(geo, el, (young * area) / geo[:, 3], 2, len(nodes))
    u_plan = tl.direct_solve(K, mask, b)
    P = tl.TwoLevel(K, mask, build_coarse_space(nodes, 2, mask))
    y, n_it, info = tl.cg(P.Kff, b, P.operator(), 40 * n + 2000)
    scale = np.max(np.abs(u_plan))
    err_ref, err = np.max(np.abs(y - u_plan)) / scale, np.max(np.abs(u - u_plan)) / scale
    eng = model._pf_engine_cache[1]
    print(f"warren {panels}: scipy CG {n_it} iterations (info {info}) error {err_ref:.2e} | solve_nr "
          f"{res.history[-1]['iterations']:.0f} Newton steps, {eng.pcg_iterations} CG iterations, error {err:.2e}")
    assert eng.coarse_space() is not None and eng.pcg_iterations <= 1.25 * n_it * res.history[-1]["iterations"]
    assert err <= 10 * err_ref
    R = res.reactions.reshape(-1, 2)
    total = np.sum(loads.reshape(-1, 2), axis=0)
    assert np.all(R.reshape(-1)[~mask] == 0.0)
    assert np.all(np.abs(R.sum(axis=0) + total) <= 1e-9 * np.linalg.norm(total))


@pytest.mark.parametrize("ex", ["example1", "example1-1", "example5", "example5-P"])
def test_nr_two_level_example_runs(ex):
    """The golden NR / scalar-hybrid examples with the two-level preconditioner: the tolerances of
    test_hip_parity.py::test_nr_and_scalar_hybrid_example_runs, and the same Newton iteration count."""
    from pinn_fem_amd.cli import generic as g
    run = load_run(ex)
    parsed = product_example(ex)
    parsed["solver_config"].nr_preconditioner = "two-level"
    out = g.solve_problem(parsed)
    ref_out = run["result"]
    assert out["converged"] == ref_out["converged"]
    assert rel_err(out["displacements"], ref_out["displacements"]) < 1e-9
    assert np.max(np.abs(np.array(out["reactions"]) - np.array(ref_out["reactions"]))) < 1e-9
    last, rlast = out["history"][-1], ref_out["history"][-1]
    assert last["iterations"] == rlast["iterations"] and last["converged"] == rlast["converged"]
    assert abs(last["max_strain"] - rlast["max_strain"]) < 1e-9
    eng = parsed["model"]._pf_engine_cache[1]
    assert eng._coarse_cache is not None and eng._coarse_cache[1] is not None      # the two-level path really ran
