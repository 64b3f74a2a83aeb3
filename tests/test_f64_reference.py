"""CPU tests of tests/f64_reference.py, the float64 reference that tests/test_pcg_f64.py holds the device's
K v and Jacobi-PCG kernels against.  No GPU needed."""
import numpy as np
import pytest
import scipy.sparse.linalg as spla

import f64_reference as ref
from helpers import _random_truss, load_npz, orc

RTOL = 1e-13


def _fixture_systems():
    out = []
    for name in ("nr_warren_scalar.npz", "nr_chain300_scalar.npz"):
        rec = load_npz(name)
        out.append((name, rec["nodes"], rec["elements"], rec["loads"] * float(rec["lam"]), rec["fixed"], 2,
                    float(rec["young"]), float(rec["area"])))
    rng = np.random.default_rng(11)
    x = np.concatenate([[0.0], np.cumsum(0.5 + rng.random(40))])
    el = np.stack([np.arange(40), np.arange(1, 41)], axis=1)
    loads = np.zeros(41)
    loads[40], loads[17] = 2.0, -0.7
    out.append(("bar1d", x, el, loads, np.array([0]), 1, 3.0, 0.25))
    return out


SYSTEMS = _fixture_systems()


@pytest.mark.parametrize("case", SYSTEMS, ids=[c[0] for c in SYSTEMS])
def test_k_csr_equals_dense_oracle_assembly(case):
    _, nodes, el, loads, fixed, dim, young, area = case
    pb = orc.Problem(nodes=nodes, elements=el, loads=loads, fixed_dofs=fixed, dimension=dim, young=young,
                     area=area, density=1.0)
    k_dense, _, _ = orc.assemble_system_f64(pb, np.zeros(pb.ndof))
    geo = ref.geo_f64(nodes, el, dim)
    s = (young * area) / geo[:, 3]
    K = ref.k_csr(geo, el, s, dim, len(nodes))
    # same products s*c2 ...; only the order of the <= degree additions per entry differs
    assert np.max(np.abs(K.toarray() - k_dense)) <= 1e-14 * np.max(np.abs(k_dense))
    Ka = ref.abs_k_csr(geo, el, s, dim, len(nodes))
    assert np.all(Ka.toarray() >= np.abs(k_dense) - 1e-14 * np.max(np.abs(k_dense)))
    assert np.max(np.abs(Ka.diagonal() - K.diagonal())) <= 1e-14 * np.max(np.abs(k_dense))
    assert abs(K - K.T).max() == 0.0


@pytest.mark.parametrize("case", SYSTEMS, ids=[c[0] for c in SYSTEMS])
def test_pcg_reference_converges_to_the_direct_solve(case):
    _, nodes, el, loads, fixed, dim, young, area = case
    geo = ref.geo_f64(nodes, el, dim)
    K = ref.k_csr(geo, el, (young * area) / geo[:, 3], dim, len(nodes))
    n = K.shape[0]
    mask = np.zeros(n, dtype=bool)
    mask[fixed] = True
    free = np.flatnonzero(~mask)
    Kff, dinv = ref.restrict_ff(K, mask), ref.jacobi_dinv(K, mask)
    b = np.where(mask, 0.0, loads)
    x, r, p, state, stop, _ = ref.pcg_reference(Kff, dinv, b, RTOL, 40 * n + 2000)
    dense = K.toarray()[np.ix_(free, free)]
    exact = np.zeros(n)
    exact[free] = np.linalg.solve(dense, b[free])
    sparse = np.zeros(n)
    sparse[free] = spla.spsolve(Kff[free][:, free].tocsc(), b[free])
    assert stop is not None and state[1] and state[0] == stop
    assert np.all(x[mask] == 0.0) and np.all(r[mask] == 0.0) and np.all(p[mask] == 0.0)
    assert state[2] <= RTOL ** 2 * state[3] and state[3] == float(b @ b)
    # |x - x*| <= cond_2(K_ff) * |b - K x| / |b| * |x*|; the true residual is the recurrence's (<= rtol |b|) plus
    # its drift, allowed here the same amount again
    assert np.linalg.norm(b - Kff @ x) <= 2 * RTOL * np.linalg.norm(b)
    cond = np.linalg.cond(dense)
    for other in (exact, sparse):
        assert np.linalg.norm(x - other) <= 2 * RTOL * cond * np.linalg.norm(other)


def test_pcg_reference_stops_at_once_on_zero_rhs_and_counts_iterations():
    _, nodes, el, loads, fixed, dim, young, area = SYSTEMS[0]
    geo = ref.geo_f64(nodes, el, dim)
    K = ref.k_csr(geo, el, (young * area) / geo[:, 3], dim, len(nodes))
    mask = np.zeros(K.shape[0], dtype=bool)
    mask[fixed] = True
    Kff, dinv = ref.restrict_ff(K, mask), ref.jacobi_dinv(K, mask)
    x, r, p, state, stop, _ = ref.pcg_reference(Kff, dinv, np.zeros(K.shape[0]), RTOL, 10)
    assert state == (0, True, 0.0, 0.0) and stop == 0 and not x.any()
    b = np.where(mask, 0.0, loads)
    x, r, p, state, stop, snaps = ref.pcg_reference(Kff, dinv, b, 0.0, 5, snapshots=(1, 5, 9))
    assert state[0] == 5 and not state[1] and stop is None and sorted(snaps) == [1, 5]
    assert np.array_equal(snaps[5][0], x) and snaps[5][1] == state[2]
    # first step by hand: alpha = r.z / p.Kp with p = z = dinv*b
    z = dinv * b
    assert np.allclose(snaps[1][0], (b @ z) / (z @ (Kff @ z)) * z, rtol=1e-15, atol=0.0)


def _grid_system(side, seed=0):
    rng = np.random.default_rng(seed)
    nodes, el, fixed = ref.pinned_grid_truss(side, rng)
    geo = ref.geo_f64(nodes, el, 2)
    s = rng.uniform(0.5, 2.0, len(el)) / geo[:, 3]
    K = ref.k_csr(geo, el, s, 2, len(nodes))
    mask = np.zeros(K.shape[0], dtype=bool)
    mask[fixed] = True
    xs = np.where(mask, 0.0, rng.standard_normal(K.shape[0]))
    Kff = ref.restrict_ff(K, mask)
    return nodes, el, fixed, mask, Kff, ref.jacobi_dinv(K, mask), xs, Kff @ xs


def test_pinned_grid_structure():
    side = 23
    nodes, el, fixed = ref.pinned_grid_truss(side, np.random.default_rng(3))
    assert nodes.shape == (side * side, 2) and el.shape == (2 * side * (side - 1) + 2 * (side - 1) ** 2, 2)
    ij = np.stack(np.divmod(np.arange(side * side), side), axis=1)
    assert np.max(np.abs(nodes - ij)) <= 0.3
    d = ij[el[:, 1]] - ij[el[:, 0]]
    assert np.all(np.max(np.abs(d), axis=1) == 1)                       # neighbours only
    assert len({(min(a, b), max(a, b)) for a, b in el.tolist()}) == len(el)   # no element twice
    lo_first = el[:, 0] < el[:, 1]
    assert 0.3 < lo_first.mean() < 0.7                                  # orientation flipped at random
    assert np.any(np.diff(np.minimum(el[:, 0], el[:, 1])) < 0)          # element order shuffled
    assert len(fixed) == 2 * 3 * 3 and np.array_equal(fixed[:2], [0, 1])   # nodes (0|8|16, 0|8|16), both dofs
    # the same generator as a loop, against the helper the irregular-truss tests use: same element set on a full grid
    n2, e2 = _random_truss(side * side, np.random.default_rng(3))
    assert {(min(a, b), max(a, b)) for a, b in e2.tolist()} == {(min(a, b), max(a, b)) for a, b in el.tolist()}


def test_pinned_grid_is_well_conditioned_independent_of_size():
    """The GPU tests rely on this: Jacobi-PCG at rtol 1e-13 needs a few hundred iterations whatever the side
    (measured: 199 / 205 / 277 iterations at side 50 / 100 / 200)."""
    its = {}
    for side in (50, 100, 200):
        nodes, el, fixed, mask, Kff, dinv, xs, b = _grid_system(side)
        x, r, p, state, stop, _ = ref.pcg_reference(Kff, dinv, b, RTOL, 2000)
        its[side] = stop
        assert stop is not None and stop < 400, its
        assert np.linalg.norm(b - Kff @ x) <= 2 * RTOL * np.linalg.norm(b)
        # |x - x*| <= cond_2(K_ff) * |b - K x| / |b| * |x*|, the extreme eigenvalues by Lanczos
        free = np.flatnonzero(~mask)
        A = Kff[free][:, free].tocsc()
        lmax = spla.eigsh(A, k=1, which="LA", return_eigenvectors=False)[0]
        lmin = spla.eigsh(A, k=1, sigma=0.0, which="LM", return_eigenvectors=False)[0]
        print("side", side, "cond", lmax / lmin, "error", np.linalg.norm(x - xs) / np.linalg.norm(xs))
        assert np.linalg.norm(x - xs) <= 2 * RTOL * (lmax / lmin) * np.linalg.norm(xs)
        if side == 100:          # the restatement and scipy's CG walk the same path
            n_cg = [0]
            y, info = spla.cg(Kff, b, rtol=RTOL, atol=0.0, maxiter=2000,
                              M=spla.LinearOperator(Kff.shape, matvec=lambda v: dinv * v, dtype=np.float64),
                              callback=lambda _: n_cg.__setitem__(0, n_cg[0] + 1))
            assert info == 0 and abs(n_cg[0] - stop) <= 2
    print("pinned grid iterations", its)


def test_pinned_bar_converges_in_few_iterations():
    """1-D bar with every 64th node fixed: independent 63-dof segments whose spectra overlap, so the iteration
    count is bounded whatever the length (measured: 569 iterations at 3000 nodes, 603 at 300 000)."""
    its = {}
    for n_nodes in (3000, 300_000):
        rng = np.random.default_rng(7)
        x0, el, fixed = ref.pinned_bar(n_nodes, rng)
        geo = ref.geo_f64(x0, el, 1)
        K = ref.k_csr(geo, el, rng.uniform(0.5, 2.0, len(el)) / geo[:, 3], 1, n_nodes)
        mask = np.zeros(n_nodes, dtype=bool)
        mask[fixed] = True
        Kff, dinv = ref.restrict_ff(K, mask), ref.jacobi_dinv(K, mask)
        xs = np.where(mask, 0.0, rng.standard_normal(n_nodes))
        b = Kff @ xs
        x, r, p, state, stop, _ = ref.pcg_reference(Kff, dinv, b, RTOL, 2000)
        print("pinned bar", n_nodes, "iterations", stop)
        its[n_nodes] = stop
        # a segment of 63 unit springs has cond = 4*64^2/pi^2 ~ 1.7e3; s varies by 4 * 3 (lengths): cond <~ 2e4, and
        # CG needs at most sqrt(cond)/2 * ln(2/rtol) ~ 2200 steps
        assert stop is not None and stop < 2200
        assert np.linalg.norm(b - Kff @ x) <= 2 * RTOL * np.linalg.norm(b)
    assert its[300_000] <= 1.5 * its[3000], its          # 100 times the segments, not 100 times the work
