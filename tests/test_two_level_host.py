"""Host side of the two-level preconditioner (pinn_fem_amd/coarse.py): aggregation map, Gram column selection and
the pipeline Gram selection -> Z^T K Z -> Cholesky inverse, used as M in scipy's CG against the iteration counts of a
float64 numpy/scipy prototype (E*A = 1, rtol 1e-13).  No GPU."""
import numpy as np
import pytest

import two_level_reference as tl
from pinn_fem_amd.coarse import (MAX_AGGREGATES, build_coarse_space, check_preconditioner, coarse_inverse,
                                 default_aggregate_count, strip_aggregates)
from pinn_fem_amd.plan import chain_mesh, warren_mesh


def _mask(n, fixed):
    m = np.zeros(n, dtype=bool)
    m[np.asarray(fixed, dtype=int)] = True
    return m


# ---- aggregation map ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_agg", [1, 7, 32, 256])
def test_strip_aggregates_assign_every_node_evenly_and_follow_the_geometry(n_agg):
    nodes = warren_mesh(300)[0]
    agg = strip_aggregates(nodes, 2, n_agg)
    assert agg.dtype == np.int32 and agg.shape == (len(nodes),)
    counts = np.bincount(agg, minlength=n_agg)
    assert agg.min() == 0 and agg.max() == n_agg - 1 and counts.sum() == len(nodes)
    assert counts.max() - counts.min() <= 1
    perm = np.random.default_rng(n_agg).permutation(len(nodes))          # new id k is old node perm[k]
    assert np.array_equal(strip_aggregates(nodes[perm], 2, n_agg), agg[perm])
    # strips along x (the axis of largest extent): an aggregate's x range ends before the next one starts
    hi = np.array([nodes[agg == a, 0].max() for a in range(n_agg)])
    lo = np.array([nodes[agg == a, 0].min() for a in range(n_agg)])
    assert np.all(hi[:-1] < lo[1:])


def test_strip_aggregates_ties_count_and_limits():
    grid = np.stack(np.meshgrid(np.arange(6.0), np.arange(4.0), indexing="ij"), -1).reshape(-1, 2)   # many equal x
    agg = strip_aggregates(grid, 2, 5)
    perm = np.random.default_rng(0).permutation(len(grid))
    assert np.array_equal(strip_aggregates(grid[perm], 2, 5), agg[perm])
    assert default_aggregate_count(3) == 1 and default_aggregate_count(402) == 50 and default_aggregate_count(10 ** 6) == 256
    assert strip_aggregates(grid, 2).max() == len(grid) // 8 - 1
    assert strip_aggregates(grid, 2, 200).max() == len(grid) - 1                     # clamped to the node count
    assert np.array_equal(np.sort(strip_aggregates(np.array([3.0, 1.0, 2.0]), 1, 3)), [0, 1, 2])
    with pytest.raises(ValueError):
        strip_aggregates(grid, 2, MAX_AGGREGATES + 1)
    with pytest.raises(ValueError):
        strip_aggregates(grid, 2, 0)
    with pytest.raises(ValueError):
        build_coarse_space(grid, 2, np.zeros(48, dtype=bool), aggregates=np.zeros(5))
    with pytest.raises(ValueError):
        build_coarse_space(np.arange(600.0), 1, np.zeros(600, dtype=bool), aggregates=np.arange(600))
    with pytest.raises(ValueError):
        check_preconditioner("ilu")
    assert check_preconditioner("two-level") == "two-level"


# ---- column selection -----------------------------------------------------------------------------------------------
def _orthonormal(cs):
    Z = tl.z_matrix(cs)
    G = (Z.T @ Z).toarray()
    return np.max(np.abs(G - np.eye(cs.n_coarse))) if cs.n_coarse else 0.0


def test_column_selection_warren():
    nodes, el, loads, fixed, _, _ = warren_mesh(100)
    cs = build_coarse_space(nodes, 2, _mask(402, fixed), 16)
    assert [cs.columns_of(a) for a in range(16)] == [3] * 16 and cs.n_coarse == 48
    assert _orthonormal(cs) <= 1e-12
    assert not cs.zcoef[_mask(402, fixed)].any()
    # node lists: every node once, ascending inside its aggregate
    for a in range(16):
        ids = cs.agg_nodes[cs.agg_ptr[a]:cs.agg_ptr[a + 1]]
        assert np.all(np.diff(ids) > 0) and np.all(cs.node_agg[ids] == a)
    assert np.array_equal(np.sort(cs.agg_nodes), np.arange(201))
    assert np.array_equal(tl.z_matrix(cs).toarray(), cs.to_sparse().toarray())


def test_column_selection_chain_fixed_aggregate_and_bar():
    nodes, el, loads, fixed, _, _ = chain_mesh(2000)
    cs = build_coarse_space(nodes, 2, _mask(4002, fixed), 64)
    assert [cs.columns_of(a) for a in range(64)] == [1] * 64 and cs.n_coarse == 64
    assert _orthonormal(cs) <= 1e-12
    assert not cs.zcoef[1::2].any() and not cs.zcoef[:, 1:].any()          # uy fixed everywhere; one column only
    # a fully fixed aggregate loses all its columns
    nodes, el, loads, fixed, _, _ = warren_mesh(40)
    agg = strip_aggregates(nodes, 2, 9)
    dead = np.flatnonzero(agg == 4)
    mask = _mask(162, np.concatenate([fixed, 2 * dead, 2 * dead + 1]))
    cs = build_coarse_space(nodes, 2, mask, 9)
    assert cs.columns_of(4) == 0 and all(cs.columns_of(a) == 3 for a in range(9) if a != 4)
    assert cs.n_coarse == 24 and _orthonormal(cs) <= 1e-12 and not cs.zcoef[mask].any()
    # 1-D bar: the translation only; an aggregate of one fixed node has none
    x = np.cumsum(0.5 + np.random.default_rng(1).random(50))
    cs = build_coarse_space(x, 1, _mask(50, [0]), 50)
    assert cs.columns_of(0) == 0 and [cs.columns_of(a) for a in range(1, 50)] == [1] * 49
    cs = build_coarse_space(x, 1, _mask(50, [0]), 5)
    assert [cs.columns_of(a) for a in range(5)] == [1] * 5 and _orthonormal(cs) <= 1e-12
    # the caller's own map, any labels
    cs = build_coarse_space(x, 1, _mask(50, [0]), aggregates=np.where(np.arange(50) < 20, 17, -3))
    assert cs.n_agg == 2 and np.array_equal(np.unique(cs.node_agg), [0, 1]) and cs.node_agg[0] == 1


def test_coarse_inverse_refuses_an_indefinite_matrix():
    with pytest.raises(np.linalg.LinAlgError):
        coarse_inverse(np.array([[1.0, 2.0], [2.0, 1.0]]))
    with pytest.raises(np.linalg.LinAlgError):
        coarse_inverse(np.array([[1.0, np.nan], [np.nan, 1.0]]))
    a = np.array([[4.0, 1.0], [1.0, 3.0]])
    assert np.allclose(coarse_inverse(a) @ a, np.eye(2), atol=1e-15)


# ---- host pipeline as M in scipy's CG -------------------------------------------------------------------------------
def _solve_pair(nodes, el, loads, fixed, n_agg, aggregates=None):
    n = 2 * len(nodes)
    K, mask = tl.mesh_system(nodes, el, fixed, 2)
    b = np.where(mask, 0.0, loads)
    cs = build_coarse_space(nodes, 2, mask, n_agg, aggregates)
    P = tl.TwoLevel(K, mask, cs)
    u = tl.direct_solve(K, mask, b)
    scale = np.max(np.abs(u))
    y2, it2, info2 = tl.cg(P.Kff, b, P.operator(), 40 * n + 2000)
    y1, it1, info1 = tl.cg(P.Kff, b, tl.jacobi_operator(K, mask), 40 * n + 2000)
    assert info1 == 0 and info2 == 0
    return dict(it2=it2, it1=it1, err2=np.max(np.abs(y2 - u)) / scale, err1=np.max(np.abs(y1 - u)) / scale, y2=y2, u=u)


@pytest.mark.parametrize("mesh, n_agg, prototype", [("warren100", 32, 77), ("warren300", 64, 126), ("chain2000", 64, 242)])
def test_host_pipeline_iteration_counts_and_error(mesh, n_agg, prototype):
    """Measured here (two-level iterations, error | Jacobi iterations, error against spsolve):
      warren100/32   77  2.1e-11 |  979  2.0e-11      warren300/64  126  2.1e-10 | 5875  1.8e-10
      chain2000/64  242  3.0e-12 | 2000  3.0e-12"""
    nodes, el, loads, fixed, _, _ = (chain_mesh(2000) if mesh == "chain2000" else warren_mesh(int(mesh[6:])))
    r = _solve_pair(nodes, el, loads, fixed, n_agg)
    print(f"{mesh}/{n_agg}: two-level {r['it2']} iterations, error {r['err2']:.2e} | Jacobi {r['it1']} iterations, "
          f"error {r['err1']:.2e}")
    assert r["it2"] <= 1.25 * prototype
    assert r["err2"] <= 10 * r["err1"]


def test_shuffled_numbering():
    nodes, el, loads, fixed, _, _ = warren_mesh(300)
    base = _solve_pair(nodes, el, loads, fixed, 64)
    rng = np.random.default_rng(4)
    n_nodes = len(nodes)
    perm = rng.permutation(n_nodes)                       # new id k is old node perm[k]
    inv = np.empty(n_nodes, dtype=np.int64)
    inv[perm] = np.arange(n_nodes)
    nodes_s, el_s = nodes[perm], inv[el]
    loads_s = loads.reshape(-1, 2)[perm].reshape(-1)
    fixed_s = np.array([2 * inv[d // 2] + d % 2 for d in fixed])
    shuf = _solve_pair(nodes_s, el_s, loads_s, fixed_s, 64)
    print(f"warren300 unshuffled {base['it2']} | shuffled, coordinate aggregates {shuf['it2']}")
    assert abs(shuf["it2"] - base["it2"]) <= 2
    # aggregates as contiguous node-id ranges of the shuffled mesh: no gain, but the same solution
    ranges = (np.arange(n_nodes) * 64) // n_nodes
    bad = _solve_pair(nodes_s, el_s, loads_s, fixed_s, None, aggregates=ranges)
    print(f"          shuffled, node-id ranges {bad['it2']} (Jacobi {bad['it1']})")
    assert bad["err2"] <= 10 * bad["err1"]
    back = bad["y2"].reshape(-1, 2)[inv].reshape(-1)
    assert np.max(np.abs(back - base["u"])) <= 10 * max(bad["err1"], base["err1"]) * np.max(np.abs(base["u"]))


# ---- SolverConfig and the JSON namespace ----------------------------------------------------------------------------
def test_json_accel_options(tmp_path):
    import json
    from helpers import input_json
    from pinn_fem_amd.cli import generic as g
    from pinn_fem_amd.fem.solver import SolverConfig
    assert SolverConfig().nr_preconditioner == "jacobi" and SolverConfig().nr_aggregates is None
    with open(input_json("example1")) as f:
        data = json.load(f)
    cfg = g.parse_problem(input_json("example1"))["solver_config"]
    assert cfg.nr_preconditioner == "jacobi" and cfg.nr_aggregates is None
    for accel, want in (({"nr_preconditioner": "two-level", "nr_aggregates": 12}, ("two-level", 12)),
                        ({"nr_preconditioner": "two-level"}, ("two-level", None)), ({"nr_aggregates": 3}, ("jacobi", 3))):
        path = tmp_path / "p.json"
        path.write_text(json.dumps(dict(data, accel=accel)))
        cfg = g.parse_problem(str(path))["solver_config"]
        assert (cfg.nr_preconditioner, cfg.nr_aggregates) == want
    path.write_text(json.dumps(dict(data, accel={"nr_preconditioner": "multigrid"})))
    with pytest.raises(ValueError, match="multigrid"):
        g.parse_problem(str(path))
