"""Node tasks that address by node id on an ORDERED path (pf_graph_ordered_path).

Where the iteration graph runs its path form and the node ids follow the path (element e joins node e to node e + 1), the
displacement update inside the graph's forward launch forms every operand address of node n from n alone — the records of
elements n-1 and n, g_f at n-1, n and n+1 — instead of walking adj_ptr, adj and adj_other (pf_node.h: node_gradu_task_path).
Eager launches keep k_node_gradu with the gather, so graph == eager, byte for byte, is the contract once more: u, theta, both
pairs of Adam moments, the state tuple and every history column except the u-norm monitor (test_path_form.py: _assert_same).
A path with other node ids keeps the gather inside the graph as well and answers 0.

A node task is 128 nodes (PF_GU_M = 2 x 64) and a path of n elements has n + 1 nodes: n = 127 fills one task, 128 puts one
node into a second one, 63 / 64 sit at the wave edge inside a task, 255 .. 257 at the next task edge, 1023 .. 1025 at the
eighth; n = 1 and 2 are the meshes whose every node is an end node or the neighbour of two."""
import numpy as np
import pytest
import torch

from graph_driver import CHAIN_MASK, FOLDED, Expect, graph_vs_eager, path_model, ring, two_net_model

gpu = pytest.mark.gpu      # (per test: the declaration test at the end needs no GPU)


def _swapped_pair(n, geom="bar", meas="all"):
    """The ordered path of n elements with the ids of two interior nodes swapped: nodes, elements, loads, fixed and measured
    dofs renumbered together, so it is the same problem and still a path in element order, but conn[2e] != e at the pair."""
    from pinn_fem_amd.fem.model import FEMModel
    m0, mv, md = path_model(n, geom, meas=meas)
    dim = 1 if geom == "bar1d" else 2
    a, b = n // 3, n // 3 + 2
    assert 0 < a < b < n
    new_id = np.arange(n + 1)
    new_id[a], new_id[b] = b, a
    dof = (new_id[:, None] * dim + np.arange(dim)[None, :]).reshape(-1)        # old dof -> new dof
    nodes = np.empty_like(np.asarray(m0.nodes))
    nodes[new_id] = np.asarray(m0.nodes)
    loads = np.empty_like(np.asarray(m0.loads))
    loads[dof] = np.asarray(m0.loads)
    elements = new_id[np.asarray(m0.elements)]
    fixed = np.unique(dof[np.asarray(m0.fixed_dofs)])
    model = FEMModel(nodes, elements, m0.material, loads, fixed, dimension=dim)
    return model, mv, (None if md is None else dof[md])


ORDERED, GATHER = Expect(CHAIN_MASK, FOLDED, ordered=1), Expect(CHAIN_MASK, FOLDED, ordered=0)


@gpu
@pytest.mark.parametrize("n", [1, 2, 63, 64, 126, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 4099])
@pytest.mark.parametrize("geom,fe", [("bar", 0), ("zigzag", 1)])
def test_ordered_graph_equals_eager_node_task_and_end_node_edges(n, geom, fe):
    """The mesh's end nodes (one incidence each; n = 1: nothing but end nodes), the wave edge inside a task, one node short
    of a task, a full task, one and two nodes into the next one, and the same at the second and the eighth task edge."""
    graph_vs_eager(lambda: path_model(n, geom), ORDERED, fe=fe)


@gpu
@pytest.mark.parametrize("geom,meas,fe,alpha_data", [
    ("bar", "third", 0, 100.0), ("bar1d", "all", 0, 100.0), ("bar1d", "third", 1, 100.0), ("bar", None, 1, 100.0),
    ("bar", "all", 0, 0.0)])
def test_ordered_graph_equals_eager_block_partition(geom, meas, fe, alpha_data):
    """131137 elements: the forward launch's blocks hold several node tasks each and the last task holds few nodes.
    Measurements at every third node, one dof per node (a one-float record; both element-force formulations), no
    measurements, the data term switched off."""
    graph_vs_eager(lambda: path_model(131_137, geom, meas=meas), ORDERED, fe=fe, alpha_data=alpha_data)


@gpu
def test_ordered_chained_replays_equal_eager():
    """Chained replays with the tail deferred to flush(): a continuation head's node tasks read the records the replay before
    it left."""
    graph_vs_eager(lambda: path_model(4099, "zigzag"), ORDERED, mode="chained")


@gpu
def test_ordered_stop_in_mid_replay_equals_eager():
    """max_iterations met at an odd count inside a replay of 20."""
    graph_vs_eager(lambda: path_model(4099, "zigzag", meas="third"), ORDERED, mode="stop", graph_iters=20, max_it=13, stop_at=13)


@gpu
@pytest.mark.parametrize("n", [129, 4099])
@pytest.mark.parametrize("kind", ["reversed", "swapped-pair"])
def test_other_node_ids_keep_the_gather(kind, n):
    """A path whose node ids run against it, and one whose ids are in order except for two interior nodes: the path form
    with the gather, query 0, graph == eager."""
    make = (lambda: path_model(n, "zigzag", reverse=True)) if kind == "reversed" else (lambda: _swapped_pair(n, "zigzag"))
    graph_vs_eager(make, GATHER, fe=1)


@gpu
@pytest.mark.parametrize("kind", ["warren", "ring", "ex3"])
def test_query_is_zero_off_the_path_form(kind):
    from bench import build_model
    from pinn_fem_amd.engine import HipEngine
    if kind == "warren":
        model, mv, md, _ = build_model(5000, "ex4", mesh="warren")
    elif kind == "ex3":
        model, mv, md, _ = build_model(5000, "ex3")
    else:
        model, mv, md = two_net_model(*ring(300))
    eng = HipEngine(model, mv, md)
    assert eng.fusion_info() == (4 if kind == "ex3" else CHAIN_MASK)
    assert eng.graph_form_info() == 0
    assert eng.graph_ordered_path() == 0


@gpu
def test_u_norm_monitor_of_the_ordered_form():
    """The u-norm column is compared with eager nowhere (the stand-alone kernel groups its sum differently), so here it is
    held to a float64 sqrt(sum u_free^2).  Row 2k - 2 of two whole replays of k iterations is written from the node tasks of
    the second replay's last forward launch; an eager run of 2k - 1 iterations ends with the displacements of that row.
    Margin: one float32 summation of n terms in any grouping, relative 1e-5 (n = 4100 nodes: pairwise-grouped partial sums
    err by a few float32 ulps, 6e-8 each)."""
    from pinn_fem_amd.engine import HipEngine
    from pinn_fem_amd.fem.solver import SolverConfig
    cfg = SolverConfig(max_iterations=200, tolerance=0.0, learning_rate_u=0.01, learning_rate_theta=5e-4,
                       alpha_physics=0.37, alpha_data=100.0)
    model, mv, md = path_model(4099, "zigzag")
    eng = HipEngine(model, mv, md)
    eng.begin(None, 0.3, cfg, want_history=True)
    assert eng.graph_ordered_path() == 1
    k = eng.GRAPH_ITERS
    eng.iterate(2 * k, use_graph=True)
    torch.cuda.synchronize()
    got = float(eng.history(2 * k)[2 * k - 2, 3])
    del eng
    model, mv, md = path_model(4099, "zigzag")
    eng = HipEngine(model, mv, md)
    eng.begin(None, 0.3, cfg, want_history=True)
    eng.iterate(2 * k - 1, use_graph=False)
    torch.cuda.synchronize()
    u = eng.u.cpu().numpy().astype(np.float64)
    free = np.ones(u.size, dtype=bool)
    free[np.asarray(model.fixed_dofs)] = False
    want = float(np.sqrt(np.sum(u[free] ** 2)))
    print(f"u-norm of row {2 * k - 2}: graph {got!r}, float64 of the eager displacements {want!r}, "
          f"relative difference {abs(got - want) / want:.3e}")
    assert want > 0.0
    assert abs(got - want) <= 1e-5 * want


def test_header_and_binding_declare_the_query():
    """No GPU: the additive entry point is declared in the header and in the ctypes binding, and the ABI version stays 9."""
    import os
    import re
    import ctypes as C
    from pinn_fem_amd import _capi
    from pinn_fem_amd.engine import HipEngine
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pinnfem_hip.h")).read()
    assert _capi.PF_ABI_VERSION == 9 and re.search(r"#define PF_ABI_VERSION 9\b", header)
    assert re.search(r"\bint pf_graph_ordered_path\(const pf_problem\* p\);", header)
    assert "pf_graph_ordered_path" in _capi.SYMBOLS
    assert _capi.SYMBOLS["pf_graph_ordered_path"] == _capi.SYMBOLS["pf_graph_form_info"]
    assert _capi.SYMBOLS["pf_graph_ordered_path"][0] is C.c_int
    assert callable(HipEngine.graph_ordered_path)
