"""The PATH form of the iteration graph (pf_graph_form_info: PF_GRAPH_FORM_FOLDED_RESIDUAL).

On a mesh whose elements form an open path in element order the captured graph has no residual launch: the fused backward
launch forms r and g_f of its elements' nodes itself (pf_node.h: path_residual), the residual's loss sums and the previous
iteration's bookkeeping ride in the theta-stage-1 launch (pf_mesh.hip: k_theta_stage1_path).  Eager launches keep
k_node_residual, so graph == eager, bit for bit, is the whole contract: u, theta, both optimisers' moments and every history
column except the u-norm monitor (which the PF_FUSED_U_UPDATE form already sums in another grouping)."""
import numpy as np
import pytest

from graph_driver import CHAIN_MASK, FOLDED, Expect, graph_vs_eager, material, path_model, ring, two_net_model

pytestmark = pytest.mark.gpu

PATH = Expect(CHAIN_MASK, FOLDED, ordered="ids")


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129])
@pytest.mark.parametrize("geom,fe", [("bar", 0), ("zigzag", 1)])
def test_path_graph_equals_eager_lane_and_task_edges(n, geom, fe):
    """One element, one lane beside the last, a full wave, one element past it, two tasks and one element: the edge lanes
    of a task (lane 0 reads element e-1, lane 63 element e+1) and the mesh's two end nodes.  alpha_physics = 0.37 so that
    g_f != r; measurements at every node."""
    graph_vs_eager(lambda: path_model(n, geom), PATH, fe=fe)


@pytest.mark.parametrize("geom,reverse,meas,fe,alpha_data", [
    ("zigzag", True, "third", 0, 100.0), ("zigzag", False, "all", 1, 100.0), ("bar", True, "all", 0, 0.0),
    ("bar1d", False, "third", 0, 100.0), ("bar1d", True, "all", 1, 100.0), ("bar", False, None, 1, 100.0)])
def test_path_graph_equals_eager_second_task(geom, reverse, meas, fe, alpha_data):
    """131137 elements = 2048 x 64 + 64 + 1: some waves of the backward launch take a second task, the last task holds one
    element.  Non-collinear geometry, a 1-D bar (one dof per node), node ids against the path, measurements at every node,
    at every third and none, the data term switched off (alpha_data = 0), both element-force formulations."""
    graph_vs_eager(lambda: path_model(131_137, geom, reverse=reverse, meas=meas), PATH, fe=fe, alpha_data=alpha_data)


@pytest.mark.parametrize("fe", [0, 1])
def test_path_graph_equals_eager_handicap_tasks(fe):
    """300000 elements on the collinear bar (the headline geometry): the elder waves of the backward launch take over tasks
    of their SIMD partners (PF_BW_SHIFT), replays of 20 iterations."""
    from pinn_fem_amd.engine import HipEngine
    assert HipEngine.GRAPH_ITERS_LARGE == 20
    graph_vs_eager(lambda: path_model(300_000, "bar", meas="third"), PATH, fe=fe)


@pytest.mark.parametrize("n,geom", [(4099, "zigzag"), (131_137, "bar")])
def test_path_chained_replays_equal_eager(n, geom):
    """Chained replays (PF_GRAPH_NO_TAIL, then PF_GRAPH_CONT_HEAD | PF_GRAPH_NO_TAIL) with the tail deferred to flush():
    iteration 0 of a continued replay books the last iteration of the replay before it from its theta-stage-1 launch."""
    graph_vs_eager(lambda: path_model(n, geom, reverse=True), PATH, mode="chained")


@pytest.mark.parametrize("max_it,tol,expect", [(40, 1e30, 12), (13, 0.0, 13), (15, 0.0, 15), (27, 0.0, 27)])
def test_path_stop_in_mid_replay_equals_eager(max_it, tol, expect):
    """The stop is raised by the bookkeeping block of a theta-stage-1 launch, one launch later than in the form with a
    residual launch: stop test met at iteration 12, max_iterations at odd counts and inside the second replay (replays of 20
    iterations).  State, moments and history end where the eager launches leave them."""
    graph_vs_eager(lambda: path_model(4099, "zigzag", meas="third"), PATH, mode="stop", graph_iters=20, max_it=max_it, tol=tol,
                   stop_at=expect)


# ---- form selection -------------------------------------------------------------------------------------------------------

def _shuffled_path(n):
    nodes = np.stack([np.arange(n + 1) * 0.1, np.zeros(n + 1)], 1)
    el = np.stack([np.arange(n), np.arange(1, n + 1)], 1)
    return nodes, el[np.random.default_rng(0).permutation(n)]


def _hub(n):
    a = 2 * np.pi * np.arange(n) / n
    nodes = np.concatenate([[[0.0, 0.0]], np.stack([np.cos(a), np.sin(a)], 1)])
    return nodes, np.stack([np.zeros(n, dtype=np.int64), np.arange(1, n + 1)], 1)


@pytest.mark.parametrize("kind", ["ring", "shuffled", "hub", "flipped-element", "warren", "ex3", "wide-net", "sharded"])
def test_other_meshes_keep_the_residual_launch(kind):
    """Everything that is not an open path in element order on the two-net one-chain problem reports the old form, and
    pf_fusion_info reports what it always did."""
    from bench import build_model
    from pinn_fem_amd.engine import HipEngine
    if kind == "sharded":
        from pinn_fem_amd.dist import build_shard_backend
        model, mv, md, _ = build_model(5000, "ex4")
        be = build_shard_backend(model, mv, md, 0, 2)
        assert be.eng.graph_form_info() == 0
        assert be.eng.fusion_info() & 16 == 0
        return
    mask = CHAIN_MASK
    if kind == "warren":
        model, mv, md, _ = build_model(5000, "ex4", mesh="warren")
    elif kind == "ex3":
        model, mv, md, _ = build_model(5000, "ex3")
        mask = 4
    elif kind == "wide-net":                                  # past the register buckets whose fused backward has the path form
        from pinn_fem_amd.fem.model import FEMModel
        m0, mv, md = path_model(500, "bar")
        model = FEMModel(m0.nodes, m0.elements, material(2, 27, 30), m0.loads, m0.fixed_dofs, dimension=2)
        mask = 1 + 2 + 4 + 16
    elif kind == "flipped-element":                           # a path as a graph, but one element runs against it
        nodes, el = np.stack([np.arange(301) * 0.1, np.zeros(301)], 1), np.stack([np.arange(300), np.arange(1, 301)], 1)
        el[137] = el[137][::-1]
        model, mv, md = two_net_model(nodes, el)
    else:
        model, mv, md = two_net_model(*{"ring": ring, "shuffled": _shuffled_path, "hub": _hub}[kind](300))
    eng = HipEngine(model, mv, md)
    assert eng.fusion_info() == mask
    assert eng.graph_form_info() == 0


def test_path_check_on_hand_made_connectivity():
    """The path-order check itself (pf_mesh.hip: k_path_check, through pf_graph_form_info) on small hand-made connectivity
    arrays: arbitrary node ids qualify, everything else does not."""
    from pinn_fem_amd.engine import HipEngine
    xy = lambda k: np.stack([np.arange(k) * 0.5, (np.arange(k) % 2) * 0.25], 1)
    cases = [
        ([[0, 1], [1, 2], [2, 3]], 4, True),                  # the plain path
        ([[2, 0], [0, 3], [3, 1]], 4, True),                  # node ids arbitrary
        ([[0, 1]], 2, True),                                  # one element
        ([[1, 0]], 2, True),
        ([[1, 2], [0, 1], [2, 3]], 4, False),                 # element order shuffled
        ([[0, 1], [2, 1], [2, 3]], 4, False),                 # one element against the path
        ([[0, 1], [1, 2], [2, 0]], 3, False),                 # closed ring
        ([[0, 1], [0, 2], [0, 3]], 4, False),                 # hub
        ([[0, 1], [1, 2], [1, 3]], 4, False),                 # branch
        ([[0, 1], [2, 3]], 4, False),                         # two pieces
        ([[0, 1], [1, 2], [0, 1]], 3, False),                 # a doubled element
    ]
    for el, nn, want in cases:
        model, mv, md = two_net_model(xy(nn), np.array(el))
        eng = HipEngine(model, mv, md)
        assert eng.fusion_info() == CHAIN_MASK, el
        assert eng.graph_form_info() == (FOLDED if want else 0), el
        del eng
