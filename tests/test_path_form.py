"""The PATH form of the iteration graph (pf_graph_form_info: PF_GRAPH_FORM_FOLDED_RESIDUAL).

On a mesh whose elements form an open path in element order the captured graph has no residual launch: the fused backward
launch forms r and g_f of its elements' nodes itself (pf_node.h: path_residual), the residual's loss sums and the previous
iteration's bookkeeping ride in the theta-stage-1 launch (pf_mesh.hip: k_theta_stage1_path).  Eager launches keep
k_node_residual, so graph == eager, bit for bit, is the whole contract: u, theta, both optimisers' moments and every history
column except the u-norm monitor (which the PF_FUSED_U_UPDATE form already sums in another grouping)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FOLDED = 1
CHAIN_MASK = 1 + 2 + 4 + 16


def _nets(dim, we=20, wa=15):
    from pinn_fem_amd.fem.model import Material
    from pinn_fem_amd.fem.properties import NNProperty
    from pinn_fem_amd.nets import SimpleNN
    torch.manual_seed(5)
    return Material(NNProperty(SimpleNN(2, we, dim + 1), dim + 1, True, 1.5), NNProperty(SimpleNN(2, wa, dim + 1), dim + 1, True, 0.7))


def _path_model(n, geom="bar", reverse=False, meas="all", seed=3):
    """A two-net model on an open path of n elements.  geom: "bar" (collinear, the headline geometry), "zigzag" (cs != 0),
    "bar1d" (one dof per node).  reverse: node ids run against the path.  Fixed dofs at both ends and one in the interior;
    measurements at every node ("all"), at every third ("third") or none (None)."""
    from pinn_fem_amd.fem.model import FEMModel
    rng = np.random.default_rng(seed)
    dim = 1 if geom == "bar1d" else 2
    pos = np.arange(n + 1)                                   # position along the path -> node id
    ids = pos[::-1].copy() if reverse else pos
    x = np.concatenate([[0.0], np.cumsum(rng.uniform(0.5, 1.5, n))]) * (3.0 / max(n, 1))
    if dim == 1:
        nodes = np.zeros(n + 1)
        nodes[ids] = x
    else:
        nodes = np.zeros((n + 1, 2))
        nodes[ids, 0] = x
        if geom == "zigzag":
            nodes[ids, 1] = (pos % 2) * (0.7 * 3.0 / max(n, 1)) + 0.1 * x
    elements = np.stack([ids[:-1], ids[1:]], 1)
    ndof = (n + 1) * dim
    loads = rng.normal(size=ndof) * 0.1
    fixed = [ids[0] * dim + c for c in range(dim)] + [ids[n] * dim + dim - 1]
    if n >= 2:
        fixed.append(ids[n // 2] * dim + dim - 1)
    fixed = np.unique(np.array(fixed))
    if meas is None:
        mv = md = None
    else:
        nd = ids[pos % 3 == 1] if meas == "third" else ids
        md = (nd[:, None] * dim + np.arange(dim)[None, :]).reshape(-1)
        mv = rng.normal(size=md.size) * 0.02
    return FEMModel(nodes, elements, _nets(dim), loads, fixed, dimension=dim), mv, md


def _state(eng, rows):
    st = eng.state()
    return (eng.u.cpu().numpy().copy(), eng.theta.flat.cpu().numpy().copy(), eng.m_t.cpu().numpy().copy(),
            eng.v_t.cpu().numpy().copy(), eng.m_u.cpu().numpy().copy(), eng.v_u.cpu().numpy().copy(),
            (st.iter, st.done, st.converged, st.theta_half, st.u_half), eng.history(rows).copy())


def _assert_same(a, b):
    for x, y in zip(a[:-2], b[:-2]):
        assert np.array_equal(x, y)
    assert a[-2] == b[-2]
    ha, hb = a[-1], b[-1]
    assert ha.shape == hb.shape
    cols = [c for c in range(ha.shape[1]) if c != 3]        # every column except the u-norm monitor
    assert np.array_equal(ha[:, cols], hb[:, cols])
    assert np.allclose(ha[:, 3], hb[:, 3], rtol=2e-6, atol=0.0)
    assert np.all(np.isfinite(ha))


def _graph_vs_eager(make, fe=0, alpha_physics=0.37, alpha_data=100.0, mode="plain", graph_iters=None, max_it=200, tol=0.0,
                    expect=None):
    from pinn_fem_amd.engine import HipEngine
    from pinn_fem_amd.fem.solver import SolverConfig
    outs = []
    for use_graph in (True, False):
        model, mv, md = make()
        eng = HipEngine(model, mv, md, fe_mode=fe)
        if graph_iters is not None:
            eng.GRAPH_ITERS = graph_iters
        cfg = SolverConfig(max_iterations=max_it, tolerance=tol, learning_rate_u=0.01, learning_rate_theta=5e-4,
                           alpha_physics=alpha_physics, alpha_data=alpha_data)
        eng.begin(None, 0.3, cfg, want_history=True)
        assert eng.fusion_info() == CHAIN_MASK
        assert eng.graph_form_info() == FOLDED
        k = eng.GRAPH_ITERS
        if mode == "plain":                                  # two whole replays and an eager remainder
            n_it = 2 * k + 3
            eng.iterate(n_it, use_graph=use_graph)
        elif mode == "chained":                              # three chained replays, the tail deferred to flush()
            n_it = 3 * k
            if use_graph:
                assert eng.prepare_graph(chained=True)
                eng.iterate(n_it, defer_tail=True)
                torch.cuda.synchronize()
                assert eng.state().iter == n_it - 1          # the last iteration's bookkeeping is still pending
                eng.flush()
            else:
                eng.iterate(n_it, use_graph=False)
        else:                                                # a stop raised in mid-replay
            eng.iterate(2 * k, use_graph=use_graph)
            n_it = expect
        torch.cuda.synchronize()
        st = eng.state()
        assert st.iter == n_it
        if mode == "stop":
            assert st.done == 1
        outs.append(_state(eng, n_it))
        del eng
    _assert_same(outs[0], outs[1])


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129])
@pytest.mark.parametrize("geom,fe", [("bar", 0), ("zigzag", 1)])
def test_path_graph_equals_eager_lane_and_task_edges(n, geom, fe):
    """One element, one lane beside the last, a full wave, one element past it, two tasks and one element: the edge lanes
    of a task (lane 0 reads element e-1, lane 63 element e+1) and the mesh's two end nodes.  alpha_physics = 0.37 so that
    g_f != r; measurements at every node."""
    _graph_vs_eager(lambda: _path_model(n, geom), fe=fe)


@pytest.mark.parametrize("geom,reverse,meas,fe,alpha_data", [
    ("zigzag", True, "third", 0, 100.0), ("zigzag", False, "all", 1, 100.0), ("bar", True, "all", 0, 0.0),
    ("bar1d", False, "third", 0, 100.0), ("bar1d", True, "all", 1, 100.0), ("bar", False, None, 1, 100.0)])
def test_path_graph_equals_eager_second_task(geom, reverse, meas, fe, alpha_data):
    """131137 elements = 2048 x 64 + 64 + 1: some waves of the backward launch take a second task, the last task holds one
    element.  Non-collinear geometry, a 1-D bar (one dof per node), node ids against the path, measurements at every node,
    at every third and none, the data term switched off (alpha_data = 0), both element-force formulations."""
    _graph_vs_eager(lambda: _path_model(131_137, geom, reverse=reverse, meas=meas), fe=fe, alpha_data=alpha_data)


@pytest.mark.parametrize("fe", [0, 1])
def test_path_graph_equals_eager_handicap_tasks(fe):
    """300000 elements on the collinear bar (the headline geometry): the elder waves of the backward launch take over tasks
    of their SIMD partners (PF_BW_SHIFT), replays of 20 iterations."""
    from pinn_fem_amd.engine import HipEngine
    assert HipEngine.GRAPH_ITERS_LARGE == 20
    _graph_vs_eager(lambda: _path_model(300_000, "bar", meas="third"), fe=fe)


@pytest.mark.parametrize("n,geom", [(4099, "zigzag"), (131_137, "bar")])
def test_path_chained_replays_equal_eager(n, geom):
    """Chained replays (PF_GRAPH_NO_TAIL, then PF_GRAPH_CONT_HEAD | PF_GRAPH_NO_TAIL) with the tail deferred to flush():
    iteration 0 of a continued replay books the last iteration of the replay before it from its theta-stage-1 launch."""
    _graph_vs_eager(lambda: _path_model(n, geom, reverse=True), mode="chained")


@pytest.mark.parametrize("max_it,tol,expect", [(40, 1e30, 12), (13, 0.0, 13), (15, 0.0, 15), (27, 0.0, 27)])
def test_path_stop_in_mid_replay_equals_eager(max_it, tol, expect):
    """The stop is raised by the bookkeeping block of a theta-stage-1 launch, one launch later than in the form with a
    residual launch: stop test met at iteration 12, max_iterations at odd counts and inside the second replay (replays of 20
    iterations).  State, moments and history end where the eager launches leave them."""
    _graph_vs_eager(lambda: _path_model(4099, "zigzag", meas="third"), mode="stop", graph_iters=20, max_it=max_it, tol=tol,
                    expect=expect)


# ---- form selection -------------------------------------------------------------------------------------------------------

def _two_net_model(nodes, elements, seed=1):
    from pinn_fem_amd.fem.model import FEMModel
    rng = np.random.default_rng(seed)
    nn = len(nodes)
    loads = rng.normal(size=2 * nn) * 0.05
    md = np.arange(2, 2 * nn)
    mv = rng.normal(size=md.size) * 0.01
    return FEMModel(np.asarray(nodes, dtype=np.float64), np.asarray(elements), _nets(2), loads, np.array([0, 1]), dimension=2), mv, md


def _ring(n):
    a = 2 * np.pi * np.arange(n) / n
    return np.stack([np.cos(a), np.sin(a)], 1), np.stack([np.arange(n), (np.arange(n) + 1) % n], 1)


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
        m0, mv, md = _path_model(500, "bar")
        model = FEMModel(m0.nodes, m0.elements, _nets(2, 27, 30), m0.loads, m0.fixed_dofs, dimension=2)
        mask = 1 + 2 + 4 + 16
    elif kind == "flipped-element":                           # a path as a graph, but one element runs against it
        nodes, el = np.stack([np.arange(301) * 0.1, np.zeros(301)], 1), np.stack([np.arange(300), np.arange(1, 301)], 1)
        el[137] = el[137][::-1]
        model, mv, md = _two_net_model(nodes, el)
    else:
        model, mv, md = _two_net_model(*{"ring": _ring, "shuffled": _shuffled_path, "hub": _hub}[kind](300))
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
        model, mv, md = _two_net_model(xy(nn), np.array(el))
        eng = HipEngine(model, mv, md)
        assert eng.fusion_info() == CHAIN_MASK, el
        assert eng.graph_form_info() == (FOLDED if want else 0), el
        del eng
