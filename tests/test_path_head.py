"""The task head of the path-form backward launch (pf_node.h: path_residual; pf_net32.hip: task_fetch_b_path, task_gea).

The head takes an element's j-end rows as its negated i-end rows, evaluates the neighbouring element once per task with
per-lane operands (lane 0: e-1, lane 63: e+1), moves values one lane up / down with whole-wave DPP shifts (across the row
boundaries at lanes 15/16, 31/32, 47/48) and loads everything its edge lanes need under one predicate.  The contract is
that of test_path_form.py: the path-form graph equals the eager launches (which keep k_node_residual), bit for bit, in u,
theta, both optimisers' moments, the state tuple and every history column except the u-norm monitor (rtol 2e-6).

The cases are the small ones test_path_form.py does not hold: the other pairing of geometry and fe_mode at the lane and
task edges (all three record entries live in the reference operation order), the 1-D bar and reversed node ids at these
sizes, a lane-0 element that is the mesh's last one, chained replays at the default replay length, handicap tasks on a
zigzag, and exact zeros (u = 0, half of the loads zero) through the negations.  Every lane carries its own random load."""
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


def _path_model(n, geom="bar", reverse=False, meas="all", seed=3, zero_loads=False):
    """A two-net model (20 / 15 wide) on an open path of n elements.  geom: "bar" (collinear), "zigzag" (cs != 0), "bar1d"
    (one dof per node).  reverse: node ids run against the path.  Random loads; zero_loads: none at every second node.
    Fixed dofs at both ends and one in the interior; measurements at every node ("all") or at every third ("third")."""
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
    if zero_loads:
        loads.reshape(n + 1, dim)[ids[pos % 2 == 0]] = 0.0
    fixed = [ids[0] * dim + c for c in range(dim)] + [ids[n] * dim + dim - 1]
    if n >= 2:
        fixed.append(ids[n // 2] * dim + dim - 1)
    fixed = np.unique(np.array(fixed))
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


def _graph_vs_eager(make, fe=0, chained=False, default_replays=None):
    """Two whole replays and an eager remainder of 3 (chained: three chained replays, the tail deferred to flush())
    against the same iterations launched eagerly.  alpha_physics = 0.37, so that g_f != r."""
    from pinn_fem_amd.engine import HipEngine
    from pinn_fem_amd.fem.solver import SolverConfig
    outs = []
    for use_graph in (True, False):
        model, mv, md = make()
        eng = HipEngine(model, mv, md, fe_mode=fe)
        if default_replays is not None:
            assert eng.GRAPH_ITERS == default_replays        # the engine's own choice for this size
        cfg = SolverConfig(max_iterations=200, tolerance=0.0, learning_rate_u=0.01, learning_rate_theta=5e-4,
                           alpha_physics=0.37, alpha_data=100.0)
        eng.begin(None, 0.3, cfg, want_history=True)
        assert eng.fusion_info() == CHAIN_MASK
        assert eng.graph_form_info() == FOLDED
        k = eng.GRAPH_ITERS
        if chained:
            n_it = 3 * k
            if use_graph:
                assert eng.prepare_graph(chained=True)
                eng.iterate(n_it, defer_tail=True)
                eng.flush()
            else:
                eng.iterate(n_it, use_graph=False)
        else:
            n_it = 2 * k + 3
            eng.iterate(n_it, use_graph=use_graph)
        torch.cuda.synchronize()
        assert eng.state().iter == n_it
        outs.append(_state(eng, n_it))
        del eng
    _assert_same(outs[0], outs[1])


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 128, 129])
@pytest.mark.parametrize("geom,fe", [("zigzag", 0), ("bar", 1)])
def test_head_lane_and_task_edges_other_pairing(n, geom, fe):
    """The pairing of geometry and fe_mode test_path_form.py leaves out: the zigzag (c2, cs, s2 all live) in the
    reference operation order, the collinear bar in the delta form.  One element, two, one lane beside a full wave, a full
    wave, one element past it, two full waves and one element past them."""
    _graph_vs_eager(lambda: _path_model(n, geom), fe=fe)


@pytest.mark.parametrize("n", [65, 129])
@pytest.mark.parametrize("fe", [0, 1])
def test_head_one_dof_per_node(n, fe):
    """The 1-D bar (one record entry, one dof per node, 8-bit flag loads) over a task boundary."""
    _graph_vs_eager(lambda: _path_model(n, "bar1d", meas="third"), fe=fe)


@pytest.mark.parametrize("fe", [0, 1])
def test_head_node_ids_against_the_path(fe):
    """Node ids run against the path: the edge lanes' far node and the j node's f_ext / flags come from descending ids."""
    _graph_vs_eager(lambda: _path_model(129, "zigzag", reverse=True), fe=fe)


@pytest.mark.parametrize("n", [64 * 17 + 1, 64])
@pytest.mark.parametrize("fe", [0, 1])
def test_head_last_element_on_an_edge_lane(n, fe):
    """64 * 17 + 1: the mesh's last element sits on lane 0 of a task of its own, so it reads element e-1 AND owns its j
    node (`last` and lane 0 coincide; with one element per task `first` cannot, n = 1 above holds that).  64: the last
    element sits on lane 63."""
    _graph_vs_eager(lambda: _path_model(n, "zigzag", meas="third"), fe=fe)


def test_head_chained_replays_default_length():
    """4100 elements, the engine's own replay length (10 below 200000 elements), three chained replays: iteration 0 of a
    continued replay runs the head on what the replay before it left.  (65 tasks on 9 blocks: every wave has one task; a
    handicap task needs more than 131072 elements, see below.)"""
    _graph_vs_eager(lambda: _path_model(4100, "zigzag", reverse=True), chained=True, default_replays=10)


def test_head_handicap_tasks_zigzag():
    """64 * (2048 + 8) + 1 elements: the launch has 2048 waves, waves 4..7 of block 0 hold a second task, and each elder
    wave 0..3 takes its partner's (PF_BW_SHIFT: (2 * 2 + 4) >> 3 = 1 task of a column of 2) — a handicap task runs the head
    on a zigzag; test_path_form.py holds the collinear bar at 300000."""
    _graph_vs_eager(lambda: _path_model(64 * (2048 + 8) + 1, "zigzag", meas="third"), fe=0)


@pytest.mark.parametrize("fe", [0, 1])
def test_head_exact_zeros(fe):
    """u starts at 0 and every second node carries no load: in the first iteration every row product is an exact zero, and
    the negated rows are zeros of the other sign; `0 + x` at the head of every sum must absorb them (r, g_f and the
    displacement update of an unloaded node keep their bits)."""
    _graph_vs_eager(lambda: _path_model(129, "zigzag", zero_loads=True), fe=fe)
