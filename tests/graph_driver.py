"""One driver for the graph-versus-eager tests of the GD iteration graph, and the models those tests share.

The contract every caller holds: replays of the captured graph end in the same bits as the same iterations launched eagerly —
u, theta, both pairs of Adam moments, the state tuple and every history column.  The one exception is the u-norm monitor
(history column 3) of a form with PF_FUSED_U_UPDATE: there the displacement update runs inside the forward launch and adds the
block partials of sum u_free^2 in another (fixed) grouping than the stand-alone kernel, the same sum to float32 round-off
(rtol 2e-6).  Every form without that bit runs the eager launches' kernel and is compared bit for bit in that column too."""
from dataclasses import dataclass
from typing import Optional, Union

import numpy as np
import torch

FOLDED = 1                        # pf_graph_form_info: PF_GRAPH_FORM_FOLDED_RESIDUAL
PF_FUSED_U_PINGPONG, PF_FUSED_U_UPDATE = 8, 16
CHAIN_MASK = 1 + 2 + 4 + 16       # pf_fusion_info of the two-net one-chain problem


# ---- models ---------------------------------------------------------------------------------------------------------------

def material(dim, we=20, wa=15, pos_e=True, pos_a=True, scale_e=1.5, scale_a=0.7):
    """E and A nets of two hidden layers, we / wa wide, seeded."""
    from pinn_fem_amd.fem.model import Material
    from pinn_fem_amd.fem.properties import NNProperty
    from pinn_fem_amd.nets import SimpleNN
    torch.manual_seed(5)
    return Material(NNProperty(SimpleNN(2, we, dim + 1), dim + 1, pos_e, scale_e),
                    NNProperty(SimpleNN(2, wa, dim + 1), dim + 1, pos_a, scale_a))


def path_model(n, geom="bar", reverse=False, meas="all", seed=3, zero_loads=False, **net):
    """A two-net model (20 / 15 wide; net: other arguments of material()) on an open path of n elements.  geom: "bar"
    (collinear, the headline geometry), "zigzag" (cs != 0), "bar1d" (one dof per node).  reverse: node ids run against the
    path.  Random loads; zero_loads: none at every second node.  Fixed dofs at both ends and one in the interior;
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
    if zero_loads:
        loads.reshape(n + 1, dim)[ids[pos % 2 == 0]] = 0.0
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
    return FEMModel(nodes, elements, material(dim, **net), loads, fixed, dimension=dim), mv, md


def zigzag(n, seed=3):
    """The zigzag path (c2, cs and s2 all live) with measurements at every third node (one element: at both)."""
    return path_model(n, "zigzag", meas="third" if n >= 2 else "all", seed=seed)


def warren(panels):
    """The two nets on a Warren girder (node degree 4): not a path."""
    from pinn_fem_amd.fem.model import FEMModel
    from pinn_fem_amd.plan import warren_mesh
    nodes, elements, loads, fixed, mv, md = warren_mesh(panels)
    return FEMModel(nodes, elements, material(2), loads, fixed, dimension=2), mv, md


def two_net_model(nodes, elements, seed=1):
    """The two nets on hand-made 2-D connectivity: random loads, nodes 1.. measured, node 0 fixed."""
    from pinn_fem_amd.fem.model import FEMModel
    rng = np.random.default_rng(seed)
    nn = len(nodes)
    loads = rng.normal(size=2 * nn) * 0.05
    md = np.arange(2, 2 * nn)
    mv = rng.normal(size=md.size) * 0.01
    return FEMModel(np.asarray(nodes, dtype=np.float64), np.asarray(elements), material(2), loads, np.array([0, 1]), dimension=2), mv, md


def ring(n):
    a = 2 * np.pi * np.arange(n) / n
    return np.stack([np.cos(a), np.sin(a)], 1), np.stack([np.arange(n), (np.arange(n) + 1) % n], 1)


def ids_follow_path(model):
    """Does element e join node e to node e + 1, for every e?  From the model's own connectivity."""
    el = np.asarray(model.elements)
    return bool(np.array_equal(el, np.stack([np.arange(len(el)), np.arange(1, len(el) + 1)], 1)))


# ---- the state and its comparison -----------------------------------------------------------------------------------------

def state(eng, rows):
    st = eng.state()
    return (eng.u.cpu().numpy().copy(), eng.theta.flat.cpu().numpy().copy(), eng.m_t.cpu().numpy().copy(),
            eng.v_t.cpu().numpy().copy(), eng.m_u.cpu().numpy().copy(), eng.v_u.cpu().numpy().copy(),
            (st.iter, st.done, st.converged, st.theta_half, st.u_half), eng.history(rows).copy())


def assert_history_same(mask, ha, hb):
    """The history comparison that the graph form `mask` (pf_fusion_info) promises."""
    assert ha.shape == hb.shape
    cols = [c for c in range(ha.shape[1]) if c != 3]        # every column except the u-norm monitor
    assert np.array_equal(ha[:, cols], hb[:, cols])
    if mask & PF_FUSED_U_UPDATE:
        assert np.allclose(ha[:, 3], hb[:, 3], rtol=2e-6, atol=0.0)
    else:
        assert np.array_equal(ha[:, 3], hb[:, 3])
    assert np.all(np.isfinite(ha))


def assert_same(a, b, mask, u_half=True):
    """Two state() tuples.  u_half=False: the state tuple without its last entry."""
    for x, y in zip(a[:-2], b[:-2]):
        assert np.array_equal(x, y)
        assert np.all(np.isfinite(x))
    assert (a[-2] == b[-2]) if u_half else (a[-2][:4] == b[-2][:4])
    assert_history_same(mask, a[-1], b[-1])


# ---- the driver -----------------------------------------------------------------------------------------------------------

@dataclass
class Expect:
    """What the library must report for the problem: pf_fusion_info, pf_graph_form_info, pf_graph_light_forward,
    pf_graph_ordered_path.  None: not asserted.  ordered = "ids": 1 where the form is FOLDED and the model's own
    connectivity has the node ids in path order (ids_follow_path), else 0."""
    mask: int
    form: Optional[int] = None
    light: Optional[int] = None
    ordered: Union[int, str, None] = None


def graph_vs_eager(make, expect, *, engine_kw=None, tweak=None, graph_iters=None, default_iters=None, fe=0,
                   load_factor=0.3, alpha_physics=0.37, alpha_data=100.0, mode="plain", remainder=3, max_it=200, tol=0.0,
                   stop_at=None, home=(), extra=None, graph_creates=None):
    """The same iterations through the captured graph and launched eagerly, from two fresh engines on make()'s model.
    mode "plain": two whole replays and `remainder` eager iterations; "chained": three chained replays, the tail deferred
    to flush(); "stop": two replays' worth asked for, a stop raised at iteration stop_at.
    engine_kw / fe: HipEngine arguments (fe=None: the engine's own fe_mode); tweak(eng.P): a change of the pf_problem record after begin() (the graph is
    captured from it).  graph_iters: replay length override; default_iters: the engine's own choice, asserted.
    alpha_physics, alpha_data: None keeps SolverConfig's.  home: names of state fields that must be 0 at the end.
    extra(eng, use_graph, n_it) -> [(name, array), ...]: further buffers, compared byte for byte.
    graph_creates: the graph run's count of captures (the eager run's is then 0)."""
    from pinn_fem_amd.engine import HipEngine
    from pinn_fem_amd.fem.solver import SolverConfig
    kw = dict(engine_kw or {})
    if fe is not None:
        kw["fe_mode"] = fe
    alphas = {k: v for k, v in (("alpha_physics", alpha_physics), ("alpha_data", alpha_data)) if v is not None}
    outs, bufs = [], []
    for use_graph in (True, False):
        model, mv, md = make()
        eng = HipEngine(model, mv, md, **kw)
        if tweak is None:
            assert eng.fusion_info() == expect.mask         # (no HIP call: valid before begin() as well)
        if default_iters is not None:
            assert eng.GRAPH_ITERS == default_iters          # the engine's own choice for this size
        if graph_iters is not None:
            eng.GRAPH_ITERS = graph_iters
        cfg = SolverConfig(max_iterations=max_it, tolerance=tol, learning_rate_u=0.01, learning_rate_theta=5e-4, **alphas)
        eng.begin(None, load_factor, cfg, want_history=True)
        if tweak is not None:
            tweak(eng.P)
        assert eng.fusion_info() == expect.mask
        if expect.form is not None:
            assert eng.graph_form_info() == expect.form
        if expect.light is not None:
            assert eng.graph_light_forward() == expect.light
        if expect.ordered is not None:
            want = int(expect.form == FOLDED and ids_follow_path(model)) if expect.ordered == "ids" else expect.ordered
            assert eng.graph_ordered_path() == want
        k = eng.GRAPH_ITERS
        if extra is not None or mode == "chained":
            assert k % 2 == 0                                # (the halves a hook reads; what a chained replay needs)
        if mode == "plain":
            n_it = 2 * k + remainder
            eng.iterate(n_it, use_graph=use_graph)
        elif mode == "chained":
            n_it = 3 * k
            if use_graph:
                assert eng.prepare_graph(chained=True)
                eng.iterate(n_it, defer_tail=True)
                torch.cuda.synchronize()
                assert eng.state().iter == n_it - 1          # the last iteration's bookkeeping is still pending
                eng.flush()
            else:
                eng.iterate(n_it, use_graph=False)
        else:
            assert mode == "stop" and stop_at is not None
            eng.iterate(2 * k, use_graph=use_graph)
            n_it = stop_at
        torch.cuda.synchronize()
        st = eng.state()
        assert st.iter == n_it
        if mode == "stop":
            assert st.done == 1
        for name in home:
            assert getattr(st, name) == 0, name
        if graph_creates is not None:
            assert eng.graph_creates == (graph_creates if use_graph else 0)
        outs.append(state(eng, n_it))
        if extra is not None:
            bufs.append(extra(eng, use_graph, n_it))
        del eng
    # a stop in mid-replay of the DAG with the displacement ping-pong: k_u_home copies the displacements home and leaves
    # state.u_half as the record of where they were, so u_half is no part of the result there
    assert_same(outs[0], outs[1], expect.mask, u_half=not (mode == "stop" and expect.mask & PF_FUSED_U_PINGPONG))
    if extra is not None:
        assert [name for name, _ in bufs[0]] == [name for name, _ in bufs[1]]
        for (name, a), (_, b) in zip(bufs[0], bufs[1]):
            assert a.tobytes() == b.tobytes(), name
            assert np.all(np.isfinite(a)), name
