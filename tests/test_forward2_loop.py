"""The element-task loop of the fused forward launch (pf_net32.hip: k_net32_forward2).

The loop keeps its counters in scalar registers, loads a task's own geometry at the task's head, requests the NEXT task's
coordinates in every task (behind the half-wave exchange, with a clamped element index: past a block's last task the loads
are valid and unread) and reads its base pointers from the kernel argument task by task.  No value changes.  The contract is
that of test_path_head.py: graph replays equal the same iterations launched eagerly, bit for bit, in u, theta, both
optimisers' moments, the state tuple and every history column except the u-norm monitor (rtol 2e-6).

Sizes are the ones at which this loop can go wrong: the launch has 256 blocks of 16 waves, an element task is 64 elements,
a node task 128 nodes.  The one-net launch (k_net32_forward: the ex3 shape, E = NN, A a constant) got the same treatment
of its rounds and is held the same way.  Eager launches run the same loop, so graph == eager cannot see an error common to
both: one test holds E, A and the stiffness records of one eager forward against a float64 evaluation of the oracle's
formulas."""
import inspect

import numpy as np
import pytest
import torch

from graph_driver import CHAIN_MASK, FOLDED, Expect, graph_vs_eager
from graph_driver import warren as _warren, zigzag as _zigzag

pytestmark = pytest.mark.gpu

# (every run below: fe_mode 0, alpha_physics = 0.37 so that g_f != r; ordered: from the model's own connectivity)
PATH = Expect(CHAIN_MASK, FOLDED, ordered="ids")
# a mesh that is not a path: the same fused launches, no folded residual (read from the parent commit's library on the
# Warren girders below: pf_fusion_info 23, pf_graph_form_info 0)
WARREN = Expect(23, 0, ordered="ids")
# one net: only the parameter update rides in the forward launch; from 200000 elements on the graph is the DAG with two
# displacement vectors (read from the parent commit's library as well)
ONE_NET, ONE_NET_DAG = Expect(4, 0, ordered="ids"), Expect(4 + 8, 0, ordered="ids")


def _one_net(n, seed=3):
    """The ex3 shape on the zigzag path: E from a 20-wide net, A a constant."""
    from pinn_fem_amd.fem.model import FEMModel, Material
    from pinn_fem_amd.fem.properties import NNProperty
    from pinn_fem_amd.nets import SimpleNN
    two, mv, md = _zigzag(n, seed)
    torch.manual_seed(5)
    mat = Material(NNProperty(SimpleNN(2, 20, 3), 3, True, 1.5), 0.7)
    return FEMModel(two.nodes, two.elements, mat, two.loads, two.fixed_dofs, dimension=2), mv, md


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_loop_lane_and_task_edges(n):
    """A single lane, a lane tail, exactly one task, a second task of one element (every other wave of block 0 requests
    clamped coordinates nobody reads)."""
    graph_vs_eager(lambda: _zigzag(n), PATH)


def test_loop_blocks_with_and_without_tasks():
    """4100 elements: 65 element tasks, one per block for 65 blocks, the rest of the grid with none; 33 node tasks: blocks
    with both kinds of task, with element tasks only, and with nothing."""
    graph_vs_eager(lambda: _zigzag(4100), PATH)


@pytest.mark.parametrize("n", [262144, 262144 + 64])
def test_loop_one_task_per_wave(n):
    """262144: every wave of the grid has exactly one task and no draw from the queue succeeds.  64 more: 4097 tasks, 17 per
    block on 241 blocks, each with one wave that draws a second task."""
    graph_vs_eager(lambda: _zigzag(n), PATH)


def test_loop_several_draws_per_wave():
    """131585 elements (test_path_head.py's handicap size): 2057 tasks, 9 per block on 228 blocks and 5 on the last, several
    draws per block, and the unconditional request past t1 in every block."""
    graph_vs_eager(lambda: _zigzag(131585), PATH)


@pytest.mark.parametrize("panels", [300, 3000])
def test_loop_warren_girder(panels):
    """A mesh that is not a path (Warren girder, node degree 4): the four-launch form, whose forward launch carries
    degree-4 node tasks beside the element tasks."""
    graph_vs_eager(lambda: _warren(panels), WARREN)


@pytest.mark.parametrize("mesh", ["zigzag4100", "warren3000"])
def test_loop_chained_replays(mesh):
    """Three chained replays, the tail deferred to flush(): iteration 0 of a continued replay runs the loop on what the
    replay before it left."""
    if mesh == "zigzag4100":
        graph_vs_eager(lambda: _zigzag(4100), PATH, mode="chained")
    else:
        graph_vs_eager(lambda: _warren(3000), WARREN, mode="chained")


@pytest.mark.parametrize("n", [65, 4100, 100000, 262144 + 65])
def test_one_net_rounds(n):
    """k_net32_forward (E = NN, A constant): one task and a second of one element, 65 tasks, the ex3 side configuration's
    size (1563 tasks on 4096 waves: one round), and 4098 tasks on 4096 waves: a second round in which two waves of block 0
    work and every other wave holds clamped coordinates, with the lockstep barriers of both rounds."""
    graph_vs_eager(lambda: _one_net(n), ONE_NET_DAG if n >= 200000 else ONE_NET)


def test_forward_values_against_float64():
    """E, A and the stiffness records after ONE eager forward (the forward of pf_loss_and_grads: k_net32_forward2 without
    the update prologue) on the 4100-element zigzag, against the oracle's formulas (properties.py:97-161,
    nn_assembly.py:74, :84-94) evaluated in float64 on the oracle's own float32 inputs.  The tolerance is the one
    test_hip_parity.py applies to what is formed from these quantities, the internal force: _check_step's tol_f, relative to
    the quantity's largest magnitude (helpers.rel_err)."""
    import test_hip_parity
    from helpers import orc, rel_err
    from pinn_fem_amd.engine import HipEngine
    tol = inspect.signature(test_hip_parity._check_step).parameters["tol_f"].default
    assert tol == 2e-6
    n, lam = 4100, 0.3
    model, mv, md = _zigzag(n)
    nets = [[p.detach().double().numpy() for p in prop.net.parameters()] for prop in (model.material.young, model.material.area)]
    pb = orc.Problem(nodes=model.nodes, elements=model.elements, loads=model.loads, fixed_dofs=model.fixed_dofs, dimension=2)
    geo = orc.element_geometry(pb)
    x = orc.nn_inputs(geo, lam).astype(np.float64)

    def prop64(t, scale):
        h = x
        for l in range(2):
            h = np.tanh(h @ t[2 * l].T + t[2 * l + 1])
        z = (h @ t[4].T + t[5])[:, 0]
        return np.logaddexp(0.0, z) * scale

    e_ref, a_ref = prop64(nets[0], 1.5), prop64(nets[1], 0.7)
    s = e_ref * a_ref / geo.l0.astype(np.float64)
    pat = geo.pattern.astype(np.float64)
    k_ref = np.stack([s * pat[:, 0, 0], s * pat[:, 0, 1], s * pat[:, 1, 1]], 1)
    eng = HipEngine(model, mv, md, fe_mode=0)
    assert eng.fusion_info() & 1                             # both nets in one launch
    u = torch.zeros(2 * (n + 1))
    eng.loss_and_grads(u, lam, 0.37, 100.0)
    torch.cuda.synchronize()
    e_got = eng.prop_e[:n].cpu().numpy()
    a_got = eng.prop_a[:n].cpu().numpy()
    k_got = eng.elem_k[:3 * n].cpu().numpy().reshape(n, 3)
    errs = (rel_err(e_got, e_ref), rel_err(a_got, a_ref), rel_err(k_got, k_ref))
    print("rel_err E, A, records:", errs)
    assert errs[0] < tol
    assert errs[1] < tol
    assert errs[2] < tol
    del eng
    # the one-net launch on the same mesh and the same E net: E and the records with the constant area
    model1, mv1, md1 = _one_net(n)
    eng = HipEngine(model1, mv1, md1, fe_mode=0)
    assert not eng.fusion_info() & 1
    eng.loss_and_grads(u, lam, 0.37, 100.0)
    torch.cuda.synchronize()
    k1_ref = k_ref * (0.7 / a_ref)[:, None]
    errs1 = (rel_err(eng.prop_e[:n].cpu().numpy(), e_ref), rel_err(eng.elem_k[:3 * n].cpu().numpy().reshape(n, 3), k1_ref))
    print("one net: rel_err E, records:", errs1)
    assert errs1[0] < tol
    assert errs1[1] < tol
