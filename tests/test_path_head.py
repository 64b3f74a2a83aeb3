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
import pytest

from graph_driver import CHAIN_MASK, FOLDED, Expect, graph_vs_eager, path_model

pytestmark = pytest.mark.gpu

PATH = Expect(CHAIN_MASK, FOLDED, ordered="ids")     # (alpha_physics = 0.37 in every run, so that g_f != r)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 128, 129])
@pytest.mark.parametrize("geom,fe", [("zigzag", 0), ("bar", 1)])
def test_head_lane_and_task_edges_other_pairing(n, geom, fe):
    """The pairing of geometry and fe_mode test_path_form.py leaves out: the zigzag (c2, cs, s2 all live) in the
    reference operation order, the collinear bar in the delta form.  One element, two, one lane beside a full wave, a full
    wave, one element past it, two full waves and one element past them."""
    graph_vs_eager(lambda: path_model(n, geom), PATH, fe=fe)


@pytest.mark.parametrize("n", [65, 129])
@pytest.mark.parametrize("fe", [0, 1])
def test_head_one_dof_per_node(n, fe):
    """The 1-D bar (one record entry, one dof per node, 8-bit flag loads) over a task boundary."""
    graph_vs_eager(lambda: path_model(n, "bar1d", meas="third"), PATH, fe=fe)


@pytest.mark.parametrize("fe", [0, 1])
def test_head_node_ids_against_the_path(fe):
    """Node ids run against the path: the edge lanes' far node and the j node's f_ext / flags come from descending ids."""
    graph_vs_eager(lambda: path_model(129, "zigzag", reverse=True), PATH, fe=fe)


@pytest.mark.parametrize("n", [64 * 17 + 1, 64])
@pytest.mark.parametrize("fe", [0, 1])
def test_head_last_element_on_an_edge_lane(n, fe):
    """64 * 17 + 1: the mesh's last element sits on lane 0 of a task of its own, so it reads element e-1 AND owns its j
    node (`last` and lane 0 coincide; with one element per task `first` cannot, n = 1 above holds that).  64: the last
    element sits on lane 63."""
    graph_vs_eager(lambda: path_model(n, "zigzag", meas="third"), PATH, fe=fe)


def test_head_chained_replays_default_length():
    """4100 elements, the engine's own replay length (10 below 200000 elements), three chained replays: iteration 0 of a
    continued replay runs the head on what the replay before it left.  (65 tasks on 9 blocks: every wave has one task; a
    handicap task needs more than 131072 elements, see below.)"""
    graph_vs_eager(lambda: path_model(4100, "zigzag", reverse=True), PATH, mode="chained", default_iters=10)


def test_head_handicap_tasks_zigzag():
    """64 * (2048 + 8) + 1 elements: the launch has 2048 waves, waves 4..7 of block 0 hold a second task, and each elder
    wave 0..3 takes its partner's (PF_BW_SHIFT: (2 * 2 + 4) >> 3 = 1 task of a column of 2) — a handicap task runs the head
    on a zigzag; test_path_form.py holds the collinear bar at 300000."""
    graph_vs_eager(lambda: path_model(64 * (2048 + 8) + 1, "zigzag", meas="third"), PATH, fe=0)


@pytest.mark.parametrize("fe", [0, 1])
def test_head_exact_zeros(fe):
    """u starts at 0 and every second node carries no load: in the first iteration every row product is an exact zero, and
    the negated rows are zeros of the other sign; `0 + x` at the head of every sum must absorb them (r, g_f and the
    displacement update of an unloaded node keep their bits)."""
    graph_vs_eager(lambda: path_model(129, "zigzag", zero_loads=True), PATH, fe=fe)
