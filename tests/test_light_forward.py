"""The LIGHT FORWARD of the iteration graph's path form (pf_graph_light_forward).

Where the graph runs the path form with both nets in the split-f16 engine, its forward launch evaluates the E net only for the
first and the last element of every 64-element task (packed 64 to a wave into edge tasks) and stores prop_a and those
elements' stiffness records; the fused backward launch, which recomputes the E net's hidden layers anyway, forms E itself and
stores prop_e and every other record.  Eager launches keep the full forward, so graph == eager, byte for byte, is the
contract again: the state tuple of test_path_form.py, and beside it the buffers whose writer changed.

Which half is compared.  Properties and records ping-pong between two halves inside a replay; eager launches use the first.
Iteration t (0-based) of a run writes half t & 1 in a replay of an even number of iterations.  A run of n iterations that
ends with eager launches (the plain mode's remainder) leaves the last iteration's values in the first half in both runs.  A
run that ends inside or at the end of a replay (chained replays with flush(), a stop in mid-replay) leaves the values of
iteration n - 1 — what the eager run holds in its first half — in half (n - 1) & 1.  After a stop in mid-replay the graph has
run one more forward / backward pair than the eager launches (the stop is raised behind the backward launch: the other half,
g_ea and g_f are scratch there, as before this form), so g_ea and g_f are compared in the other two modes only."""
import pytest

from graph_driver import CHAIN_MASK, FOLDED, Expect, graph_vs_eager, path_model, ring, two_net_model

gpu = pytest.mark.gpu      # (per test: the declaration test at the end needs no GPU)


def _buffers(eng, half, with_adjoint):
    """prop_e, prop_a and the stiffness records of one half, and (with_adjoint) g_ea and g_f, as bytes-exact arrays."""
    ne = eng.plan.n_elems
    kw = 3 if eng.plan.dim == 2 else 1
    out = [("prop_e", eng.prop_e[half * ne:(half + 1) * ne]), ("prop_a", eng.prop_a[half * ne:(half + 1) * ne]),
           ("elem_k", eng.elem_k[half * ne * kw:(half + 1) * ne * kw])]
    if with_adjoint:
        out += [("g_ea", eng.g_ea[:ne]), ("g_f", eng.g_f)]
    return [(name, t.cpu().numpy().copy()) for name, t in out]


def _light_vs_eager(make, fe=0, mode="plain", light=1, form=FOLDED, **kw):
    """The shared driver, with the buffers of the half that holds the last iteration's values (module docstring)."""
    def extra(eng, use_graph, n_it):
        half = (n_it - 1) & 1 if use_graph and mode != "plain" else 0
        return _buffers(eng, half, mode != "stop")
    graph_vs_eager(make, Expect(CHAIN_MASK, form, light=light, ordered="ids"), fe=fe, mode=mode, extra=extra, **kw)


@gpu
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 127, 128, 129, 2047, 2048, 2049, 4099])
@pytest.mark.parametrize("geom,fe", [("bar", 0), ("zigzag", 1)])
def test_light_graph_equals_eager_task_and_wave_edges(n, geom, fe):
    """Task edges (63 .. 65, 127 .. 129), the mesh's two ends (1, 2), n not a multiple of 64, and 2048 elements = 32 tasks,
    where the packed edge elements first fill a whole wave (2047: one short, 2049: one slot of a second edge task)."""
    _light_vs_eager(lambda: path_model(n, geom), fe=fe)


@gpu
@pytest.mark.parametrize("geom,reverse,fe", [("bar1d", False, 1), ("zigzag", True, 0)])
def test_light_graph_equals_eager_1d_and_reversed_ids(geom, reverse, fe):
    """One dof per node (a one-float stiffness record), and node ids running against the path."""
    _light_vs_eager(lambda: path_model(4099, geom, reverse=reverse, meas="third"), fe=fe)


@gpu
def test_light_graph_equals_eager_second_task():
    """131137 elements = 2048 x 64 + 64 + 1: the elder waves of the backward launch take extra tasks (PF_BW_SHIFT), some
    blocks of the forward launch hold more than one edge task, the last task holds one element."""
    _light_vs_eager(lambda: path_model(131_137, "bar", meas="third"))


@gpu
@pytest.mark.parametrize("n,geom", [(129, "bar"), (4099, "zigzag")])
def test_light_chained_replays_equal_eager(n, geom):
    """Chained replays with the tail deferred to flush(): a continuation head's node tasks read the records the replay
    before it left, pf_graph_tail's displacement update those of the last iteration."""
    _light_vs_eager(lambda: path_model(n, geom, reverse=True), mode="chained")


@gpu
@pytest.mark.parametrize("max_it,tol,expect", [(40, 1e30, 12), (13, 0.0, 13), (27, 0.0, 27)])
def test_light_stop_in_mid_replay_equals_eager(max_it, tol, expect):
    """A stop raised inside a replay at an even (12) and at odd counts (13; 27 in the second replay), replays of 20."""
    _light_vs_eager(lambda: path_model(4099, "zigzag", meas="third"), mode="stop", graph_iters=20, max_it=max_it, tol=tol,
                    stop_at=expect)


@gpu
@pytest.mark.parametrize("n", [129, 4099])
@pytest.mark.parametrize("net", [dict(pos_e=False), dict(pos_a=False), dict(pos_e=False, pos_a=False),
                                 dict(scale_e=3.25, scale_a=0.011), dict(we=16, wa=3), dict(we=13, wa=24)],
                         ids=["E-free", "A-free", "both-free", "scales", "w16x3", "w13x24"])
def test_light_net_variants(n, net):
    """enforce_positive off on E, on A and on both (the backward's own output value takes the z branch), scales != 1, and
    other bucket pairs that have the form (widths 16 and 3: register buckets 8 and 2; 13 and 24: buckets 8 and 12)."""
    _light_vs_eager(lambda: path_model(n, "zigzag", **net), fe=1)


@gpu
@pytest.mark.parametrize("n", [129, 4099])
def test_wider_nets_keep_the_full_forward(n):
    """Widths 27 and 30 (past the buckets whose fused backward has the path form): the four-launch chain as before, the query
    answers 0, and graph == eager."""
    _light_vs_eager(lambda: path_model(n, "zigzag", we=27, wa=30), light=0, form=0)


@gpu
@pytest.mark.parametrize("n", [129, 4099])
def test_young_net_of_bucket_12_keeps_the_full_forward(n):
    """A young net 21 .. 24 wide on a 2-D mesh (register bucket 12, three inputs): its light backward would spill registers
    the path backward holds (profiles/r17_light_forward_registers.txt), so the pair stays on the path form with the full
    forward by dispatch: the query answers 0, the form and graph == eager are unchanged."""
    _light_vs_eager(lambda: path_model(n, "zigzag", we=24, wa=3), light=0)


@gpu
@pytest.mark.parametrize("kind", ["warren", "ring", "ex3", "sharded"])
def test_query_is_zero_off_the_path_form(kind):
    from bench import build_model
    from pinn_fem_amd.engine import HipEngine
    if kind == "sharded":
        from pinn_fem_amd.dist import build_shard_backend
        model, mv, md, _ = build_model(5000, "ex4")
        eng = build_shard_backend(model, mv, md, 0, 2).eng
        assert eng.fusion_info() & 16 == 0
    else:
        if kind == "warren":
            model, mv, md, _ = build_model(5000, "ex4", mesh="warren")
        elif kind == "ex3":
            model, mv, md, _ = build_model(5000, "ex3")
        else:
            model, mv, md = two_net_model(*ring(300))
        eng = HipEngine(model, mv, md)
        assert eng.fusion_info() == (4 if kind == "ex3" else CHAIN_MASK)
    assert eng.graph_form_info() == 0
    assert eng.graph_light_forward() == 0


def test_header_and_binding_declare_the_query():
    """No GPU: the additive entry point is declared in the header and in the ctypes binding, and the ABI version stays 9."""
    import os
    import re
    import ctypes as C
    from pinn_fem_amd import _capi
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pinnfem_hip.h")).read()
    assert _capi.PF_ABI_VERSION == 9 and re.search(r"#define PF_ABI_VERSION 9\b", header)
    assert re.search(r"\bint pf_graph_light_forward\(const pf_problem\* p\);", header)
    assert "pf_graph_light_forward" in _capi.SYMBOLS
    assert _capi.SYMBOLS["pf_graph_light_forward"] == _capi.SYMBOLS["pf_graph_form_info"]
    assert _capi.SYMBOLS["pf_graph_light_forward"][0] is C.c_int
