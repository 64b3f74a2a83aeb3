"""Tension-only (cable) elements in the static Green-Lagrange Newton solve on the device: pf_gl_state_cable through the C ABI
against the bar entry points (bit for bit wherever an element is not slack, the bytes of +0.0 where it is, the slack set
and its counts against the host rule on the device's own strains), then solve_nr, solve() and the CLI against the device's
own bar solve of the structure without its slack elements and against the restatement
tests/gl_cable_static_reference.py (itself pinned by tests/test_gl_cable_static_host.py).

The solves' bound is the one test_gl_f64.py's girder comparison uses: ten times the distance at which the restatement with
scipy's Jacobi-CG (same rtol) ends from the restatement with the direct solve.  On the systems of one or two free dofs CG
is exact and that distance is round-off or 0.0, so the bound has the floor test_gl_cable_static_host.py states between
two Newton solutions of one structure, 1e-12 of max |u|.  The measured figures are printed in front of every assertion.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import gl_cable_reference as gc
import gl_cable_static_reference as gs
import gl_reference as gl
from device_driver import EA, RTOL, GlTruss, flipped_chain_1d, gl_config, gl_field, gl_system, run_cli, system_cache, truss_model
from gl_cable_static_driver import CableState, host_slack

pytestmark = pytest.mark.gpu

SIZES = (1, 255, 256, 257, 1000)
MESHES = [f"{kind}_{n}" for kind in ("truss", "chain") for n in SIZES]
SAME_SOLUTION = 1e-12


@pytest.fixture(scope="module")
def systems():
    yield from system_cache(gl_system)


def _bytes(*arrays):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)


def _check_against_the_bar(S, CS, u, cable, e0, ea, label):
    """One cable state from a cleared set against the bar entry point at the same operands.  Returns (record, slack)."""
    bar = S.state(u, e0, ea)
    CS.clear()
    strain, fe, kt, slack, (n_slack, n_changed) = CS.state(u, cable, e0, ea)
    want = host_slack(np.broadcast_to(cable, (S.ne,)), strain, e0)
    print(f"{label}: {int(want.sum())} of {S.ne} slack, counts ({n_slack}, {n_changed})")
    assert np.array_equal(slack, want) and n_slack == float(want.sum()) and n_changed == n_slack
    assert strain.tobytes() == bar[0].tobytes()
    taut = ~slack
    assert _bytes(fe[taut], kt[taut]) == _bytes(bar[1][taut], bar[2][taut])
    assert _bytes(fe[slack], kt[slack]) == bytes(8 * (fe[slack].size + kt[slack].size))        # +0.0, not -0.0
    # the whole record by value: the bar entry point with E*A = 0 on the slack set
    zeroed = S.state(u, e0, np.where(slack, 0.0, EA if ea is None else ea))
    assert all(np.array_equal(a, b) for a, b in zip((strain, fe, kt), zeroed))
    return (strain, fe, kt), slack


# ---------------------------------------------------------------------------------------------------------------------
# 1. the state kernel against the bar kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MESHES)
def test_cable_state_against_the_bar_state(systems, name):
    """e0 absent, random and cancelling (e0 = e, so e - e0 == 0: taut), E*A absent and given; all-zero flags and all flags
    with everything taut are the bar record to the bit with counts (0, 0); the seeded half and all flags at a field with about
    half the elements in compression follow the rule."""
    S = systems(name)
    CS = CableState(S)
    rng = np.random.default_rng(3000 + S.ne)
    field = gl_field(S, "large", rng)
    seen = 0
    for u in ((field, -field) if S.ne == 1 else (field,)):             # one element: stretched once, compressed once
        ea_given = EA * rng.uniform(0.5, 2.0, S.ne)
        strain_bar = S.state(u)[0]
        if S.ne >= 255:
            assert 0.25 < np.mean(strain_bar < 0.0) < 0.75
        for ea_label, ea in (("model E*A", None), ("E*A given", ea_given)):
            for e0_label, e0 in (("no e0", None), ("random e0", rng.uniform(-0.05, 0.05, S.ne)), ("e0 = e", strain_bar.copy())):
                label = f"{name}, {ea_label}, {e0_label}"
                bar = S.state(u, e0, ea)
                CS.clear()
                got = CS.state(u, False, e0, ea)
                assert _bytes(*got[:3]) == _bytes(*bar) and not got[3].any() and got[4] == (0.0, 0.0), label
                for which, cable in (("half", gc.seeded_half(S.ne)), ("all", True)):
                    record, slack = _check_against_the_bar(S, CS, u, cable, e0, ea, f"{label}, {which}")
                    seen += int(slack.sum())
                    if e0_label == "e0 = e":                # e - e0 == 0 is taut: the bar record, nothing slack
                        assert not slack.any() and _bytes(*record) == _bytes(*bar), label
            # all flags, everything taut: e0 below every strain
            e0 = strain_bar - rng.uniform(1e-3, 1e-2, S.ne)
            bar = S.state(u, e0, ea)
            CS.clear()
            got = CS.state(u, True, e0, ea)
            assert _bytes(*got[:3]) == _bytes(*bar) and not got[3].any() and got[4] == (0.0, 0.0)
    assert seen > 0


@pytest.mark.parametrize("name", ["truss_257", "chain_1000"])
def test_counts_follow_the_set_and_repeats_are_the_same_bytes(systems, name):
    S = systems(name)
    CS = CableState(S)
    rng = np.random.default_rng(3100 + S.ne)
    u, other, e0 = gl_field(S, "large", rng), gl_field(S, "large", rng), rng.uniform(-0.05, 0.05, S.ne)
    cable = gc.seeded_half(S.ne)
    CS.clear()
    first = CS.state(u, cable, e0)
    bytes_first = CS.everything()
    assert first[4] == (float(first[3].sum()), float(first[3].sum())) and first[3].any()
    again = CS.state(u, cable, e0)                          # the same u: nothing changes
    assert again[4] == (first[4][0], 0.0) and np.array_equal(again[3], first[3])
    moved = CS.state(other, cable, e0)
    want = host_slack(cable, moved[0], e0)
    print(f"{name}: slack {first[4][0]:.0f} -> {moved[4][0]:.0f}, changed {moved[4][1]:.0f} (host {int((want != first[3]).sum())})")
    assert np.array_equal(moved[3], want) and moved[4] == (float(want.sum()), float((want != first[3]).sum())) and moved[4][1] > 0
    # the partials behind the counts are exact integers that add up, and what lies behind them is not written
    counts = CS.counts.cpu().numpy()
    part = counts[2: 2 + 2 * CS.blocks].reshape(-1, 2)
    assert np.all(part == np.floor(part)) and part[:, 0].sum() == counts[0] and part[:, 1].sum() == counts[1]
    assert np.all(counts[2 + 2 * CS.blocks:] == 7.0)
    # a repeat from the same entry state: the same bytes, counts and partial buffers included
    CS.clear()
    CS.state(u, cable, e0)
    assert CS.everything() == bytes_first


def test_grid_stride_wrap_in_one_launch():
    """PF_MAX_NODE_BLOCKS * 256 + 37 elements: the first 37 threads take a second element."""
    from pinn_fem_amd import _capi
    ne = _capi.PF_MAX_NODE_BLOCKS * 256 + 37
    rng = np.random.default_rng(ne)
    S = GlTruss(*flipped_chain_1d(ne, rng), 1)
    CS = CableState(S)
    assert CS.blocks == _capi.PF_MAX_NODE_BLOCKS
    u = gl_field(S, "large", rng)
    cable = np.arange(ne) % 3 != 0
    bar = S.state(u)
    CS.clear()
    strain, fe, kt, slack, (n_slack, n_changed) = CS.state(u, cable)
    want = host_slack(cable, strain, None)
    print(f"{ne} elements: {int(want.sum())} slack, counts ({n_slack:.0f}, {n_changed:.0f}), slack in the wrap {want[-37:].sum()}")
    assert 0.2 < want.mean() < 0.5 and want[-37:].any() and not want[-37:].all()
    assert np.array_equal(slack, want) and n_slack == float(want.sum()) == n_changed
    assert strain.tobytes() == bar[0].tobytes()
    assert _bytes(fe[~slack], kt[~slack]) == _bytes(bar[1][~slack], bar[2][~slack])
    assert _bytes(fe[slack], kt[slack]) == bytes(8 * (fe[slack].size + kt[slack].size))
    part = CS.counts.cpu().numpy()[2: 2 + 2 * CS.blocks].reshape(-1, 2)
    assert np.array_equal(part[:, 0], _block_counts(want, CS.blocks)) and np.array_equal(part[:, 1], part[:, 0])
    del S, CS
    torch.cuda.empty_cache()


def _block_counts(flags, blocks):
    """Per block, the number of set flags among the elements its threads take in the grid-stride loop."""
    out = np.zeros(blocks)
    np.add.at(out, (np.arange(flags.size) // 256) % blocks, flags.astype(float))
    return out


@pytest.mark.parametrize("name", ["truss_257", "chain_257"])
def test_fint_and_kt_diag_after_a_cable_state(systems, name):
    """pf_gl_fint and pf_kt_diag_f64 read the cable record as they read the bar's: per dof the sequential sum over the
    node's elements in ascending incidence order of the device's own records, to the bit (a slack element adds +-0.0 in its
    place)."""
    S = systems(name)
    CS = CableState(S)
    rng = np.random.default_rng(3200 + S.ne)
    CS.clear()
    _, fe, kt, slack, _ = CS.state(gl_field(S, "large", rng), gc.seeded_half(S.ne), rng.uniform(-0.05, 0.05, S.ne))
    assert slack.any()
    fint, diag = S.fint(), S.kt_diag()
    plan = S.eng.plan
    adj_ptr, adj = np.asarray(plan.adj_ptr), np.asarray(plan.adj)
    want_f, want_d = np.zeros(S.n), np.zeros(S.n)
    for node in range(S.n_nodes):
        for c in range(S.dim):
            acc_f, acc_d = 0.0, 0.0
            for code in adj[adj_ptr[node]:adj_ptr[node + 1]]:
                e = code >> 1
                term = float(fe[e, c])
                acc_f = acc_f + (term if S.el[e, 1] == node else -term)
                acc_d = acc_d + float(kt[e, 2 * c if S.dim == 2 else 0])
            want_f[node * S.dim + c], want_d[node * S.dim + c] = acc_f, acc_d
    want_d[S.mask] = 0.0
    differ = int((fint != want_f).sum())
    print(f"{name}: f_int entries that differ from the host sum {differ}, {int(slack.sum())} slack elements")
    assert diag.tobytes() == want_d.tobytes()
    assert fint.tobytes() == want_f.tobytes()


def test_argument_errors_touch_nothing(systems):
    S = systems("truss_257")
    CS = CableState(S)
    rng = np.random.default_rng(61)
    CS.state(gl_field(S, "large", rng), gc.seeded_half(S.ne))
    CS.counts.fill_(7.0)
    S.refill()
    before = CS.everything()
    eng = S.eng
    u = S.dev(np.ones(S.n))
    ok = dict(cable=CS.cable.data_ptr(), slack=CS.slack.data_ptr(), counts=CS.counts.data_ptr(), u=u.data_ptr())

    def refused(text, problem=None, rec=None, **bad):
        a = {**ok, **bad}
        with eng.on_stream():
            rc = S.lib.pf_gl_state_cable(eng._ref() if problem is None else problem, C.byref(S.rec if rec is None else rec), None,
                                         None, a["cable"], a["slack"], a["counts"], a["u"], eng._stream())
        torch.cuda.synchronize()
        assert rc == S.capi.PF_ERR_ARG and S.lib.pf_last_error().decode().startswith("pf_gl_state_cable: " + text)

    for name in ("cable", "slack", "counts"):
        refused("null cable, slack or counts (pf_gl_state / pf_gl_state_ea / pf_gl_state_e0", **{name: None})
    refused("bad argument", u=None)
    refused("bad argument", rec=S.capi.PfGl())
    bad_mesh = S.capi.PfProblem.from_buffer_copy(eng.P)
    bad_mesh.mesh.dim = 3
    refused("bad argument", problem=C.byref(bad_mesh))
    bad_mesh.mesh.dim, bad_mesh.mesh.n_elems = 2, -1
    refused("bad argument", problem=C.byref(bad_mesh))
    assert CS.everything() == before
    # no elements: PF_OK and zero counts
    empty = S.capi.PfProblem.from_buffer_copy(eng.P)
    empty.mesh.n_elems = 0
    with eng.on_stream():
        assert S.lib.pf_gl_state_cable(C.byref(empty), C.byref(S.rec), None, None, ok["cable"], ok["slack"], ok["counts"], ok["u"],
                                       eng._stream()) == S.capi.PF_OK
    torch.cuda.synchronize()
    counts = CS.counts.cpu().numpy()
    assert counts[0] == 0.0 and counts[1] == 0.0 and np.all(counts[2:] == 7.0)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the solves
# ---------------------------------------------------------------------------------------------------------------------
def _bound(nodes, el, loads, fixed, dim, cable, e0, u_ref):
    """test_gl_f64.py's: 10 x the distance of the restatement with scipy's Jacobi-CG from the one with the direct solve,
    with the floor SAME_SOLUTION (see the module's docstring)."""
    u_cg = gs.newton_cable(nodes, el, loads, fixed, EA, dim, cable, e0=e0, linear_solve=gl.jacobi_cg(RTOL))[0]
    err_ref = np.max(np.abs(u_cg - u_ref)) / np.max(np.abs(u_ref))
    return max(10.0 * err_ref, SAME_SOLUTION), err_ref


def _check_solve(label, res, nodes, el, loads, fixed, dim, cable, e0=None, config=None):
    """A converged device solve with cables against the restatement (displacements, slack set, history) and against the
    device's own bar solve of the structure without its slack elements."""
    from pinn_fem_amd.fem.solver import solve_nr
    u_ref, it_ref, ok, slack_ref, _ = gs.newton_cable(nodes, el, loads, fixed, EA, dim, cable, e0=e0)
    bound, err_ref = _bound(nodes, el, loads, fixed, dim, cable, e0, u_ref)
    u, scale = res.displacements.reshape(-1), np.max(np.abs(u_ref))
    err = np.max(np.abs(u - u_ref)) / scale
    keep = ~res.slack
    reduced = truss_model(nodes, np.asarray(el)[keep], loads, fixed, dim)
    bar = solve_nr(reduced, gl_config(**{**(config or {}), "initial_strain": None if e0 is None else np.asarray(e0)[keep]}),
                   1.0, u_initial=torch.from_numpy(u.copy()))
    err_bar = np.max(np.abs(u - bar.displacements.reshape(-1))) / scale
    last = res.history[-1]
    print(f"{label}: {int(last['iterations'])} iterations (restatement {it_ref}), {int(res.slack.sum())} slack, error "
          f"{err:.2e} (scipy-CG Newton {err_ref:.2e}, bound {bound:.2e}), to the device's bar solve of the reduced "
          f"structure {err_bar:.2e}")
    assert ok and res.converged and bar.converged
    assert np.array_equal(res.slack, slack_ref) and last["slack_elements"] == float(slack_ref.sum())
    assert err <= bound and err_bar <= 2.0 * bound
    assert np.all(res.axial_forces[res.slack] == 0.0) and np.all(res.axial_forces[keep & np.broadcast_to(cable, keep.shape)] >= 0.0)
    want_n = gl.axial_forces(nodes, el, u_ref, EA, dim, e0)
    assert np.allclose(res.axial_forces[keep], want_n[keep], rtol=0.0, atol=1e-6 * np.max(np.abs(want_n)))
    return u_ref


@pytest.mark.parametrize("preconditioner", ["jacobi", "two-level-updated"])
def test_solve_nr_guyed_mast(preconditioner):
    from pinn_fem_amd.fem.solver import solve_nr
    T, nodes, el, fixed, e0 = gc.guyed_mast(2.0)
    model = truss_model(nodes, el, T.loads, fixed)
    config = dict(nr_preconditioner=preconditioner)
    res = solve_nr(model, gl_config(initial_strain=e0, cable_elements=[1, 2], **config), 1.0)
    _check_solve(f"guyed mast, {preconditioner}", res, nodes, el, T.loads, fixed, 2, T.cable, e0, config)
    assert res.slack.tolist() == [False, False, True] and res.reactions.reshape(-1)[6] == 0.0 and res.reactions.reshape(-1)[7] == 0.0
    # without cable_elements: the all-bar answer as before, 2e-2 away
    bars = solve_nr(model, gl_config(initial_strain=e0, **config), 1.0)
    u_bar, _, ok = gl.newton(nodes, el, T.loads, fixed, EA, 2, e0=e0)
    away = np.max(np.abs(bars.displacements.reshape(-1) - res.displacements.reshape(-1)))
    miss = np.max(np.abs(bars.displacements.reshape(-1) - u_bar)) / np.max(np.abs(u_bar))
    print(f"without cable_elements: {miss:.2e} from the all-bar restatement, {away:.2e} from the cable solve")
    assert ok and bars.converged and miss <= SAME_SOLUTION and away > 1e-2
    assert bars.slack is None and "slack_elements" not in bars.history[-1] and bars.axial_forces[2] < 0.0


@pytest.mark.parametrize("n_panels", [8, 64])
def test_solve_nr_xbraced_girder_in_one_increment(n_panels):
    from pinn_fem_amd.fem.solver import solve_nr
    nodes, el, unit, fixed, tip, cable = gs.xbraced_girder(n_panels)
    loads = gs.GIRDER_LOADS[n_panels] * unit
    res = solve_nr(truss_model(nodes, el, loads, fixed), gl_config(cable_elements=np.flatnonzero(cable).tolist()), 1.0)
    _check_solve(f"x-braced girder, {n_panels} panels", res, nodes, el, loads, fixed, 2, cable)
    assert res.slack.reshape(n_panels, 5)[:, 3:].sum(axis=1).tolist() == [1] * n_panels


def test_solve_xbraced_girder_in_four_increments():
    from pinn_fem_amd.fem.solver import solve
    nodes, el, unit, fixed, tip, cable = gs.xbraced_girder(8)
    loads = gs.GIRDER_LOADS[8] * unit
    res = solve(truss_model(nodes, el, loads, fixed), gl_config(cable_elements=np.flatnonzero(cable).tolist(), method="nr", n_increments=4))
    u_ref = _check_solve("x-braced girder, 8 panels, four increments", res, nodes, el, loads, fixed, 2, cable)
    u4, slack4, _ = gs.incremental_cable(nodes, el, loads, fixed, EA, 2, cable, 4)
    assert np.array_equal(res.slack, slack4) and np.max(np.abs(u4 - u_ref)) <= SAME_SOLUTION * np.max(np.abs(u_ref))
    assert res.history[-1]["load_factor"] == 1.0


@pytest.mark.parametrize("load", [50.0, -50.0])
def test_solve_nr_bilinear_1d(load):
    from pinn_fem_amd.fem.solver import solve_nr
    x, el, fixed, cable = gs.bilinear_1d()
    loads = np.array([0.0, load, 0.0])
    res = solve_nr(truss_model(x, el, loads, fixed, dim=1), gl_config(cable_elements=[1]), 1.0)
    _check_solve(f"1-D bilinear, load {load}", res, x, el, loads, fixed, 1, cable)
    u = float(res.displacements.reshape(-1)[1])
    if load > 0.0:
        assert res.slack.tolist() == [False, True] and abs(gl.bar_1d_load(EA, 1.0, u) / load - 1.0) <= 1e-12
    else:
        assert not res.slack.any() and res.axial_forces[1] > 0.0


def test_a_slack_mechanism_is_refused():
    """One cable, one free node, the load pushes towards the support: the second iteration's state holds the node with
    nothing; the loop raises before the CG solve."""
    from pinn_fem_amd.fem.solver import solve_nr
    model = truss_model(np.array([0.0, 1.0]), np.array([[0, 1]]), np.array([0.0, -1.0]), np.array([0]), dim=1)
    with pytest.raises(RuntimeError, match=r"Newton iteration 2: its diagonal is 0 at free dof 1, which only slack cables hold "
                                           r".*solve_dynamic with rest_tolerance"):
        solve_nr(model, gl_config(cable_elements="all"), 1.0)
    assert solve_nr(model, gl_config(), 1.0).converged        # the same load on a bar is an ordinary solve


def test_cli_on_the_static_inputs(tmp_path):
    out = run_cli(tmp_path, "guyed_mast_static")
    T, nodes, el, fixed, e0 = gc.guyed_mast(2.0)
    u_ref, _, ok, slack, _ = gs.newton_cable(nodes, el, T.loads, fixed, EA, 2, T.cable, e0=e0)
    miss = np.max(np.abs(np.array(out["displacements"]) - u_ref)) / np.max(np.abs(u_ref))
    print(f"CLI, guyed mast: slack {out['slack_elements']}, axial {out['axial_forces']}, miss {miss:.2e}")
    assert ok and out["converged"] and out["slack_elements"] == [2] and out["axial_forces"][2] == 0.0 and miss <= SAME_SOLUTION
    assert out["history"][-1]["slack_elements"] == 1.0
    out = run_cli(tmp_path, "xbraced_girder_static")
    nodes, el, unit, fixed, tip, cable = gs.xbraced_girder(8)
    u_ref, slack, _ = gs.incremental_cable(nodes, el, gs.GIRDER_LOADS[8] * unit, fixed, EA, 2, cable, 4)
    bound = _bound(nodes, el, gs.GIRDER_LOADS[8] * unit, fixed, 2, cable, None, u_ref)[0]
    miss = np.max(np.abs(np.array(out["displacements"]) - u_ref)) / np.max(np.abs(u_ref))
    print(f"CLI, x-braced girder: {len(out['slack_elements'])} slack, miss {miss:.2e} (bound {bound:.2e})")
    assert out["converged"] and out["slack_elements"] == np.flatnonzero(slack).tolist() and miss <= bound
    assert all(out["axial_forces"][e] == 0.0 for e in out["slack_elements"])
