"""Tension-only (cable) elements in the explicit dynamics on the device: pf_gl_dyn_start_cable / _steps_cable /
_graph_create_cable / _energy_cable called through the C ABI and held against the float64 restatement of
tests/gl_cable_reference.py (itself pinned by tests/test_gl_cable_host.py), then solve_dynamic and the CLI on a cable in free
flight and on a guyed mast whose leeward guy goes slack.

The bounds are the bar step's own (test_gl_dynamics_f64.step_bounds, derived there from 2^-53 and operation counts), taken
over ALL elements, slack ones included: device and restatement can disagree on a slack decision only where |e - e0| is below
its own rounding, and the disputed force is then inside the bound's term for e - e0.  The measured figures are printed in
front of every assertion.
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

import gl_cable_reference as gc
import gl_reference as gl
from device_driver import EA, U53, GlTruss, gl_field, gl_system, run_cli, system_cache
from test_gl_dynamics_f64 import DynRun, check_step, multi_step_case, restatement, same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def systems():
    yield from system_cache(gl_system)


class CableRun(DynRun):
    """DynRun through the _cable entry points: the flags ride right behind the pf_dyn record."""

    def __init__(self, S, T, u, v, dt, cable, **kw):
        super().__init__(S, T, u, v, dt, **kw)
        dev = S.eng.device
        self.cable = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(cable, (S.ne,)), dtype=np.uint8)).to(dev)
        self.out = torch.full((self.capi.PF_DYN_CABLE_ENERGY_COUNT,), 7.0, dtype=torch.float64, device=dev)

    def start(self):
        self.call("pf_gl_dyn_start_cable", self.cable.data_ptr())

    def steps(self, n):
        self.call("pf_gl_dyn_steps_cable", self.cable.data_ptr(), int(n))

    def graph(self, n):
        g = C.c_void_p()
        eng = self.S.eng
        with eng.on_stream():
            self.capi.check(eng.lib.pf_gl_dyn_graph_create_cable(eng._ref(), C.byref(self.S.rec), C.byref(self.rec),
                                                                 self.cable.data_ptr(), int(n), eng._stream(), C.byref(g)),
                            "pf_gl_dyn_graph_create_cable")
        return g

    def energy(self):
        self.call("pf_gl_dyn_energy_cable", self.cable.data_ptr(), self.out.data_ptr())
        torch.cuda.synchronize()
        return self.out[:5].cpu().numpy()

    def everything(self):
        return super().everything() + b"".join(t.cpu().numpy().tobytes() for t in (self.out, self.cable, self.minv, self.f_ext))


def flags_of(which, ne):
    return np.ones(ne, dtype=bool) if which == "all" else gc.seeded_half(ne)


def all_slack_dofs(T, u):
    """bool [n_dofs]: the free dofs of the nodes whose every element is slack at u."""
    s = T.slack(u)
    slack_count, count = np.zeros(T.n_nodes, dtype=int), np.zeros(T.n_nodes, dtype=int)
    np.add.at(slack_count, T.el.reshape(-1), np.repeat(s, 2))
    np.add.at(count, T.el.reshape(-1), 1)
    return np.repeat((slack_count == count) & (count > 0), T.dim) & T.free


# ---------------------------------------------------------------------------------------------------------------------
# 1. one step to the derived bound
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", ["random", "cancelling"])
@pytest.mark.parametrize("which", ["all", "half"])
@pytest.mark.parametrize("name", ["truss_257", "chain_257"])
def test_one_step_against_the_restatement(systems, name, which, field):
    """The bar step's case with every element flagged, then the seeded half: u = where(free, 0.05 standard normal, 0), an odd
    step number inside the load ramp, damping, a velocity, e0 drawn from +-1e-2.  With all flagged 47 % of the truss's
    elements are slack and 4 free nodes have every element slack (asserted: the case cannot thin out).  Those nodes' dofs
    get v = c1 v + g lam F / m with no f_int term, held to the bound; f_int there is 0.0 to the bit, read off a step with no
    load, no velocity and c1 = 1, which leaves v == 0.0 exactly.  Fixed dofs come out exactly 0.0.  cancelling: e0 = e, so
    se = +0.0 on the restatement and nothing is slack; the bar's bound holds."""
    S = systems(name)
    rng = np.random.default_rng(7)
    u = np.where(S.free, 0.05 * rng.standard_normal(S.n), 0.0)
    v, e0 = 0.1 * rng.standard_normal(S.n), rng.uniform(-1e-2, 1e-2, S.ne)
    if field == "cancelling":
        e0 = restatement(S).strain(u)[0].copy()
    cable = flags_of(which, S.ne)
    T = gc.with_cables(restatement(S, EA, e0), cable)
    slack, lonely = T.slack(u), all_slack_dofs(T, u)
    print(f"{name} {which} {field}: {slack.mean():.3f} of the elements slack, {int(lonely.sum()) // S.dim} free nodes with every "
          f"element slack")
    if field == "cancelling":
        assert not slack.any()
    elif name == "truss_257" and which == "all":
        assert slack.mean() > 0.4 and lonely.sum() // 2 >= 4
    else:
        assert slack.any() and (which == "half" or lonely.any())
    dt, alpha, lam0, lam1, t_ramp, n = 0.5 * T.stable_time_step(u), 3.0, 0.25, 1.5, 1.0, 5
    assert n * dt < t_ramp
    run = CableRun(S, T, u, v, dt, cable, alpha=alpha, lam0=lam0, lam1=lam1, t_ramp=t_ramp, e0=e0, clock=n)
    run.steps(1)
    got_u, got_v, clock = run.read()
    assert clock == n + 1
    check_step(S, T, got_u, got_v, u, v, n, dt, alpha, lam0, lam1, t_ramp, f"{name} {which} {field}")
    assert run.u[n & 1].cpu().numpy().tobytes() == np.ascontiguousarray(u).tobytes()        # u_n is only read
    if field == "random":
        # the slack rule changes the answer: the bar's step is elsewhere
        bar_v = restatement(S, EA, e0)
        bar_v.loads = T.loads
        assert np.max(np.abs(bar_v.step(u, v, n, dt, alpha, lam0, lam1, t_ramp)[1] - got_v)) > 1e-6
        # f_int of the all-slack nodes: no load, no velocity, alpha = 0 (c1 = 1)
        T0 = gc.with_cables(restatement(S, EA, e0), cable)
        T0.loads = np.zeros(S.n)
        still = CableRun(S, T0, u, np.zeros(S.n), dt, cable, e0=e0, clock=n)
        still.steps(1)
        v0 = still.read()[1]
        assert np.max(np.abs(v0[S.free])) > 0.0
        assert v0[lonely].tobytes() == np.zeros(int(lonely.sum())).tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# 2. bit-for-bit identities
# ---------------------------------------------------------------------------------------------------------------------
def changing_case(S):
    """The multi-step case of the bar's tests (a step load of 20 x standard normal from rest at half the bound of the
    undeformed truss) with the seeded half flagged: on the restatement 121 elements change state on the way to step 256."""
    T, zero, dt = multi_step_case(S)
    cable = gc.seeded_half(S.ne)
    return gc.with_cables(T, cable), cable, zero, dt


def test_zero_flags_and_taut_cables_are_the_bar_run(systems):
    """All-zero flags through the _cable entry points equal the bar entry points after 64 steps (u0, u1, v, clock), start
    included; and a taut string with every element flagged, in tension throughout, equals its bar run."""
    S = systems("truss_257")
    T, zero, dt = multi_step_case(S)
    rng = np.random.default_rng(43)
    u0, v0 = np.where(S.free, 1e-3 * rng.standard_normal(S.n), 0.0), np.where(S.free, 1e-2 * rng.standard_normal(S.n), 0.0)
    kw = dict(alpha=0.7, lam0=0.0, lam1=1.0, t_ramp=40.5 * dt)
    bar, none = DynRun(S, T, u0, v0, dt, **kw), CableRun(S, T, u0, v0, dt, False, **kw)
    for run in (bar, none):
        run.start()
        run.steps(63)
    assert bar.read()[2] == 64 and np.max(np.abs(bar.read()[0])) > 1e-3
    assert bar.everything() == DynRun.everything(none)
    flagged = CableRun(S, gc.with_cables(T, True), u0, v0, dt, True, **kw)
    flagged.start()
    flagged.steps(63)
    assert not same(flagged.read(), bar.read())             # the flags are read: this case has compression
    # a pretensioned string, plucked sideways: every element stays in tension
    n = 64
    x = np.linspace(-1.0, 1.0, n + 1)
    nodes = np.stack([x, np.zeros_like(x)], axis=1)
    el = np.stack([np.arange(n), np.arange(1, n + 1)], axis=1)
    St = GlTruss(nodes, el, np.array([0, 1, 2 * n, 2 * n + 1]), 2)
    e0 = np.full(n, -1e-3)
    Tt = gc.with_cables(restatement(St, EA, e0), True)
    Tt.loads = np.zeros(St.n)
    us = np.zeros(St.n)
    us[1::2] = 1e-2 * np.sin(np.pi * np.arange(n + 1) / n)
    dts = 0.5 * Tt.stable_time_step(us)
    ref_u, ref_v = us, np.zeros(St.n)
    for k in range(64):                                     # the restatement: in tension at every step
        assert not Tt.slack(ref_u).any()
        ref_u, ref_v = Tt.step(ref_u, ref_v, k, dts)
    string_bar, string_cable = DynRun(St, Tt, us, np.zeros(St.n), dts, e0=e0), CableRun(St, Tt, us, np.zeros(St.n), dts, True, e0=e0)
    string_bar.steps(64)
    string_cable.steps(64)
    assert np.max(np.abs(string_bar.read()[0] - us)) > 1e-6 and same(string_bar.read(), string_cable.read())


def test_graph_replay_split_runs_and_repeats(systems):
    """On the run in which elements change state: graph replay equals eager launches; two graphs of 32 steps equal one of
    64; an odd count followed by more steps equals one run; a repeated run equals itself."""
    S = systems("truss_257")
    T, cable, zero, dt = changing_case(S)
    _, _, at, ever = T.state_changes(zero, zero, 0, 64, dt)
    print(f"64 steps: {int(ever.sum())} elements change state at {len(at)} steps")
    assert ever.sum() > 20

    def make():
        return CableRun(S, T, zero, zero, dt, cable)

    eager = make()
    eager.steps(64)
    want = eager.read()
    assert want[2] == 64 and np.max(np.abs(want[0])) > 1e-3
    graphs = []
    try:
        one = make()
        graphs.append(one.graph(64))
        assert one.read()[2] == 0 and not one.read()[0].any()          # capture runs nothing
        one.replay(graphs[-1])
        assert same(one.read(), want)
        two = make()
        graphs.append(two.graph(32))
        two.replay(graphs[-1], times=2)
        assert same(two.read(), want)
    finally:
        for g in graphs:
            S.lib.pf_graph_destroy(g)
    again = make()
    again.steps(64)
    assert same(again.read(), want)
    split = make()
    split.steps(7)
    assert split.read()[2] == 7
    split.steps(57)
    assert same(split.read(), want)
    bar = DynRun(S, T, zero, zero, dt)
    bar.steps(64)
    assert not same(bar.read(), want)


# ---------------------------------------------------------------------------------------------------------------------
# 3. many steps against the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_steps", [64, 256])
def test_many_steps_against_the_restatement(systems, n_steps):
    """The bar's rule and the bar's factor on the state-changing case: device - restatement <= 8 x the restatement's own
    ascending-against-descending summation spread after 64 and 256 steps (max norm of u and of v).  The measured ratios are in
    profiles/."""
    S = systems("truss_257")
    T, cable, zero, dt = changing_case(S)
    run = CableRun(S, T, zero, zero, dt, cable)
    run.steps(n_steps)
    got_u, got_v, clock = run.read()
    assert clock == n_steps
    asc, desc = T.run(zero, zero, 0, n_steps, dt), T.run(zero, zero, 0, n_steps, dt, descending=True)
    print(f"{n_steps} steps: {int(T.slack(asc[0]).sum())} elements slack on the restatement, "
          f"{int((T.slack(asc[0]) != T.slack(got_u)).sum())} decided otherwise at the device's state")
    for what, got, a, d in (("u", got_u, asc[0], desc[0]), ("v", got_v, asc[1], desc[1])):
        spread, err = np.max(np.abs(a - d)), np.max(np.abs(got - a))
        print(f"{n_steps} steps {what}: max |{what}| {np.max(np.abs(a)):.3f}, spread {spread:.3e}, device - restatement "
              f"{err:.3e}, ratio {err / spread:.3f}")
        assert spread > 0.0 and err <= 8.0 * spread


# ---------------------------------------------------------------------------------------------------------------------
# 4. the grid-stride loop
# ---------------------------------------------------------------------------------------------------------------------
def test_long_chain_step_by_step():
    """A 1-D chain of 300 001 nodes with alternating flags: more nodes than the 1024 workgroups of 256 threads the node kernels
    launch, so every thread takes a second node and reads flags past the first sweep.  Two steps, both parities of the
    ping-pong, each held to the one-step bound from the device's own previous state."""
    from device_driver import flipped_chain_1d
    n_nodes = 300_001
    rng = np.random.default_rng(n_nodes)
    S = GlTruss(*flipped_chain_1d(n_nodes - 1, rng), 1)
    cable = np.arange(S.ne) % 2 == 1
    T = gc.with_cables(restatement(S), cable)
    u, v = gl_field(S, "large", rng), 0.1 * rng.standard_normal(S.n)
    u[S.mask], v[S.mask] = 0.0, 0.0
    assert 0.2 < T.slack(u).mean() < 0.3
    dt, alpha = 0.5 * T.stable_time_step(u), 0.5
    run = CableRun(S, T, u, v, dt, cable, alpha=alpha)
    for n in range(2):
        run.steps(1)
        got_u, got_v, clock = run.read()
        assert clock == n + 1
        check_step(S, T, got_u, got_v, u, v, n, dt, alpha, 1.0, 1.0, 0.0, f"{n_nodes} nodes, step {n}")
        u, v = got_u, got_v
    del S
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------------
# 5. the energy kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["all", "half"])
@pytest.mark.parametrize("name", ["truss_257", "chain_257"])
def test_energy_against_the_restatement(systems, name, which):
    """pf_gl_dyn_energy_cable at the state the clock points to (an odd clock: u1), to the bounds of the bar's test: a sum of K
    terms in any order is off by at most (K - 1) 2^-53 sum |terms| per side; kinetic m v^2 / 2 with m = 1 / minv 5 roundings
    per side, f u one, the strain energy six on the term and twice the relative error of e - e0, (8 e_abs + 2 (|e| + |e0|))
    2^-53 / |e - e0|, that last sum over all elements, slack ones included (a disputed element's whole term is below it).
    max |v| is exact and out[4] is the restatement's slack count as an integer.  With all-zero flags out[0..3] are the bar
    call's bits and out[4] is 0.0."""
    S = systems(name)
    rng = np.random.default_rng(S.ne + 53)
    u, v, e0 = gl_field(S, "large", rng), np.where(S.free, rng.standard_normal(S.n), 0.0), rng.uniform(-1e-2, 1e-2, S.ne)
    cable = flags_of(which, S.ne)
    T = gc.with_cables(restatement(S, EA, e0), cable)
    run = CableRun(S, T, u, v, 1e-3, cable, e0=e0, clock=3)
    got = run.energy().copy()
    want = T.energies(u, v)
    e, _, du = T.strain(u)
    taut = ~T.slack(u)
    e_abs = (2.0 * np.sum(np.abs(T.d0) * np.abs(du), axis=1) + np.sum(du * du, axis=1)) / (2.0 * T.l02)
    b_strain = ((2 * S.ne + 12) * U53 * want[1]
                + np.sum(T.ea * T.l0 * np.abs(e - T.e0) * (8 * e_abs + 2 * (np.abs(e) + np.abs(T.e0)))) * U53)
    bounds = ((2 * S.n + 10) * U53 * want[0], b_strain, (2 * S.n + 2) * U53 * float(np.sum(np.abs(T.loads * u))), 0.0, 0.0)
    for what, g, w, b in zip(("kinetic", "strain", "f.u", "max |v|", "slack elements"), got, want, bounds):
        print(f"{name} {which} {what}: {g:.15e}, restatement {w:.15e}, error / bound {abs(g - w) / max(b, 1e-300):.3f}")
        assert np.isfinite(g) and abs(g - w) <= b
    assert got[4] == int(got[4]) == want[4] == S.ne - int(taut.sum()) and want[4] > S.ne // 8
    full = restatement(S, EA, e0).energies(u, v)[1]
    assert 0.0 < got[1] < full and full - want[1] > 1e-2 * full         # the slack elements' energy is left out
    assert run.energy().tobytes() == got.tobytes() and run.read()[2] == 3
    bar, none = DynRun(S, T, u, v, 1e-3, e0=e0, clock=3), CableRun(S, T, u, v, 1e-3, False, e0=e0, clock=3)
    e_bar, e_none = bar.energy().copy(), none.energy().copy()
    assert e_none[:4].tobytes() == e_bar.tobytes() and e_none[4] == 0.0 and abs(e_bar[1] - full) <= 1e-12 * full


# ---------------------------------------------------------------------------------------------------------------------
# 6. argument errors
# ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors_touch_nothing(systems):
    """A null cable, every refusal of the bar entry points' check, n_steps < 1, a null result buffer and a non-zero clock at
    _start_cable: PF_ERR_ARG with a message that begins with the function's name, before anything is enqueued; the clock and
    every buffer stay as they were, byte for byte."""
    S = systems("chain_257")
    T = gc.with_cables(restatement(S), True)
    rng = np.random.default_rng(59)
    run = CableRun(S, T, rng.standard_normal(S.n), rng.standard_normal(S.n), 1e-3, gc.seeded_half(S.ne), alpha=0.5, lam0=0.0,
                   lam1=1.0, t_ramp=0.25)
    before = run.everything()
    graph = C.c_void_p()
    entry = {"pf_gl_dyn_start_cable": (), "pf_gl_dyn_steps_cable": (1,), "pf_gl_dyn_energy_cable": (run.out.data_ptr(),)}

    def refused(name, rec=None, problem=None, args=None, gl_rec=None, cable=run.cable.data_ptr(), text=""):
        eng = S.eng
        rec = run.rec if rec is None else rec
        problem = eng._ref() if problem is None else problem
        gl_rec = C.byref(S.rec) if gl_rec is None else gl_rec
        with eng.on_stream():
            if name == "pf_gl_dyn_graph_create_cable":
                rc = eng.lib.pf_gl_dyn_graph_create_cable(problem, gl_rec, C.byref(rec), cable, 1 if args is None else args[0],
                                                          eng._stream(), C.byref(graph))
            else:
                rc = getattr(eng.lib, name)(problem, gl_rec, C.byref(rec), cable, *(entry[name] if args is None else args),
                                            eng._stream())
        assert rc == S.capi.PF_ERR_ARG, (name, rc)
        assert S.lib.pf_last_error().decode().startswith(name + ": " + text), S.lib.pf_last_error()
        assert not graph

    def changed(**fields):
        rec = S.capi.PfDyn()
        C.memmove(C.byref(rec), C.byref(run.rec), C.sizeof(rec))
        for key, value in fields.items():
            setattr(rec, key, value)
        return rec

    names = list(entry) + ["pf_gl_dyn_graph_create_cable"]
    for name in names:
        refused(name, cable=None, text="null cable")
        for pointer in ("minv", "f_ext", "u0", "u1", "v", "clock"):
            refused(name, changed(**{pointer: None}), text="null pointer")
        for bad, text in ((dict(dt=0.0), "dt"), (dict(dt=-1e-3), "dt"), (dict(dt=float("nan")), "dt"), (dict(dt=float("inf")), "dt"),
                          (dict(alpha=-1.0), "alpha"), (dict(t_ramp=-1.0), "t_ramp"), (dict(lam1=float("inf")), "non-finite")):
            refused(name, changed(**bad), text=text)
        bad_mesh = S.capi.PfProblem()
        C.memmove(C.byref(bad_mesh), C.byref(S.eng.P), C.sizeof(bad_mesh))
        bad_mesh.mesh.n_dofs += 1
        refused(name, problem=C.byref(bad_mesh), text="bad mesh")
        no_d0 = S.capi.PfGl()
        refused(name, gl_rec=C.byref(no_d0), text="null pointer")
    for name in ("pf_gl_dyn_steps_cable", "pf_gl_dyn_graph_create_cable"):
        for n in (0, -3):
            refused(name, args=(n,), text="n_steps")
    refused("pf_gl_dyn_energy_cable", args=(None,), text="null pointer")
    assert run.everything() == before
    # a non-zero clock at the start
    run.steps(1)
    moved = run.everything()
    assert run.read()[2] == 1 and moved != before
    refused("pf_gl_dyn_start_cable", text="the clock must be 0")
    assert run.everything() == moved


# ---------------------------------------------------------------------------------------------------------------------
# 7. solve_dynamic and the CLI
# ---------------------------------------------------------------------------------------------------------------------
def test_cli_cable_free_flight(tmp_path):
    """One slack cable flies freely: u = -(F / m)(n dt)^2 / 2 to the bit, -0.0078125 after 64 steps and -0.125 after 256, from
    the CLI and from solve_dynamic; the same file as a bar is held back."""
    from pinn_fem_amd.fem.dynamics import solve_dynamic
    out, parsed = run_cli(tmp_path, "cable_free_flight", parse=True)
    d = out["dynamics"]
    rec = [r[1] for r in d["recorded_displacements"]]
    print(f"free flight: recorded u {rec}, slack {d['slack_elements']}, strain energies {[e['strain'] for e in d['energies']]}")
    assert d["steps"] == 256 and d["dt"] == 2.0 ** -10
    assert rec == [-4.0 * (n * 2.0 ** -10) ** 2 / 2.0 for n in (0, 64, 128, 192, 256)] and rec[1] == -0.0078125
    assert out["displacements"] == [0.0, -0.125] and d["slack_elements"] == [0] and out["axial_forces"] == [0.0]
    assert [e["slack_elements"] for e in d["energies"]] == [0, 1, 1, 1, 1] and all(e["strain"] == 0.0 for e in d["energies"])
    assert d["residual_norm"] == 1.0                        # nothing holds the load
    config = parsed["dynamics"]["config"]
    res = solve_dynamic(parsed["model"], parsed["solver_config"], config)
    assert res.displacements.reshape(-1).tolist() == [0.0, -0.125] and res.slack.tolist() == [True]
    bar = solve_dynamic(parsed["model"], parsed["solver_config"], dataclasses.replace(config, cable_elements=None))
    print(f"the same file as a bar ends at {bar.displacements.reshape(-1)[1]:.3e}")
    assert abs(bar.displacements.reshape(-1)[1]) < 1e-2 and not bar.slack.any() and "slack_elements" not in bar.energies[-1]


def test_cli_guyed_mast_rests_without_its_slack_guy(tmp_path):
    """The damped run comes to rest with the leeward guy slack, on the Newton solution of the structure without it: u within
    1e-9 max |u| (the restatement's own run is at 3e-14 with this file's dt; the margin is for the device's different
    summation order moving the record point at which rest_tolerance trips, not a measured device figure), a residual below
    1e-9 of the load and an axial force of 0.0 in the slack guy.  The same file without cable_elements ends more than 1e-2
    away, and cable_elements = [] is the run without the key, to the bit.
    The file sets dt = 0.01, a tenth of the bound: rest_tolerance compares with the largest RECORDED kinetic energy, and at
    0.9 of the bound the first record comes after the motion has died down to 1e-9, 1e-26 of which is below the kinetic
    energy round-off of the residual leaves (2e-33 on the restatement)."""
    from pinn_fem_amd.fem.dynamics import solve_dynamic
    out, parsed = run_cli(tmp_path, "guyed_mast_slack", parse=True)
    M, nodes, el, fixed, e0 = gc.guyed_mast(2.0)
    reduced = gc.guyed_mast(2.0, elements=[0, 1])
    u_red, _, ok = gl.newton(nodes, reduced[2], M.loads, fixed, EA, 2, e0=reduced[4])
    u_bar, _, ok_bar = gl.newton(nodes, el, M.loads, fixed, EA, 2, e0=e0)
    d, u = out["dynamics"], np.array(out["displacements"])
    miss = np.max(np.abs(u - u_red)) / np.max(np.abs(u_red))
    print(f"mast: at rest {d['at_rest']} after {d['steps']} steps, slack {d['slack_elements']}, axial {out['axial_forces']}, "
          f"residual {d['residual_norm']:.2e}, miss {miss:.2e} max |u|, all-bar solution {np.max(np.abs(u - u_bar)):.2e} away")
    assert ok and ok_bar and d["at_rest"] and out["converged"] and d["steps"] < 20000
    assert d["slack_elements"] == [2] and out["axial_forces"][2] == 0.0 and min(out["axial_forces"][1], -out["axial_forces"][0]) > 0.0
    assert d["residual_norm"] <= 1e-9 * 2.0 and miss <= 1e-9
    assert np.max(np.abs(u - u_bar)) > 1e-2
    assert d["energies"][0]["slack_elements"] == 0 and d["energies"][-1]["slack_elements"] == 1
    assert np.allclose(np.array(out["reactions"])[[0, 4, 6]].sum(), -2.0, rtol=1e-9) and out["reactions"][6] == 0.0
    config = parsed["dynamics"]["config"]
    res = solve_dynamic(parsed["model"], parsed["solver_config"], config)
    assert res.at_rest and res.slack.tolist() == [False, False, True] and res.axial_forces[2] == 0.0
    assert np.array_equal(res.displacements.reshape(-1), u)
    bars = solve_dynamic(parsed["model"], parsed["solver_config"], dataclasses.replace(config, cable_elements=None))
    away = np.max(np.abs(bars.displacements.reshape(-1) - u_red))
    print(f"mast without cable_elements: at rest {bars.at_rest}, {away:.2e} from the reduced structure's solution")
    assert away > 1e-2 and not bars.slack.any() and bars.axial_forces[2] < 0.0
    short = dataclasses.replace(config, n_steps=300, rest_tolerance=None)
    a = solve_dynamic(parsed["model"], parsed["solver_config"], dataclasses.replace(short, cable_elements=None))
    b = solve_dynamic(parsed["model"], parsed["solver_config"], dataclasses.replace(short, cable_elements=[]))
    for x, y in ((a.displacements, b.displacements), (a.velocities, b.velocities), (a.recorded, b.recorded), (a.axial_forces, b.axial_forces)):
        assert x.tobytes() == y.tobytes()
    assert a.energies == b.energies and a.residual_norm == b.residual_norm
