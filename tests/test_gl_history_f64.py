"""Load and support-motion time histories in the explicit dynamics on the device: pf_gl_dyn_start_hist / _steps_hist /
_graph_create_hist called through the C ABI and held against the float64 restatement of tests/gl_history_reference.py (itself
pinned by tests/test_gl_history_host.py), then solve_dynamic and the CLI on a string under a load pulse and on a guyed mast
whose foundation is shaken.

On the free dofs the bounds are the bar step's own (test_gl_dynamics_f64.step_bounds, derived there from 2^-53 and operation
counts) with lam taken from the sample, an exact input; a fixed dof is one IEEE product, or the bytes of 0.0, and is compared
to the bit.  The measured figures are printed in front of every assertion.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import gl_cable_reference as gc
import gl_dynamics_reference as gd
import gl_history_reference as gh
from device_driver import EA, U53, GlTruss, flipped_chain_1d, gl_field, gl_system, run_cli, system_cache
from test_gl_cable_f64 import CableRun, changing_case
from test_gl_dynamics_f64 import DynRun, multi_step_case, restatement, same, step_bounds

pytestmark = pytest.mark.gpu

RAMP = (0.25, 1.5, 1.0)         # lam0, lam1, t_ramp of the runs without a load history


@pytest.fixture(scope="module")
def systems():
    yield from system_cache(gl_system)


class HistRun(DynRun):
    """DynRun through the _hist entry points: the histories' record and the cable flags (or null) ride behind pf_dyn.  lam,
    sup: sample arrays or None; amp: [n_dofs] or None; cable: flags or None (bars)."""

    def __init__(self, S, T, u, v, dt, lam=None, sup=None, amp=None, cable=None, n_samples=None, **kw):
        super().__init__(S, T, u, v, dt, **kw)
        dev = S.eng.device
        self.lam, self.sup, self.amp = (None if a is None else S.dev(a) for a in (lam, sup, amp))
        self.cable = None if cable is None else torch.from_numpy(
            np.ascontiguousarray(np.broadcast_to(cable, (S.ne,)), dtype=np.uint8)).to(dev)
        h = self.hist = self.capi.PfDynHist()
        h.lam, h.sup, h.sup_amp = (None if t is None else t.data_ptr() for t in (self.lam, self.sup, self.amp))
        h.n_samples = len(lam if lam is not None else sup) if n_samples is None else n_samples

    def tail(self):
        return C.byref(self.hist), None if self.cable is None else self.cable.data_ptr()

    def start(self):
        self.call("pf_gl_dyn_start_hist", *self.tail())

    def steps(self, n):
        self.call("pf_gl_dyn_steps_hist", *self.tail(), int(n))

    def graph(self, n):
        g = C.c_void_p()
        eng = self.S.eng
        with eng.on_stream():
            self.capi.check(eng.lib.pf_gl_dyn_graph_create_hist(eng._ref(), C.byref(self.S.rec), C.byref(self.rec), *self.tail(),
                                                                int(n), eng._stream(), C.byref(g)), "pf_gl_dyn_graph_create_hist")
        return g

    def everything(self):
        """DynRun's (u0, u1, v, clock) and every input array."""
        inputs = [t for t in (self.lam, self.sup, self.amp, self.cable, self.minv, self.f_ext) if t is not None]
        return super().everything() + b"".join(t.cpu().numpy().tobytes() for t in inputs)


def tables(S, rng, n_samples=16):
    """Seeded, non-constant histories, and amplitudes on about half of the fixed dofs (0.0 on the others; with more than one
    fixed dof at least one of each) and on every free dof, where they must not be read."""
    lam, sup = rng.uniform(0.25, 1.5, n_samples), rng.standard_normal(n_samples)
    amp = rng.standard_normal(S.n)
    amp[S.mask & (rng.random(S.n) < 0.5)] = 0.0
    if S.mask.sum() > 1:
        fixed = np.flatnonzero(S.mask)
        amp[fixed[0]], amp[fixed[1]] = 0.0, 0.37
    return lam, sup, amp


def check_hist_step(S, T, got_u, got_v, u, v, n, dt, alpha, lam, sup, amp, label):
    """One step against the restatement's from (u, v): the free dofs to step_bounds with lam = the sample (or the ramp), the
    fixed dofs to the bit: amp * sup[i(n + 1)] where amp != 0.0, the bytes of 0.0 elsewhere, and v = 0.0."""
    lam_n = gh.held(lam, n) if lam is not None else gd.load_factor(n * dt, *RAMP)
    (_, b_u), (_, b_v) = step_bounds(T, u, v, n, dt, alpha, lam_n, lam_n, 0.0)
    want_u, want_v = gh.step(T, u, v, n, dt, alpha, lam=lam, sup=None if sup is None else (amp, sup), ramp=RAMP)
    for what, got, want, bound in (("u", got_u, want_u, b_u), ("v", got_v, want_v, b_v)):
        assert np.all(np.isfinite(got)), what
        err = np.abs(got - want)
        print(f"{label} {what}: worst error / bound {np.max(err[S.free] / np.maximum(bound[S.free], 1e-300)):.3f}")
        assert np.all(err[S.free] <= bound[S.free]), what
        assert got[S.mask].tobytes() == want[S.mask].tobytes(), what
    assert want_v[S.mask].tobytes() == np.zeros(int(S.mask.sum())).tobytes()
    if sup is None:
        assert want_u[S.mask].tobytes() == np.zeros(int(S.mask.sum())).tobytes()
    else:
        s = gh.held(sup, n + 1)
        still = S.mask & (amp == 0.0)
        moved = S.mask & (amp != 0.0)
        assert want_u[still].tobytes() == np.zeros(int(still.sum())).tobytes() and np.array_equal(want_u[moved], (amp * s)[moved])
        assert S.mask.sum() < 2 or (still.any() and moved.any())


# ---------------------------------------------------------------------------------------------------------------------
# 5. one step and the start
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 4])
@pytest.mark.parametrize("cable", [False, True])
@pytest.mark.parametrize("which", ["load", "support", "both"])
@pytest.mark.parametrize("name", ["truss_257", "chain_257"])
def test_one_step_against_the_restatement(systems, name, which, cable, n):
    """The bar step's case (damping, a velocity, displacements that are not zero on the fixed dofs, e0 from +-1e-2) at an odd
    and an even clock with seeded 16-sample tables: a load history alone (the supports come out 0.0), a support history alone
    (lam is the ramp's), both; bars and the seeded half flagged.  The support sample of the odd clock, sup[6], is negative: a
    support that is not moved must still be the bytes of 0.0, not -0.0."""
    S = systems(name)
    rng = np.random.default_rng(S.ne + 61)
    u = np.where(S.free, 0.05 * rng.standard_normal(S.n), 0.1 * rng.standard_normal(S.n)) if cable else gl_field(S, "large", rng)
    v, e0 = 0.1 * rng.standard_normal(S.n), rng.uniform(-1e-2, 1e-2, S.ne)
    lam, sup, amp = tables(S, rng)
    sup[6], sup[5] = -abs(sup[6]) - 0.1, abs(sup[5]) + 0.1
    lam, sup = (lam if which != "support" else None), (sup if which != "load" else None)
    flags = gc.seeded_half(S.ne) if cable else None
    T = gc.with_cables(restatement(S, EA, e0), False if flags is None else flags)
    if cable:
        assert T.slack(u).any()
    dt, alpha = 0.5 * T.stable_time_step(u), 3.0
    assert n * dt < RAMP[2]
    run = HistRun(S, T, u, v, dt, lam, sup, None if sup is None else amp, flags, alpha=alpha, lam0=RAMP[0], lam1=RAMP[1],
                  t_ramp=RAMP[2], e0=e0, clock=n)
    run.steps(1)
    got_u, got_v, clock = run.read()
    assert clock == n + 1
    check_hist_step(S, T, got_u, got_v, u, v, n, dt, alpha, lam, sup, amp, f"{name} {which} cable {cable} n {n}")
    assert run.u[n & 1].cpu().numpy().tobytes() == np.ascontiguousarray(u).tobytes()        # u_n is only read
    # the sample is read: the neighbouring step's is another
    if lam is not None:
        other = gh.step(T, u, v, n + 1, dt, alpha, lam=lam, sup=None, ramp=RAMP)[1]
        assert np.max(np.abs(other - got_v)[S.free]) > 1e-9


@pytest.mark.parametrize("cable", [False, True])
def test_start_is_the_half_kick(systems, cable):
    """pf_gl_dyn_start_hist from (u_0, v_0): the step with c1 = 1 - alpha dt / 2 and g = dt / 2 (inside the step's bound: c1 <=
    1 and g <= dt), with lam[0], and the supports of step 1, sup[1], to the bit; the clock goes to 1; a second start is
    PF_ERR_ARG and changes nothing."""
    S = systems("truss_257")
    rng = np.random.default_rng(71)
    flags = gc.seeded_half(S.ne) if cable else None
    T = gc.with_cables(restatement(S), False if flags is None else flags)
    u, v = gl_field(S, "large", rng), 0.1 * rng.standard_normal(S.n)
    lam, sup, amp = tables(S, rng)
    dt, alpha = 0.5 * T.stable_time_step(u), 2.0
    run = HistRun(S, T, u, v, dt, lam, sup, amp, flags, alpha=alpha)
    run.start()
    got_u, got_v, clock = run.read()
    assert clock == 1
    want_u, want_v = gh.start(T, u, v, dt, alpha, lam=lam, sup=(amp, sup))
    (_, b_u), (_, b_v) = step_bounds(T, u, v, 0, dt, alpha, lam[0], lam[0], 0.0)
    for what, got, want, bound in (("u", got_u, want_u, b_u), ("v", got_v, want_v, b_v)):
        err = np.abs(got - want)
        print(f"start cable {cable} {what}: worst error / bound {np.max(err[S.free] / bound[S.free]):.3f}")
        assert np.all(err[S.free] <= bound[S.free]) and got[S.mask].tobytes() == want[S.mask].tobytes()
    assert np.array_equal(want_u[S.mask], np.where(amp != 0.0, amp * sup[1], 0.0)[S.mask]) and want_u[S.mask].any()
    before = run.everything()
    assert run.call("pf_gl_dyn_start_hist", *run.tail(), check=False) == S.capi.PF_ERR_ARG
    assert S.lib.pf_last_error().decode().startswith("pf_gl_dyn_start_hist: the clock must be 0")
    assert run.everything() == before


# ---------------------------------------------------------------------------------------------------------------------
# 6. holding the last sample
# ---------------------------------------------------------------------------------------------------------------------
def test_steps_beyond_the_table_hold_its_last_sample(systems):
    """n_samples = 3, eight steps from clock 0, every step held to the one-step rule from the device's own previous state:
    step n reads lam[min(n, 2)] and writes the supports at sup[min(n + 1, 2)].  The arrays are longer than n_samples says, with
    other values behind it: they are never read."""
    S = systems("truss_257")
    rng = np.random.default_rng(73)
    T = restatement(S)
    lam, sup, amp = tables(S, rng, 8)
    u, v = np.where(S.free, gl_field(S, "large", rng), amp * sup[0]), np.where(S.free, 0.1 * rng.standard_normal(S.n), 0.0)
    dt, alpha = 0.5 * T.stable_time_step(u), 0.5
    run = HistRun(S, T, u, v, dt, lam, sup, amp, n_samples=3, alpha=alpha)
    for n in range(8):
        run.steps(1)
        got_u, got_v, clock = run.read()
        assert clock == n + 1
        check_hist_step(S, T, got_u, got_v, u, v, n, dt, alpha, lam[:3], sup[:3], amp, f"held, step {n}")
        u, v = got_u, got_v
    assert np.array_equal(u[S.mask], np.where(amp != 0.0, amp * sup[2], 0.0)[S.mask])


# ---------------------------------------------------------------------------------------------------------------------
# 7. bit-for-bit identities
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cable", [False, True])
def test_constant_histories_are_the_plain_runs(systems, cable):
    """A lam array filled with lam1 gives the bits of the step-load run (t_ramp = 0) of pf_gl_dyn_steps; a sup array of zeros
    (under amplitudes that are not negative), and a sup_amp of zeros under a sup that is not, give the bits of the run with the
    supports at rest; with flags given the same against the _cable namesake.  u0, u1, v and the clock, start included."""
    S = systems("truss_257")
    if cable:
        T, flags, zero, dt = changing_case(S)
    else:
        (T, zero, dt), flags = multi_step_case(S), None
    rng = np.random.default_rng(43)
    u0, v0 = np.where(S.free, 1e-3 * rng.standard_normal(S.n), 0.0), np.where(S.free, 1e-2 * rng.standard_normal(S.n), 0.0)
    kw = dict(alpha=0.7, lam0=0.0, lam1=1.25, t_ramp=0.0)
    lam, sup, amp = tables(S, rng, 70)

    def plain(**more):
        return CableRun(S, T, u0, v0, dt, flags, **dict(kw, **more)) if cable else DynRun(S, T, u0, v0, dt, **dict(kw, **more))

    def go(run):
        run.start()
        run.steps(63)
        assert run.read()[2] == 64
        return DynRun.everything(run)

    want = go(plain())
    assert go(HistRun(S, T, u0, v0, dt, np.full(70, 1.25), None, None, flags, **dict(kw, lam1=-3.0))) == want
    ramped = dict(kw, t_ramp=40.5 * dt)
    want_ramped = go(plain(**ramped))
    assert want_ramped != want
    # (amplitudes >= 0 here: the moved support is the one product a * s, and a negative a times the sample +0.0 is -0.0: equal to
    # the support at rest, the free dofs to the bit, but not its bytes on that support)
    assert go(HistRun(S, T, u0, v0, dt, None, np.zeros(70), np.abs(amp), flags, **ramped)) == want_ramped
    signed = HistRun(S, T, u0, v0, dt, None, np.zeros(70), amp, flags, **ramped)
    signed_bytes, rest = go(signed), plain(**ramped)
    go(rest)
    assert (amp[S.mask] < 0.0).any() and signed_bytes != want_ramped and signed.read()[2] == rest.read()[2]
    for a, b in zip(signed.read()[:2], rest.read()[:2]):
        assert np.array_equal(a, b) and a[S.free].tobytes() == b[S.free].tobytes()
    assert go(HistRun(S, T, u0, v0, dt, None, -np.abs(sup) - 0.1, np.zeros(S.n), flags, **ramped)) == want_ramped
    assert go(HistRun(S, T, u0, v0, dt, np.full(70, 1.25), -np.abs(sup) - 0.1, np.where(S.free, amp, 0.0), flags, **kw)) == want
    # and the histories are read: these runs are others
    assert go(HistRun(S, T, u0, v0, dt, lam, None, None, flags, **kw)) != want
    assert go(HistRun(S, T, u0, v0, dt, None, sup, amp, flags, **ramped)) != want_ramped
    if cable:
        assert go(HistRun(S, T, u0, v0, dt, np.full(70, 1.25), None, None, None, **kw)) != want       # the flags are read too


def test_graph_replay_and_split_runs(systems):
    """With both histories and the seeded half flagged: a 5-step graph replayed three times equals 15 eager steps (a replay
    reads the samples of the steps it stands at), and a run split 7 + 8 equals 15 at once.  Capture runs nothing: the clock
    stays 0 and the buffer the clock does not point to keeps its fill value."""
    S = systems("truss_257")
    T, flags, zero, dt = changing_case(S)
    rng = np.random.default_rng(79)
    lam, sup, amp = tables(S, rng, 12)                 # 12 samples: the last steps hold the last one
    amp = 1e-2 * amp
    u0 = gh.supports(T, (amp, sup), 0)

    def make():
        return HistRun(S, T, u0, zero, dt, lam, sup, amp, flags, alpha=0.3)

    eager = make()
    eager.steps(15)
    want = eager.read()
    assert want[2] == 15 and np.max(np.abs(want[0][S.free])) > 1e-4
    one = make()
    g = one.graph(5)
    try:
        assert one.read()[2] == 0 and one.read()[0].tobytes() == u0.tobytes() and bool((one.u[1] == 7.0).all())
        one.replay(g, times=3)
        assert same(one.read(), want) and one.everything() == eager.everything()
    finally:
        S.lib.pf_graph_destroy(g)
    split = make()
    split.steps(7)
    assert split.read()[2] == 7
    split.steps(8)
    assert same(split.read(), want) and split.everything() == eager.everything()
    shifted = HistRun(S, T, u0, zero, dt, np.roll(lam, 1), sup, amp, flags, alpha=0.3)
    shifted.steps(15)
    assert not same(shifted.read(), want)               # a wrong index shows


# ---------------------------------------------------------------------------------------------------------------------
# 8. many steps against the restatement
# ---------------------------------------------------------------------------------------------------------------------
def many_steps_case(S, n_steps):
    """The state-changing case of the cable tests (a step load of 20 x standard normal from rest, half the bound, the seeded
    half flagged) under a load history with the values 0.5, 1 and 2 and supports shaken by 2e-2 x standard normal amplitudes.
    The load factors are powers of two because the unit of the many-step rule, the restatement's ascending-against-descending
    spread, holds summation order alone: the bar's and the cable's many-step tests run at lam = 1, where lam F is exact.
    A lam whose product with F rounds adds the difference between the device's fused lam F - f_int and numpy's two roundings,
    which no reordering shows.  On the CPU alone, fusing that one expression in the restatement (in extended precision) moves
    its 64-step run by 4.8 / 6.8 spreads in u / v with lam drawn from 0.5 .. 1.5, and by nothing with powers of two (the first
    device run, with lam in 0.5 .. 1.5, stood at 2.7 / 8.8 spreads).  The one-step tests hold rounding load factors to the
    derived bound."""
    T, flags, zero, dt = changing_case(S)
    rng = np.random.default_rng(83)
    t = np.arange(n_steps + 2) * dt
    lam = np.exp2(np.round(np.log2(1.0 + 0.5 * np.sin(40.0 * t + 1.0) * rng.uniform(0.5, 1.0, t.size))))
    assert set(lam.tolist()) == {0.5, 1.0, 2.0}
    sup = np.sin(55.0 * t) + 0.1 * rng.standard_normal(t.size)
    amp = np.where(S.mask & (rng.random(S.n) < 0.5), 2e-2 * rng.standard_normal(S.n), 0.0)
    return T, flags, dt, lam, sup, amp


@pytest.mark.parametrize("n_steps", [64, 256])
def test_many_steps_against_the_restatement(systems, n_steps):
    """The bar's rule and the bar's factor with both histories and half the elements flagged: device - restatement <= 8 x the
    restatement's own ascending-against-descending summation spread after 64 and 256 steps (max norm of u and of v), and
    device and restatement decide no element's slack state differently at the end (with this seed the restatement's two
    orders agree on every element, checked on the CPU).  The measured ratios are in profiles/."""
    S = systems("truss_257")
    T, flags, dt, lam, sup, amp = many_steps_case(S, n_steps)
    zero, u0 = np.zeros(S.n), gh.supports(T, (amp, sup), 0)
    run = HistRun(S, T, u0, zero, dt, lam, sup, amp, flags)
    run.steps(n_steps)
    got_u, got_v, clock = run.read()
    assert clock == n_steps
    kw = dict(lam=lam, sup=(amp, sup))
    asc, desc = gh.run(T, u0, zero, 0, n_steps, dt, **kw), gh.run(T, u0, zero, 0, n_steps, dt, descending=True, **kw)
    assert got_u[S.mask].tobytes() == asc[0][S.mask].tobytes() and np.abs(got_u[S.mask]).max() > 1e-3
    assert np.array_equal(T.slack(asc[0]), T.slack(desc[0])) and T.slack(asc[0]).sum() > 20
    print(f"{n_steps} steps: {int(T.slack(asc[0]).sum())} elements slack on the restatement, "
          f"{int((T.slack(asc[0]) != T.slack(got_u)).sum())} decided otherwise at the device's state")
    for what, got, a, d in (("u", got_u, asc[0], desc[0]), ("v", got_v, asc[1], desc[1])):
        spread, err = np.max(np.abs(a - d)), np.max(np.abs(got - a))
        print(f"{n_steps} steps {what}: max |{what}| {np.max(np.abs(a)):.3f}, spread {spread:.3e}, device - restatement "
              f"{err:.3e}, ratio {err / spread:.3f}")
        assert spread > 0.0 and err <= 8.0 * spread
    assert np.array_equal(T.slack(asc[0]), T.slack(got_u))


# ---------------------------------------------------------------------------------------------------------------------
# 9. the grid-stride loop
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_nodes, n_steps", [(70_001, 4), (300_001, 2)])
def test_long_chain_step_by_step(n_nodes, n_steps):
    """A 1-D chain of 70 001 nodes (274 workgroups) for four steps, and one of 300 001 nodes for two: more nodes than the 1024
    workgroups of 256 threads the node kernels launch, so every thread takes a second node.  Held at both ends, both ends
    moved, under a load history; both parities of the ping-pong, each step held to the one-step rule from the device's own
    previous state.  The far support is the last dof: an index that is right only in the first sweep leaves it wrong."""
    rng = np.random.default_rng(n_nodes)
    x, el, _ = flipped_chain_1d(n_nodes - 1, rng)
    S = GlTruss(x, el, np.array([0, n_nodes - 1]), 1)
    assert S.n_nodes == n_nodes and S.mask[0] and S.mask[-1] and S.mask.sum() == 2
    T = restatement(S)
    lam, sup = rng.uniform(0.25, 1.5, 6), rng.standard_normal(6)
    amp = rng.standard_normal(S.n)
    amp[0], amp[-1] = 0.4, -0.3
    u, v = gl_field(S, "large", rng), 0.1 * rng.standard_normal(S.n)
    u[S.mask], v[S.mask] = (amp * sup[0])[S.mask], 0.0
    dt, alpha = 0.5 * T.stable_time_step(u), 0.5
    run = HistRun(S, T, u, v, dt, lam, sup, amp, alpha=alpha)
    for n in range(n_steps):
        run.steps(1)
        got_u, got_v, clock = run.read()
        assert clock == n + 1
        lam_n = gh.held(lam, n)
        (_, b_u), (_, b_v) = step_bounds(T, u, v, n, dt, alpha, lam_n, lam_n, 0.0)
        want_u, want_v = gh.step(T, u, v, n, dt, alpha, lam=lam, sup=(amp, sup))
        for what, got, want, bound in (("u", got_u, want_u, b_u), ("v", got_v, want_v, b_v)):
            err = np.abs(got - want)
            print(f"{n_nodes} nodes, step {n} {what}: worst error / bound {np.max(err[S.free] / np.maximum(bound[S.free], 1e-300)):.3f}")
            assert np.all(np.isfinite(got)) and np.all(err[S.free] <= bound[S.free])
            assert got[S.mask].tobytes() == want[S.mask].tobytes()
        assert got_u[0] == 0.4 * sup[n + 1] and got_u[-1] == -0.3 * sup[n + 1]
        u, v = got_u, got_v
    del S
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------------
# 10. argument errors
# ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors_touch_nothing(systems):
    """A null hist, lam and sup both null, sup without sup_amp, n_samples < 1, and everything the namesakes refuse (a null
    pointer in pf_dyn, dt, alpha, t_ramp, a non-finite load factor, a bad mesh, no d0, n_steps < 1, a null graph_out, a clock
    that is not 0 at the start): PF_ERR_ARG with a message that begins with the function's name, before anything is enqueued;
    u0, u1, v, the clock and every input stay as they were, byte for byte.  A null cable is no error here: it means bars."""
    S = systems("chain_257")
    T = restatement(S)
    rng = np.random.default_rng(89)
    lam, sup, amp = tables(S, rng)
    run = HistRun(S, T, rng.standard_normal(S.n), rng.standard_normal(S.n), 1e-3, lam, sup, amp, gc.seeded_half(S.ne), alpha=0.5,
                  lam0=0.0, lam1=1.0, t_ramp=0.25)
    before = run.everything()
    graph = C.c_void_p()
    entry = {"pf_gl_dyn_start_hist": (), "pf_gl_dyn_steps_hist": (1,)}
    names = list(entry) + ["pf_gl_dyn_graph_create_hist"]

    def refused(name, text, rec=None, hist=run.hist, problem=None, args=None, gl_rec=None, graph_out=C.byref(graph)):
        eng = S.eng
        rec = run.rec if rec is None else rec
        problem = eng._ref() if problem is None else problem
        gl_rec = C.byref(S.rec) if gl_rec is None else gl_rec
        h = None if hist is None else C.byref(hist)
        with eng.on_stream():
            if name == "pf_gl_dyn_graph_create_hist":
                rc = eng.lib.pf_gl_dyn_graph_create_hist(problem, gl_rec, C.byref(rec), h, run.cable.data_ptr(),
                                                         1 if args is None else args[0], eng._stream(), graph_out)
            else:
                rc = getattr(eng.lib, name)(problem, gl_rec, C.byref(rec), h, run.cable.data_ptr(),
                                            *(entry[name] if args is None else args), eng._stream())
        assert rc == S.capi.PF_ERR_ARG, (name, text, rc)
        assert S.lib.pf_last_error().decode().startswith(name + ": " + text), S.lib.pf_last_error()
        assert not graph

    def changed(kind, source, **fields):
        rec = kind()
        C.memmove(C.byref(rec), C.byref(source), C.sizeof(rec))
        for key, value in fields.items():
            setattr(rec, key, value)
        return rec

    for name in names:
        refused(name, "null hist", hist=None)
        refused(name, "hist holds neither lam nor sup", hist=changed(S.capi.PfDynHist, run.hist, lam=None, sup=None))
        refused(name, "sup without sup_amp", hist=changed(S.capi.PfDynHist, run.hist, sup_amp=None))
        for n in (0, -1):
            refused(name, "n_samples", hist=changed(S.capi.PfDynHist, run.hist, n_samples=n))
        for pointer in ("minv", "f_ext", "u0", "u1", "v", "clock"):
            refused(name, "null pointer", rec=changed(S.capi.PfDyn, run.rec, **{pointer: None}))
        for bad, text in ((dict(dt=0.0), "dt"), (dict(dt=-1e-3), "dt"), (dict(dt=float("nan")), "dt"), (dict(dt=float("inf")), "dt"),
                          (dict(alpha=-1.0), "alpha"), (dict(t_ramp=-1.0), "t_ramp"), (dict(lam1=float("inf")), "non-finite")):
            refused(name, text, rec=changed(S.capi.PfDyn, run.rec, **bad))
        bad_mesh = changed(S.capi.PfProblem, S.eng.P)
        bad_mesh.mesh.n_dofs += 1
        refused(name, "bad mesh", problem=C.byref(bad_mesh))
        refused(name, "null pointer", gl_rec=C.byref(S.capi.PfGl()))
    for name in ("pf_gl_dyn_steps_hist", "pf_gl_dyn_graph_create_hist"):
        for n in (0, -3):
            refused(name, "n_steps", args=(n,))
    refused("pf_gl_dyn_graph_create_hist", "null pointer", graph_out=None)
    assert run.everything() == before
    # the record itself is good, with and without flags: one step goes through, and then a start is refused
    bars = HistRun(S, T, rng.standard_normal(S.n), rng.standard_normal(S.n), 1e-3, lam, sup, amp)
    bars.steps(1)
    run.steps(1)
    moved = run.everything()
    assert run.read()[2] == 1 and bars.read()[2] == 1 and moved != before
    refused("pf_gl_dyn_start_hist", "the clock must be 0")
    assert run.everything() == moved


# ---------------------------------------------------------------------------------------------------------------------
# 11. solve_dynamic and the CLI
# ---------------------------------------------------------------------------------------------------------------------
def test_cli_taut_string_pulse(tmp_path):
    """A triangular load pulse (0 -> 1 -> 0 over 0.4) at mid-span of the 8-element string, 300 steps of 0.004: every record's
    load_factor is the sample of its step (production's to the bit, the restatement's within the sampling's 4 x 2^-53), the
    work is that sample times f.u, and the closing residual is taken with the last sample, 0: it is max |f_int| on the free dofs
    (held to the restatement's f_int at the returned state within the bound of two sums, step_bounds' first line), not max |F -
    f_int|.  solve_dynamic gives the CLI's numbers."""
    from pinn_fem_amd.fem.dynamics import history_samples, solve_dynamic
    out, parsed = run_cli(tmp_path, "taut_string_pulse", parse=True)
    d = out["dynamics"]
    config = parsed["dynamics"]["config"]
    T, _, _ = gd.string()
    T.loads = np.asarray(parsed["model"].loads, dtype=np.float64).reshape(-1)
    assert T.loads[9] == 0.01 and d["steps"] == 300 and d["dt"] == 0.004
    records = list(range(0, 301, 25))
    assert d["times"] == [n * 0.004 for n in records]
    prod = history_samples(config.load_history, np.arange(302, dtype=np.float64) * 0.004)
    ref = gh.sample(config.load_history, 302, 0.004)
    got = [e["load_factor"] for e in d["energies"]]
    print(f"pulse: load factors {got}, mid-span record {[r[0] for r in d['recorded_displacements']]}")
    assert got == [float(prod[n]) for n in records] and np.max(np.abs(np.array(got) - ref[records])) <= 4 * U53
    assert got[0] == 0.0 and 0.4 < got[1] < 0.6 and got[2] == 1.0 and 0.4 < got[3] < 0.6 and got[4:] == [0.0] * 9
    assert max(abs(r[0]) for r in d["recorded_displacements"]) > 1e-4
    u = np.array(out["displacements"])
    for e, rec in zip(d["energies"], d["recorded_displacements"]):
        assert e["work"] == e["load_factor"] * (0.01 * rec[0]) or abs(e["work"] - e["load_factor"] * 0.01 * rec[0]) <= 4 * U53 * abs(e["work"])
    f_int = T.f_int(u)
    bound = np.max(((2 * T.degree + 24) * U53 * T.f_int_scale(u))[T.free])
    with_load = np.max(np.abs(T.loads - f_int)[T.free])
    print(f"pulse: residual {d['residual_norm']:.6e}, max |f_int| {np.max(np.abs(f_int[T.free])):.6e}, with lam = 1 it were "
          f"{with_load:.6e}; bound {bound:.2e}")
    assert abs(d["residual_norm"] - np.max(np.abs(f_int[T.free]))) <= bound and abs(with_load - d["residual_norm"]) > 1e-4
    ref_u, _ = gh.solve(T, 0.004, 300, lam=ref)
    print(f"pulse: max |u - restatement's run| {np.max(np.abs(u - ref_u)):.3e} at max |u| {np.max(np.abs(ref_u)):.3e}")
    res = solve_dynamic(parsed["model"], parsed["solver_config"], config)
    assert np.array_equal(res.displacements.reshape(-1), u) and res.steps == 300
    assert [e["load_factor"] for e in res.energies] == got


def test_cli_guyed_mast_shaken(tmp_path):
    """The guyed mast with its three supports shaken sideways by 0.02 sin(2 pi t) (a 41-knot table), cables on, 190 steps of
    0.01: the moved dofs end at amplitude x s(t_end) to the bit (a negative sample), the other supports at the bytes of 0.0,
    the free dofs within 8 x the restatement's own ascending-against-descending spread of its run of the same file, and the
    slack set at the end is the restatement's (its two orders agree on it).  On the restatement the guys are slack in 60 and
    127 of the steps."""
    from pinn_fem_amd.fem.dynamics import history_samples, solve_dynamic
    out, parsed = run_cli(tmp_path, "guyed_mast_shaken", parse=True)
    d, config = out["dynamics"], parsed["dynamics"]["config"]
    m = config.support_motion
    M = gc.guyed_mast(0.5)[0]
    assert np.array_equal(M.loads, np.asarray(parsed["model"].loads).reshape(-1)) and d["steps"] == 190 and d["dt"] == 0.01
    amp = np.zeros(8)
    amp[m.dofs] = m.amplitudes
    prod = history_samples(m.history, np.arange(192, dtype=np.float64) * 0.01)
    ref = gh.sample(m.history, 192, 0.01)
    u = np.array(out["displacements"])
    assert prod[190] < -0.5 and np.max(np.abs(prod - ref)) <= 4 * U53
    assert u[[0, 4, 6]].tolist() == [0.02 * float(prod[190])] * 3 and u[[1, 5, 7]].tobytes() == np.zeros(3).tobytes()
    assert not np.array(d["velocities"])[[0, 1, 4, 5, 6, 7]].any()
    kw = dict(alpha=config.damping, sup=(amp, ref))
    asc, desc = gh.solve(M, 0.01, 190, **kw), gh.solve(M, 0.01, 190, descending=True, **kw)
    free = M.free
    for what, got, a, b in (("u", u, asc[0], desc[0]), ("v", np.array(d["velocities"]), asc[1], desc[1])):
        spread, err = np.max(np.abs(a - b)[free]), np.max(np.abs(got - a)[free])
        print(f"mast {what}: max |{what}| {np.max(np.abs(a[free])):.3e}, spread {spread:.3e}, device - restatement {err:.3e}, "
              f"ratio {err / spread:.3f}")
        assert spread > 0.0 and err <= 8.0 * spread
    slack = M.slack(asc[0])
    print(f"mast: slack at the end {d['slack_elements']}, restatement {np.flatnonzero(slack).tolist()}, records "
          f"{[e['slack_elements'] for e in d['energies']]}")
    assert np.array_equal(slack, M.slack(desc[0])) and slack.tolist() == [False, False, True]
    assert d["slack_elements"] == np.flatnonzero(slack).tolist() and out["axial_forces"][2] == 0.0 and out["axial_forces"][1] > 0.0
    assert d["times"] == [n * 0.01 for n in (0, 50, 100, 150, 190)]
    res = solve_dynamic(parsed["model"], parsed["solver_config"], config)
    assert np.array_equal(res.displacements.reshape(-1), u) and res.slack.tolist() == slack.tolist()
