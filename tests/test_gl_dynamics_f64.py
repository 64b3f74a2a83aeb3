"""Explicit dynamics of Green-Lagrange trusses on the device: pf_gl_dyn_start / _steps / _graph_create / _energy called
through the C ABI and held against the float64 restatement of tests/gl_dynamics_reference.py (itself pinned by
tests/test_gl_dynamics_host.py), then solve_dynamic and the CLI on a vibrating string and a snapping two-bar truss.

Every bound is derived next to its assertion from 2^-53 and operation counts, or is the stated multiple of the
restatement's own summation spread.  The measured figures are printed in front of every assertion.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import gl_dynamics_reference as gd
import gl_reference as gl
from device_driver import EA, U53, GlTruss, flipped_chain_1d, gl_field, gl_system, run_cli, system_cache

pytestmark = pytest.mark.gpu

AREA_DENSITY = 0.5      # rho A of device_driver's material: area 0.5, density 1.0


@pytest.fixture(scope="module")
def systems():
    yield from system_cache(gl_system)


def restatement(S, ea=EA, e0=None, seed=0):
    """S as a gd.Truss with rho A = 1 and standard-normal loads."""
    loads = np.random.default_rng(100 + seed).standard_normal(S.n)
    return gd.Truss(S.nodes, S.el, S.fixed, S.dim, ea, e0, gd.lumped_mass(S.nodes, S.el, 1.0, S.dim), loads)


class DynRun:
    """One pf_dyn record with test-owned buffers.  The displacement buffer the clock does not point to is filled with 7.0, so
    what a launch does not write stays visible."""

    def __init__(self, S, T, u, v, dt, alpha=0.0, lam0=1.0, lam1=1.0, t_ramp=0.0, ea=None, e0=None, clock=0, minv=None):
        self.S, self.capi = S, S.capi
        dev = S.eng.device
        self.minv, self.f_ext = S.dev(1.0 / T.mass if minv is None else minv), S.dev(T.loads)
        self.u = [torch.full((S.n,), 7.0, dtype=torch.float64, device=dev) for _ in range(2)]
        self.u[clock & 1].copy_(S.dev(u))
        self.v = S.dev(v).clone()
        self.clock = torch.tensor([clock], dtype=torch.int64, device=dev)
        self.ea, self.e0 = (None if a is None else S.dev(np.broadcast_to(a, (S.ne,))) for a in (ea, e0))
        self.out = torch.full((self.capi.PF_DYN_ENERGY_COUNT,), 7.0, dtype=torch.float64, device=dev)
        r = self.rec = self.capi.PfDyn()
        r.minv, r.f_ext, r.u0, r.u1, r.v = (t.data_ptr() for t in (self.minv, self.f_ext, self.u[0], self.u[1], self.v))
        r.ea, r.e0 = (None if t is None else t.data_ptr() for t in (self.ea, self.e0))
        r.clock = self.clock.data_ptr()
        r.dt, r.alpha, r.lam0, r.lam1, r.t_ramp = dt, alpha, lam0, lam1, t_ramp

    def call(self, name, *args, rec=None, problem=None, check=True):
        eng = self.S.eng
        with eng.on_stream():
            rc = getattr(eng.lib, name)(eng._ref() if problem is None else problem, C.byref(self.S.rec),
                                        C.byref(self.rec if rec is None else rec), *args, eng._stream())
        if check:
            self.capi.check(rc, name)
        return rc

    def start(self):
        self.call("pf_gl_dyn_start")

    def steps(self, n):
        self.call("pf_gl_dyn_steps", int(n))

    def graph(self, n):
        g = C.c_void_p()
        eng = self.S.eng
        with eng.on_stream():
            self.capi.check(eng.lib.pf_gl_dyn_graph_create(eng._ref(), C.byref(self.S.rec), C.byref(self.rec), int(n),
                                                           eng._stream(), C.byref(g)), "pf_gl_dyn_graph_create")
        return g

    def replay(self, g, times=1):
        eng = self.S.eng
        with eng.on_stream():
            for _ in range(times):
                self.capi.check(eng.lib.pf_graph_launch(g, eng._stream()), "pf_graph_launch")

    def energy(self):
        self.call("pf_gl_dyn_energy", self.out.data_ptr())
        torch.cuda.synchronize()
        return self.out[:4].cpu().numpy()

    def read(self):
        """(u at the clock, v, clock) on the host."""
        torch.cuda.synchronize()
        n = int(self.clock.cpu()[0])
        return self.u[n & 1].cpu().numpy(), self.v.cpu().numpy(), n

    def everything(self):
        torch.cuda.synchronize()
        return b"".join(t.cpu().numpy().tobytes() for t in (self.u[0], self.u[1], self.v, self.clock))


def same(a, b):
    return a[2] == b[2] and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# 1. one step to a derived bound
# ---------------------------------------------------------------------------------------------------------------------
def step_bounds(T, u, v, n, dt, alpha, lam0, lam1, t_ramp):
    """(u_next, v_next) of the restatement and their round-off bounds for device and restatement together, in units of
    2^-53 (U53).  `scale` is T.f_int_scale: per dof the sum of the magnitudes E A (e_abs + |e0|) (|d0| + |du|) / l0 the terms are
    formed from, in front of every cancellation.
      a term: e 8, e - e0 2, the chain (N, l0, the division, d, the product) 14 for both sides (tests/test_gl_e0_f64.py): 24
      f_int: one rounding per accumulated incidence and side: (2 degree + 24) scale
      r = lam F - f_int: lam (its own product may be contracted) and lam F 6 |lam F|, the difference 2 (|lam F| + scale)
      a = r minv against r / m: 3 on (|lam F| + scale) / m
      v' = c1 v + g a: two products, a sum and the coefficients, 6 on |c1 v| + g |a|
      u' = u + dt v': a product and a sum on both sides, 4 on |u| + dt |v'|."""
    h = 0.5 * alpha * dt
    c1, g = (1.0 - h) / (1.0 + h), dt / (1.0 + h)
    lam = gd.load_factor(n * dt, lam0, lam1, t_ramp)
    scale, lf = T.f_int_scale(u), np.abs(lam * T.loads)
    b_r = (2 * T.degree + 24) * U53 * scale + 6 * U53 * lf + 2 * U53 * (lf + scale)
    a_mag = (lf + scale) / T.mass
    b_a = b_r / T.mass + 3 * U53 * a_mag
    v_mag = np.abs(c1 * v) + g * a_mag
    b_v = g * b_a + 6 * U53 * v_mag
    b_u = dt * b_v + 4 * U53 * (np.abs(u) + dt * v_mag)
    u_next, v_next = T.step(u, v, n, dt, alpha, lam0, lam1, t_ramp)
    return (u_next, b_u), (v_next, b_v)


def check_step(S, T, got_u, got_v, u, v, n, dt, alpha, lam0, lam1, t_ramp, label):
    (want_u, b_u), (want_v, b_v) = step_bounds(T, u, v, n, dt, alpha, lam0, lam1, t_ramp)
    for what, got, want, bound in (("u", got_u, want_u, b_u), ("v", got_v, want_v, b_v)):
        assert np.all(np.isfinite(got)), what
        err = np.abs(got - want)
        print(f"{label} {what}: worst error / bound {np.max(err[S.free] / np.maximum(bound[S.free], 1e-300)):.3f}")
        assert np.all(err[S.free] <= bound[S.free]), what
        assert not got[S.mask].any() and got[S.mask].tobytes() == np.zeros(int(S.mask.sum())).tobytes(), what


@pytest.mark.parametrize("field", ["random", "cancelling"])
@pytest.mark.parametrize("name", ["truss_257", "chain_257"])
def test_one_step_against_the_restatement(systems, name, field):
    """The 257-element irregular truss (121 nodes, hubs of odd and even degree) and a flipped 1-D chain; an odd step number
    inside the load ramp, damping, a velocity and displacements that are not zero on the fixed dofs (which come out exactly
    0.0).  random: e0 drawn per element from +-1e-2; cancelling: e0 equal to the strain of the field, so every N is
    round-off of e alone and the bound (stated in e_abs + |e0|, not in e - e0) is all that is left."""
    S = systems(name)
    if name == "truss_257":
        assert S.n_nodes == 121
        high = S.degree[::2][S.degree[::2] >= 5]
        assert (high % 2 == 1).any() and (high % 2 == 0).any()
    rng = np.random.default_rng(S.ne + 31)
    u, v = gl_field(S, "large", rng), 0.1 * rng.standard_normal(S.n)
    e0 = rng.uniform(-1e-2, 1e-2, S.ne)
    if field == "cancelling":
        e0 = restatement(S).strain(u)[0].copy()
    T = restatement(S, EA, e0)
    dt, alpha, lam0, lam1, t_ramp, n = 0.5 * T.stable_time_step(u), 3.0, 0.25, 1.5, 1.0, 5
    assert n * dt < t_ramp
    run = DynRun(S, T, u, v, dt, alpha, lam0, lam1, t_ramp, e0=e0, clock=n)
    run.steps(1)
    got_u, got_v, clock = run.read()
    assert clock == n + 1
    check_step(S, T, got_u, got_v, u, v, n, dt, alpha, lam0, lam1, t_ramp, f"{name} {field}")
    assert run.u[n & 1].cpu().numpy().tobytes() == np.ascontiguousarray(u).tobytes()        # u_n is only read
    if field == "cancelling":
        f_scale = T.f_int_scale(u)
        print(f"{name} cancelling: max |f_int| of the restatement {np.max(np.abs(T.f_int(u))):.2e}, scale {np.max(f_scale):.2e}")
        assert np.max(np.abs(T.f_int(u))) <= 1e-12 * np.max(f_scale)


def test_start_is_the_half_kick(systems):
    """pf_gl_dyn_start from (u_0, v_0): the step with c1 = 1 - alpha dt / 2 and g = dt / 2, held to the one-step bound with
    those coefficients; the clock goes to 1; a second start (the clock is 1) is PF_ERR_ARG and changes nothing."""
    S = systems("truss_257")
    rng = np.random.default_rng(41)
    T = restatement(S)
    u, v = gl_field(S, "large", rng), 0.1 * rng.standard_normal(S.n)
    dt, alpha = 0.5 * T.stable_time_step(u), 2.0
    run = DynRun(S, T, u, v, dt, alpha)
    run.start()
    got_u, got_v, clock = run.read()
    assert clock == 1
    want_u, want_v = T.start(u, v, dt, alpha)
    (_, b_u), (_, b_v) = step_bounds(T, u, v, 0, dt, alpha, 1.0, 1.0, 0.0)          # c1 <= 1 and g <= dt: the step's bound holds
    for what, got, want, bound in (("u", got_u, want_u, b_u), ("v", got_v, want_v, b_v)):
        err = np.abs(got - want)
        print(f"start {what}: worst error / bound {np.max(err[S.free] / bound[S.free]):.3f}")
        assert np.all(err[S.free] <= bound[S.free]) and not got[S.mask].any()
    before = run.everything()
    assert run.call("pf_gl_dyn_start", check=False) == S.capi.PF_ERR_ARG
    assert S.lib.pf_last_error().decode().startswith("pf_gl_dyn_start: the clock must be 0")
    assert run.everything() == before


# ---------------------------------------------------------------------------------------------------------------------
# 2. the grid-stride loop
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_nodes, n_steps", [(70_001, 16), (300_001, 4)])
def test_long_chain_step_by_step(n_nodes, n_steps):
    """A 1-D chain of 70 001 nodes (274 workgroups) for 16 steps, and one of 300 001 nodes for 4: more nodes than the 1024
    workgroups of 256 threads the node kernels launch, so every thread takes a second node.  Every step is held to the
    one-step bound against the restatement's step from the device's own previous state (downloaded after every launch), so
    the sixteen are checked one by one, both parities of the ping-pong included; the whole run is printed against the
    restatement's own run."""
    rng = np.random.default_rng(n_nodes)
    S = GlTruss(*flipped_chain_1d(n_nodes - 1, rng), 1)
    assert S.n_nodes == n_nodes
    T = restatement(S)
    u, v = gl_field(S, "large", rng), 0.1 * rng.standard_normal(S.n)
    u[S.mask], v[S.mask] = 0.0, 0.0
    dt, alpha = 0.5 * T.stable_time_step(u), 0.5
    run = DynRun(S, T, u, v, dt, alpha)
    ref_u, ref_v = u, v
    for n in range(n_steps):
        run.steps(1)
        got_u, got_v, clock = run.read()
        assert clock == n + 1
        check_step(S, T, got_u, got_v, u, v, n, dt, alpha, 1.0, 1.0, 0.0, f"{n_nodes} nodes, step {n}")
        ref_u, ref_v = T.step(ref_u, ref_v, n, dt, alpha)
        u, v = got_u, got_v
    print(f"{n_nodes} nodes: after {n_steps} steps max |u - restatement's run| {np.max(np.abs(u - ref_u)):.3e} at max |u| "
          f"{np.max(np.abs(u)):.3e}")
    del S
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------------
# 3. many steps against the restatement
# ---------------------------------------------------------------------------------------------------------------------
def multi_step_case(S):
    """A step load of 20 x standard normal from rest at half the bound of the undeformed truss."""
    T = restatement(S)
    T.loads = 20.0 * T.loads
    zero = np.zeros(S.n)
    return T, zero, 0.5 * T.stable_time_step(zero)


@pytest.mark.parametrize("n_steps", [64, 256])
def test_many_steps_against_the_restatement(systems, n_steps):
    """device - restatement <= 8 x the restatement's own ascending-against-descending summation spread after 64 and 256 steps
    (max norm of u and of v).  The factor 8 covers the contraction of products and sums into FMAs, which a reordered sum
    does not show.  The measured ratios are in profiles/."""
    S = systems("truss_257")
    T, zero, dt = multi_step_case(S)
    run = DynRun(S, T, zero, zero, dt)
    run.steps(n_steps)
    got_u, got_v, clock = run.read()
    assert clock == n_steps
    asc, desc = T.run(zero, zero, 0, n_steps, dt), T.run(zero, zero, 0, n_steps, dt, descending=True)
    for what, got, a, d in (("u", got_u, asc[0], desc[0]), ("v", got_v, asc[1], desc[1])):
        spread, err = np.max(np.abs(a - d)), np.max(np.abs(got - a))
        print(f"{n_steps} steps {what}: max |{what}| {np.max(np.abs(a)):.3f}, spread {spread:.3e}, device - restatement "
              f"{err:.3e}, ratio {err / spread:.3f}")
        assert spread > 0.0 and err <= 8.0 * spread


# ---------------------------------------------------------------------------------------------------------------------
# 4. bit-for-bit identities
# ---------------------------------------------------------------------------------------------------------------------
def test_bit_for_bit_identities(systems):
    """Graph replay equals eager launches; two graphs of 32 steps equal one of 64; a repeated run equals itself; an odd step
    count followed by more steps equals one run (the parity of the ping-pong); e0 of all zeros gives the bits of e0 = None;
    ea filled with the model's E*A gives the bits of ea = None."""
    S = systems("truss_257")
    T, zero, dt = multi_step_case(S)
    rng = np.random.default_rng(43)
    u0, v0 = np.where(S.free, 1e-3 * rng.standard_normal(S.n), 0.0), np.where(S.free, 1e-2 * rng.standard_normal(S.n), 0.0)
    kw = dict(alpha=0.7, lam0=0.0, lam1=1.0, t_ramp=40.5 * dt)

    def make(**more):
        return DynRun(S, T, u0, v0, dt, **dict(kw, **more))

    eager = make()
    eager.steps(64)
    want = eager.read()
    assert want[2] == 64 and np.max(np.abs(want[0])) > 1e-3
    graphs = []
    try:
        one = make()
        graphs.append(one.graph(64))
        assert one.read()[2] == 0 and one.read()[0].tobytes() == np.ascontiguousarray(u0).tobytes()    # capture runs nothing
        one.replay(graphs[-1])
        assert same(one.read(), want)
        two = make()
        graphs.append(two.graph(32))
        two.replay(graphs[-1], times=2)
        assert same(two.read(), want)
        two.replay(graphs[-1])                      # a third replay goes on from step 64, as 32 eager steps do
        eager.steps(32)
        assert same(two.read(), eager.read()) and eager.read()[2] == 96
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
    zeros = make(e0=np.zeros(S.ne))
    zeros.steps(64)
    assert same(zeros.read(), want)
    filled = make(ea=np.full(S.ne, EA))
    filled.steps(64)
    assert same(filled.read(), want)
    other = make(e0=np.full(S.ne, 1e-3))
    other.steps(64)
    assert not same(other.read(), want)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the step's internal force against pf_gl_state_e0 + pf_gl_fint
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["truss_257", "chain_257"])
def test_internal_force_against_the_existing_kernels(systems, name):
    """One step with v = 0, no load, alpha = 0, dt = 1 and minv = 1: c1 = 1 and g = 1 = m, so v' = 0 + 1 ((0 - f_int) 1) is
    -f_int of the step's gather to the bit.  It equals pf_gl_fint after pf_gl_state_e0 to the bound of two device sums:
    (2 degree + 24) 2^-53 scale (step_bounds)."""
    S = systems(name)
    rng = np.random.default_rng(S.ne + 47)
    u, e0 = gl_field(S, "large", rng), rng.uniform(-1e-2, 1e-2, S.ne)
    T = restatement(S, EA, e0)
    T.loads = np.zeros(S.n)
    run = DynRun(S, T, u, np.zeros(S.n), 1.0, e0=e0, minv=np.ones(S.n))
    run.steps(1)
    f_step = -run.read()[1]
    S.state(u, e0)
    f_old = S.fint()
    bound = (2 * T.degree + 24) * U53 * T.f_int_scale(u)
    err = np.abs(f_step - f_old)
    print(f"{name}: step's f_int against pf_gl_fint, worst error / bound {np.max(err[S.free] / bound[S.free]):.3f}, max |f_int| "
          f"{np.max(np.abs(f_old)):.3e}")
    assert np.max(np.abs(f_old[S.free])) > 1.0 and np.all(err[S.free] <= bound[S.free]) and not f_step[S.mask].any()


# ---------------------------------------------------------------------------------------------------------------------
# 6. the energy kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["truss_257", "chain_257"])
def test_energy_against_the_restatement(systems, name):
    """pf_gl_dyn_energy at the state the clock points to (an odd clock: u1).  A sum of K terms in any order is off by at most
    (K - 1) 2^-53 sum |terms| per side; the terms themselves: kinetic m v^2 / 2 with m = 1 / minv 5 roundings per side, f u one,
    the strain energy E A l0 (e - e0)^2 / 2 six on the term and twice the relative error of e - e0, (8 e_abs + 2 (|e| + |e0|))
    2^-53 / |e - e0|.  max |v| is exact.  A second call repeats the bits."""
    S = systems(name)
    rng = np.random.default_rng(S.ne + 53)
    u, v, e0 = gl_field(S, "large", rng), np.where(S.free, rng.standard_normal(S.n), 0.0), rng.uniform(-1e-2, 1e-2, S.ne)
    T = restatement(S, EA, e0)
    run = DynRun(S, T, u, v, 1e-3, e0=e0, clock=3)
    got = run.energy().copy()
    want = T.energies(u, v)
    e, _, du = T.strain(u)
    e_abs = (2.0 * np.sum(np.abs(T.d0) * np.abs(du), axis=1) + np.sum(du * du, axis=1)) / (2.0 * T.l02)
    terms = 0.5 * T.ea * T.l0 * (e - T.e0) ** 2
    b_strain = (2 * S.ne + 12) * U53 * np.sum(terms) + np.sum(T.ea * T.l0 * np.abs(e - T.e0) * (8 * e_abs + 2 * (np.abs(e) + np.abs(T.e0)))) * U53
    bounds = ((2 * S.n + 10) * U53 * want[0], b_strain, (2 * S.n + 2) * U53 * float(np.sum(np.abs(T.loads * u))), 0.0)
    for what, g, w, b in zip(("kinetic", "strain", "f.u", "max |v|"), got, want, bounds):
        print(f"{name} {what}: {g:.15e}, restatement {w:.15e}, error / bound {abs(g - w) / max(b, 1e-300):.3f}")
        assert np.isfinite(g) and abs(g - w) <= b
    assert got[0] > 0.0 and got[1] > 0.0
    assert run.energy().tobytes() == got.tobytes()
    assert run.read()[2] == 3


# ---------------------------------------------------------------------------------------------------------------------
# 7. argument errors
# ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors_touch_nothing(systems):
    """Every refusal is PF_ERR_ARG with a message that begins with the function's name, comes before anything is enqueued and
    leaves the clock and the buffers as they were."""
    S = systems("chain_257")
    T = restatement(S)
    rng = np.random.default_rng(59)
    run = DynRun(S, T, rng.standard_normal(S.n), rng.standard_normal(S.n), 1e-3, 0.5, 0.0, 1.0, 0.25)
    before = run.everything()
    graph = C.c_void_p()
    entry = {"pf_gl_dyn_start": (), "pf_gl_dyn_steps": (1,), "pf_gl_dyn_energy": (run.out.data_ptr(),)}

    def refused(name, rec=None, problem=None, args=None, gl_rec=None):
        eng = S.eng
        rec = run.rec if rec is None else rec
        problem = eng._ref() if problem is None else problem
        gl_rec = C.byref(S.rec) if gl_rec is None else gl_rec
        with eng.on_stream():
            if name == "pf_gl_dyn_graph_create":
                rc = eng.lib.pf_gl_dyn_graph_create(problem, gl_rec, C.byref(rec), 1 if args is None else args[0], eng._stream(),
                                                    C.byref(graph))
            else:
                rc = getattr(eng.lib, name)(problem, gl_rec, C.byref(rec), *(entry[name] if args is None else args), eng._stream())
        assert rc == S.capi.PF_ERR_ARG, (name, rc)
        assert S.lib.pf_last_error().decode().startswith(name + ": "), S.lib.pf_last_error()
        assert not graph

    def changed(**fields):
        rec = S.capi.PfDyn()
        C.memmove(C.byref(rec), C.byref(run.rec), C.sizeof(rec))
        for key, value in fields.items():
            setattr(rec, key, value)
        return rec

    names = list(entry) + ["pf_gl_dyn_graph_create"]
    for name in names:
        for pointer in ("minv", "f_ext", "u0", "u1", "v", "clock"):
            refused(name, changed(**{pointer: None}))
        for bad in (dict(dt=0.0), dict(dt=-1e-3), dict(dt=float("nan")), dict(dt=float("inf")), dict(alpha=-1.0),
                    dict(t_ramp=-1.0)):
            refused(name, changed(**bad))
        bad_mesh = S.capi.PfProblem()
        C.memmove(C.byref(bad_mesh), C.byref(S.eng.P), C.sizeof(bad_mesh))
        bad_mesh.mesh.n_dofs += 1
        refused(name, problem=C.byref(bad_mesh))
        no_d0 = S.capi.PfGl()
        refused(name, gl_rec=C.byref(no_d0))
    for name in ("pf_gl_dyn_steps", "pf_gl_dyn_graph_create"):
        for n in (0, -3):
            refused(name, args=(n,))
    refused("pf_gl_dyn_energy", args=(None,))
    assert run.everything() == before
    # the record itself is good: one step goes through
    run.steps(1)
    assert run.read()[2] == 1 and run.everything() != before


# ---------------------------------------------------------------------------------------------------------------------
# 8. solve_dynamic and the CLI
# ---------------------------------------------------------------------------------------------------------------------
def test_cli_taut_string_vibration(tmp_path):
    """One discrete period of mode 1 of the 8-element string from rest (567 steps of dt = 2 sin(pi / 567) / omega_1): the
    string returns to within 1e-5 a, a = 1e-5 (the restatement: 3.2e-6 a).  solve_dynamic gives the CLI's numbers."""
    from pinn_fem_amd.fem.dynamics import solve_dynamic
    out, parsed = run_cli(tmp_path, "taut_string_vibration", parse=True)
    a, u0 = 1e-5, gd.string_mode(1, 8, 1e-5)
    d = out["dynamics"]
    miss = np.max(np.abs(np.array(out["displacements"]) - u0)) / a
    print(f"string: {d['steps']} steps, miss {miss:.3e} a, mid-span record {[r[0] for r in d['recorded_displacements']]}")
    assert d["steps"] == 567 and d["times"] == [k * d["dt"] for k in (0, 189, 378, 567)] and not d["at_rest"]
    assert miss <= 1e-5
    mid = np.array([r[0] for r in d["recorded_displacements"]])
    assert mid[0] == a and abs(mid[1] - a * np.cos(2 * np.pi / 3)) <= 1e-5 * a and abs(mid[3] - a) <= 1e-5 * a
    assert len(d["energies"]) == 4 and len(out["axial_forces"]) == 8
    assert np.allclose(out["axial_forces"], 1.0, rtol=1e-6)                   # the pretension: T = -E A e0 = 1
    res = solve_dynamic(parsed["model"], parsed["solver_config"], parsed["dynamics"]["config"],
                        u_initial=parsed["dynamics"]["u_initial"])
    assert np.array_equal(res.displacements.reshape(-1), np.array(out["displacements"])) and res.steps == 567


def test_cli_two_bar_snaps_through(tmp_path):
    """A step load of 1.5 times the limit load, which solve_nr refuses under load control: the damped run comes to rest on the
    far root of P(w) = load to 1e-10 of h, with a residual below 1e-10 of the load."""
    from pinn_fem_amd.fem.solver import solve_nr
    out, parsed = run_cli(tmp_path, "two_bar_snap_dynamic", parse=True)
    tb = gl.TwoBar(a=1.0, h=0.1, ea=EA)
    load = 1.5 * tb.p_lim
    far, d = gd.two_bar_far_root(tb, load), out["dynamics"]
    w = -out["displacements"][5]
    print(f"two-bar: {d['steps']} steps, w {w:.15f}, far root {far:.15f}, miss {abs(w - far) / tb.h:.2e} h, residual "
          f"{d['residual_norm']:.2e}")
    assert far > 2.0 * tb.h and abs(w - far) <= 1e-10 * tb.h
    assert d["at_rest"] and out["converged"] and d["steps"] < 20000 and d["residual_norm"] <= 1e-10 * load
    assert np.allclose(np.array(out["reactions"])[[1, 3]].sum(), load, rtol=1e-9)
    with pytest.raises(RuntimeError, match="not positive definite|singular"):
        solve_nr(parsed["model"], parsed["solver_config"], 1.0)


def test_a_step_above_the_bound_is_refused(systems):
    from pinn_fem_amd.fem.dynamics import DynamicsConfig, solve_dynamic, stable_time_step
    from pinn_fem_amd.fem.solver import SolverConfig
    S = systems("truss_257")
    config = SolverConfig(method="nr", kinematics="green-lagrange")
    limit = stable_time_step(S.model, config, safety=1.0)
    T = gd.Truss(S.nodes, S.el, S.fixed, 2, EA, None, gd.lumped_mass(S.nodes, S.el, AREA_DENSITY, 2))
    assert limit == pytest.approx(2.0 / T.omega_bound(np.zeros(S.n)), rel=1e-12)
    with pytest.raises(RuntimeError, match=r"above the stability limit .* at t = 0 \(step 0\)"):
        solve_dynamic(S.model, config, DynamicsConfig(dt=1.01 * limit, n_steps=10))
    res = solve_dynamic(S.model, config, DynamicsConfig(dt=0.9 * limit, n_steps=10, record_every=4))
    assert res.steps == 10 and list(res.times) == [k * res.dt for k in (0, 4, 8, 10)] and not res.displacements.any()

