"""Elastoplastic bars in the Green-Lagrange Newton solve on the device: pf_gl_state_plastic through the C ABI against the bar
entry points (bit for bit wherever nothing yields) and against the restatement tests/gl_plastic_reference.py (itself pinned
by tests/test_gl_plastic_host.py) on seeded yielding fields that keep the margin condition, the engine's committed / trial
state, then solve_nr, solve() with load_factors and the CLI against the restatement's load programs.

The round-off bounds of the yielding fields extend test_gl_f64.py's (_state_bounds there) by the return map's operations;
they are derived at _plastic_bounds.  The solves' bound is test_gl_cable_static_f64.py's: ten times the distance at which the
restatement with scipy's Jacobi-CG (same rtol) ends from the restatement with the direct solve, with the floor 1e-12 of
max |u| between two Newton solutions of one structure.  The measured figures are printed in front of every assertion.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import gl_plastic_reference as gp
import gl_reference as gl
from device_driver import EA, RTOL, U53, GlTruss, gl_config, gl_field, gl_system, run_cli, system_cache, truss_model
from gl_plastic_driver import FIELD_SEEDS, KAPPAS, PlasticState, field_case, wrap_case

pytestmark = pytest.mark.gpu

EY = gp.EY
SIZES = (1, 255, 256, 257, 1000)
MESHES = [f"{kind}_{n}" for kind in ("truss", "chain") for n in SIZES]
SAME_SOLUTION = 1e-12


@pytest.fixture(scope="module")
def systems():
    yield from system_cache(gl_system)


def _bytes(*arrays):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)


# ---------------------------------------------------------------------------------------------------------------------
# 1. nothing yields: the bar's bits
# ---------------------------------------------------------------------------------------------------------------------
def _never_yields(S, PS, rng, label):
    u = gl_field(S, "large", rng)
    ea_given, e0 = EA * rng.uniform(0.5, 2.0, S.ne), rng.uniform(-0.05, 0.05, S.ne)
    kappa = rng.uniform(0.0, 0.5, S.ne)
    for what, zz, ee in (("pf_gl_state", None, None), ("pf_gl_state_ea", None, ea_given), ("pf_gl_state_e0", e0, None),
                         ("pf_gl_state_e0 with ea", e0, ea_given)):
        bar = S.state(u, zz, ee)
        PS.clear()
        strain, fe, kt, ep, al, flags, counts = PS.state(u, np.inf, kappa, 0.0, 0.0, zz, ee)
        assert _bytes(strain, fe, kt) == _bytes(*bar), f"{label}, {what}"
        assert _bytes(ep, al) == bytes(16 * S.ne) and not flags.any() and counts == (0.0, 0.0), f"{label}, {what}"


@pytest.mark.parametrize("name", MESHES)
def test_never_yields_is_the_bar_to_the_bit(systems, name):
    """ey = inf, a zero state: strain, fe and kt of pf_gl_state / _ea / _e0 to the bit; ep and alpha out are zero bytes, no
    flag, counts (0, 0).  1-D and 2-D on both sides of the block."""
    S = systems(name)
    _never_yields(S, PlasticState(S), np.random.default_rng(6000 + S.ne), name)


def test_never_yields_across_the_grid_stride_wrap():
    """PF_MAX_NODE_BLOCKS * 256 + 37 elements: the first 37 threads take a second element."""
    from pinn_fem_amd import _capi
    x, el, fixed, u = wrap_case()
    ne = len(el)
    S = GlTruss(x, el, fixed, 1)
    PS = PlasticState(S)
    assert PS.blocks == _capi.PF_MAX_NODE_BLOCKS and ne == PS.blocks * 256 + 37
    _never_yields(S, PS, np.random.default_rng(ne + 2), f"{ne} elements")
    # and a yielding state over the wrap: flags, both counts and the block partials against the host rule on the same field
    # (tests/test_gl_plastic_host.py asserts the margin condition for it)
    margin = gp.yield_margin(S.nodes, S.el, u, 1, EY, 0.05)
    want = gp.element_state_plastic(S.nodes, S.el, u, EA, 1, EY, 0.05)[5]
    PS.clear()
    flags, counts = PS.state(u, EY, 0.05)[5:]
    part = PS.counts.cpu().numpy()[2: 2 + 2 * PS.blocks].reshape(-1, 2)
    blocks = np.zeros(PS.blocks)
    np.add.at(blocks, (np.arange(ne) // 256) % PS.blocks, want.astype(float))
    print(f"{ne} elements: margin {margin:.2e} ey, {int(want.sum())} plastic, counts {counts}, plastic in the wrap {int(want[-37:].sum())}")
    assert margin >= gp.MARGIN and want[-37:].any() and not want[-37:].all()
    assert np.array_equal(flags, want) and counts == (float(want.sum()), float(want.sum()))
    assert np.array_equal(part[:, 0], blocks) and np.array_equal(part[:, 1], blocks)
    del S, PS
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------------
# 2. a committed state, nothing yielding
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["truss_257", "chain_1000"])
def test_committed_state_without_yielding_is_the_e0_kernel_at_ep(systems, name):
    """tr = e - ep_n is the subtraction pf_gl_state_e0 does with e0 := ep_n, so with e0 null the record is that kernel's to
    the bit; ep and alpha out are the bytes of the inputs.  The yield strain is far above every |tr| (10 against 0.4)."""
    S = systems(name)
    PS = PlasticState(S)
    rng = np.random.default_rng(6100 + S.ne)
    u = gl_field(S, "large", rng)
    ep_n = rng.uniform(-0.05, 0.05, S.ne)
    al_n = np.abs(ep_n) + rng.uniform(0.0, 0.01, S.ne)
    for ee in (None, EA * rng.uniform(0.5, 2.0, S.ne)):
        bar = S.state(u, ep_n, ee)
        PS.clear()
        strain, fe, kt, ep, al, flags, counts = PS.state(u, 10.0, rng.uniform(0.0, 0.5, S.ne), ep_n, al_n, None, ee)
        assert _bytes(strain, fe, kt) == _bytes(*bar)
        assert _bytes(ep, al) == _bytes(ep_n, al_n) and not flags.any() and counts == (0.0, 0.0)


# ---------------------------------------------------------------------------------------------------------------------
# 3. yielding fields
# ---------------------------------------------------------------------------------------------------------------------
def _plastic_bounds(nodes, el, dim, u, kappa, ep_n, al_n, e0, ea):
    """Reference values and round-off bounds of strain, ep, alpha, fe and kt per element, in units of 2^-53, for device and
    restatement together.  test_gl_f64.py's _state_bounds gives b_e = 8 e_abs for the strain, 14 relative for N / l0 behind
    the strain that carries stress and 25 for the material term of B.  The return map adds, one rounding per operation and
    side (both sides round every operation on its own, and r = ey + kappa alpha_n and 1 + kappa have the same inputs on
    both, so they are the same bits and carry nothing):
      se = e - e0:        b_se = b_e + 2 |se|        (nothing without an e0)
      tr = se - ep_n:     b_tr = b_se + 2 |tr|
      f  = |tr| - r:      b_f  = b_tr + 2 |f|
      dg = f / (1 + k):   b_dg = b_f / (1 + k) + 2 |dg|
      ep = ep_n +- dg:    b_ep = b_dg + 2 |ep|;      alpha = alpha_n + dg:  b_al = b_dg + 2 |alpha|
      s  = tr -+ dg:      b_s  = b_tr + b_dg + 2 |s|
    and where the element is not plastic ep and alpha are the inputs' bytes and s = tr, b_s = b_tr.  N / l0 = E A s / l0
    then carries (b_s + 14 |s|) E A / l0, and E A_t = E A kappa / (1 + kappa) two more roundings per side: 29 for the
    material term of B where the element is plastic.  The margin condition makes the branch the same on both sides."""
    strain, fe, B, ep, al, plastic, t = gp.element_state_plastic(nodes, el, u, EA if ea is None else ea, dim, EY, kappa, ep_n, al_n, e0)
    b_e = 8 * U53 * t["e_abs"]
    b_se = b_e + (2 * U53 * np.abs(strain - t["e0"]) if e0 is not None else 0.0)
    b_tr = b_se + 2 * U53 * np.abs(t["tr"])
    b_f = b_tr + 2 * U53 * np.abs(t["f"])
    dg = np.where(plastic, t["f"] / (1.0 + t["kappa"]), 0.0)
    b_dg = b_f / (1.0 + t["kappa"]) + 2 * U53 * np.abs(dg)
    b_ep = np.where(plastic, b_dg + 2 * U53 * np.abs(ep), 0.0)
    b_al = np.where(plastic, b_dg + 2 * U53 * np.abs(al), 0.0)
    b_s = np.where(plastic, b_tr + b_dg + 2 * U53 * np.abs(t["s"]), b_tr)
    n_l0 = (b_s + 14 * U53 * np.abs(t["s"])) * t["ea"] / t["l0"]
    b_fe = n_l0[:, None] * np.abs(t["d"])
    k = t["ea_t"] / (t["l02"] * t["l0"])
    dd = np.abs(t["d"][:, :, None] * t["d"][:, None, :])
    b_B = (np.where(plastic, 29, 25) * U53 * k)[:, None, None] * dd + n_l0[:, None, None] * np.eye(dim)
    pick = (lambda M: np.stack([M[:, 0, 0], M[:, 0, 1], M[:, 1, 1]], axis=1)) if dim == 2 else (lambda M: M[:, 0, 0][:, None])
    return plastic, {"strain": (strain, b_e), "ep": (ep, b_ep), "alpha": (al, b_al), "fe": (fe, b_fe), "kt": (pick(B), pick(b_B))}


WORST = {}                     # what -> the worst error / bound over the yielding-field cases (printed by the last of them)


@pytest.mark.parametrize("with_e0_ea", [False, True])
@pytest.mark.parametrize("kappa_name", KAPPAS)
@pytest.mark.parametrize("name", sorted(FIELD_SEEDS))
def test_yielding_fields_against_the_restatement(systems, name, kappa_name, with_e0_ea):
    """|du| / l0 up to 5e-3 against ey = 1e-3, a non-zero committed state; the seeds keep the margin condition
    (tests/test_gl_plastic_host.py asserts it), so flags and both counts are the restatement's exactly and every element is
    compared.  A second call at another field counts the changed flags."""
    S = systems(name)
    PS = PlasticState(S)
    nodes, el, fixed, dim, u, other, kappa, ep_n, al_n, e0, ea = field_case(name, kappa_name, with_e0_ea)
    assert np.array_equal(nodes, S.nodes.reshape(np.shape(nodes))) and np.array_equal(el, S.el)
    plastic, want = _plastic_bounds(nodes, el, dim, u, kappa, ep_n, al_n, e0, ea)
    PS.clear()
    strain, fe, kt, ep, al, flags, counts = PS.state(u, EY, kappa, ep_n, al_n, e0, ea)
    label = f"{name}, kappa {kappa_name}, e0/ea {with_e0_ea}"
    print(f"{label}: {int(plastic.sum())} of {S.ne} plastic, counts {counts}")
    assert np.array_equal(flags, plastic) and counts == (float(plastic.sum()), float(plastic.sum()))
    for what, got in (("strain", strain), ("ep", ep), ("alpha", al), ("fe", fe), ("kt", kt)):
        ref, bound = want[what]
        got = got.reshape(ref.shape)
        err = np.abs(got - ref)
        ratio = float(np.max(np.where(err > 0.0, err / np.maximum(bound, 1e-300), 0.0)))
        WORST[what] = max(WORST.get(what, 0.0), ratio)
        print(f"{label} {what}: worst error / bound {ratio:.3f}, relative {np.max(err) / max(np.max(np.abs(ref)), 1e-300):.2e}")
        assert np.all(np.isfinite(got)) and np.all(err <= bound), what
    # where the element is not plastic, ep and alpha are the inputs' bytes
    assert _bytes(ep[~plastic], al[~plastic]) == _bytes(ep_n[~plastic], al_n[~plastic])
    # a second call at another field: n_changed against the flags the first call left
    plastic_other = gp.element_state_plastic(nodes, el, other, EA if ea is None else ea, dim, EY, kappa, ep_n, al_n, e0)[5]
    flags_other, counts_other = PS.state(other, EY, kappa, ep_n, al_n, e0, ea)[5:]
    changed = float((plastic_other != plastic).sum())
    print(f"{label}: second field {int(plastic_other.sum())} plastic, changed {counts_other[1]:.0f} (host {changed:.0f})")
    assert np.array_equal(flags_other, plastic_other) and counts_other == (float(plastic_other.sum()), changed) and changed > 0
    print("worst error / bound so far: " + ", ".join(f"{k} {v:.3f}" for k, v in WORST.items()))


# ---------------------------------------------------------------------------------------------------------------------
# 4. repeats and input safety
# ---------------------------------------------------------------------------------------------------------------------
def test_repeats_are_the_same_bytes_and_inputs_are_not_written(systems):
    S = systems("truss_257")
    PS = PlasticState(S)
    nodes, el, fixed, dim, u, other, kappa, ep_n, al_n, e0, ea = field_case("truss_257", "per-element", True)
    PS.clear()
    PS.state(u, EY, kappa, ep_n, al_n, e0, ea)
    first, inputs = PS.everything(), PS.inputs()
    want_inputs = _bytes(np.full(S.ne, EY), kappa, ep_n, al_n)
    assert inputs == want_inputs
    PS.clear()
    PS.state(u, EY, kappa, ep_n, al_n, e0, ea)
    assert PS.everything() == first and PS.inputs() == want_inputs
    # the partials behind the counts are exact integers that add up, and what lies behind them is not written
    counts = PS.counts.cpu().numpy()
    part = counts[2: 2 + 2 * PS.blocks].reshape(-1, 2)
    assert np.all(part == np.floor(part)) and part[:, 0].sum() == counts[0] and part[:, 1].sum() == counts[1]
    assert np.all(counts[2 + 2 * PS.blocks:] == 7.0)


def test_argument_errors_touch_nothing(systems):
    S = systems("truss_257")
    PS = PlasticState(S)
    nodes, el, fixed, dim, u, other, kappa, ep_n, al_n, e0, ea = field_case("truss_257", "0.05", False)
    PS.state(u, EY, kappa, ep_n, al_n)
    for t in (PS.ep, PS.al, PS.counts):
        t.fill_(7.0)
    S.refill()
    before = PS.everything()
    eng = S.eng
    uu = S.dev(np.ones(S.n))

    def refused(text, problem=None, rec=None, pl=None, u_ptr=uu.data_ptr(), null_record=False):
        pl = PS.record() if pl is None else pl
        with eng.on_stream():
            rc = S.lib.pf_gl_state_plastic(eng._ref() if problem is None else problem, C.byref(S.rec if rec is None else rec), None,
                                           None, None if null_record else C.byref(pl), u_ptr, eng._stream())
        torch.cuda.synchronize()
        assert rc == S.capi.PF_ERR_ARG and S.lib.pf_last_error().decode().startswith("pf_gl_state_plastic: " + text)

    refused("null plastic record or a null pointer in it", null_record=True)
    for name in ("ey", "kappa", "ep_n", "al_n", "ep", "al", "yielding", "counts"):
        refused("null plastic record or a null pointer in it", pl=PS.record(**{name: None}))
    refused("ep == ep_n or al == al_n", pl=PS.record(ep=PS.ep_n))
    refused("ep == ep_n or al == al_n", pl=PS.record(al=PS.al_n))
    refused("bad argument", u_ptr=None)
    refused("bad argument", rec=S.capi.PfGl())
    bad_mesh = S.capi.PfProblem.from_buffer_copy(eng.P)
    bad_mesh.mesh.dim = 3
    refused("bad argument", problem=C.byref(bad_mesh))
    assert PS.everything() == before
    # no elements: PF_OK and zero counts
    empty = S.capi.PfProblem.from_buffer_copy(eng.P)
    empty.mesh.n_elems = 0
    pl = PS.record()
    with eng.on_stream():
        assert S.lib.pf_gl_state_plastic(C.byref(empty), C.byref(S.rec), None, None, C.byref(pl), uu.data_ptr(), eng._stream()) == S.capi.PF_OK
    torch.cuda.synchronize()
    counts = PS.counts.cpu().numpy()
    assert counts[0] == 0.0 and counts[1] == 0.0 and np.all(counts[2:] == 7.0)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the readers of the record
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["truss_257", "chain_257"])
def test_fint_kt_diag_and_kt_v_read_the_plastic_record(systems, name):
    """pf_gl_fint against the restatement with test_gl_f64.py's bound, (degree + 4) 2^-53 of the sum of the terms' magnitudes
    in front of any cancellation; those are E A (e_abs + |e0| + |ep_n| + |dg|) |d_c| / l0 here, every part of N counted
    with its magnitude.  pf_kt_diag_f64 is the sequential sum of the device's own record to the bit
    (test_gl_cable_static_f64.py's statement), and pf_kt_v_f64 against the CSR product of the restatement's blocks within
    test_gl_f64.py's (16 + 2 degree) 2^-53 |K_t||v|."""
    S = systems(name)
    PS = PlasticState(S)
    nodes, el, fixed, dim, u, other, kappa, ep_n, al_n, e0, ea = field_case(name, "per-element", True)
    PS.clear()
    _, fe, kt, _, _, flags, _ = PS.state(u, EY, kappa, ep_n, al_n, e0, ea)
    st = gp.element_state_plastic(nodes, el, u, ea, dim, EY, kappa, ep_n, al_n, e0)
    t = st[6]
    assert np.array_equal(flags, st[5]) and flags.any()
    n_nodes = len(gl._as2d(nodes, dim))
    want_f = gl._scatter(n_nodes, dim, el, st[1], -1.0)
    dg = np.where(st[5], t["f"] / (1.0 + t["kappa"]), 0.0)
    mag = (t["ea"] * (t["e_abs"] + np.abs(t["e0"]) + np.abs(ep_n) + np.abs(dg)) / t["l0"])[:, None] * np.abs(t["d"])
    bound = (S.degree + 4) * U53 * gl._scatter(n_nodes, dim, el, mag, 1.0)
    fint = S.fint()
    err = np.abs(fint - want_f)
    print(f"{name}: f_int worst error / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert np.all(np.isfinite(fint)) and np.all(err <= bound)
    # the diagonal: the device's own record, summed in ascending incidence order
    plan = S.eng.plan
    adj_ptr, adj = np.asarray(plan.adj_ptr), np.asarray(plan.adj)
    want_d = np.zeros(S.n)
    for node in range(S.n_nodes):
        for c in range(S.dim):
            acc = 0.0
            for code in adj[adj_ptr[node]:adj_ptr[node + 1]]:
                acc = acc + float(kt[code >> 1, 2 * c if S.dim == 2 else 0])
            want_d[node * S.dim + c] = acc
    want_d[S.mask] = 0.0
    assert S.kt_diag().tobytes() == want_d.tobytes()
    # K_t v
    K, Kabs = gl.blocks_csr(st[2], el, n_nodes, dim), gl.blocks_csr(st[2], el, n_nodes, dim, absolute=True)
    v = np.random.default_rng(S.ne + 5).standard_normal(S.n)
    scale = Kabs @ np.abs(v)
    max_deg = int(S.degree.max())
    err = np.abs(S.kt_v(v) - K @ v)
    print(f"{name}: K_t v worst error {np.max(err / np.maximum(scale, 1e-300)) / U53:.2f} * 2^-53 |K_t||v| (bound {16 + 2 * max_deg})")
    assert np.all(err <= (16 + 2 * max_deg) * U53 * scale)


# ---------------------------------------------------------------------------------------------------------------------
# 6. the engine's committed and trial state
# ---------------------------------------------------------------------------------------------------------------------
def test_engine_commit_reset_and_counts(systems):
    S = systems("truss_257")
    eng = S.eng
    nodes, el, fixed, dim, u, other, kappa, ep_n, al_n, e0, ea = field_case("truss_257", "0.05", False)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)
    ey = np.full(S.ne, EY)
    eng.gl_plastic_reset()
    with pytest.raises(RuntimeError, match="gl_plastic_commit: no plastic state formed"):
        eng.gl_plastic_commit()
    with pytest.raises(RuntimeError, match="gl_plastic_counts: no plastic state formed"):
        eng.gl_plastic_counts()
    # from the zero state
    first = gp.element_state_plastic(nodes, el, u, EA, dim, EY, kappa)
    strain = eng.gl_state_plastic(dev(u), dev(ey), dev(kappa))
    ep, al, flags = eng.gl_plastic_state()
    assert np.array_equal(flags, first[5]) and eng.gl_plastic_counts() == (int(first[5].sum()), int(first[5].sum()))
    assert strain.shape == (S.ne,) and np.allclose(ep, first[3], rtol=0.0, atol=1e-15) and first[5].any()
    # a second evaluation before the commit starts from the committed (zero) state again, not from the trial one
    eng.gl_state_plastic(dev(u), dev(ey), dev(kappa))
    ep_again, al_again, _ = eng.gl_plastic_state()
    assert _bytes(ep_again, al_again) == _bytes(ep, al) and eng.gl_plastic_counts() == (int(first[5].sum()), 0)
    # commit: the trial state is the committed one; at the same u nothing yields any more (it sits on the surface, under
    # the threshold), and the state handed back is the committed one's bytes
    eng.gl_plastic_commit()
    with pytest.raises(RuntimeError, match="no plastic state formed"):
        eng.gl_plastic_commit()
    eng.gl_state_plastic(dev(u), dev(ey), dev(kappa))
    ep2, al2, flags2 = eng.gl_plastic_state()
    print(f"engine: {int(first[5].sum())} plastic from the zero state, {int(flags2.sum())} at the same u after the commit")
    assert not flags2.any() and _bytes(ep2, al2) == _bytes(ep, al)
    assert eng.gl_plastic_counts() == (0, int(first[5].sum()))
    # reset with a given state, and to zeros
    eng.gl_plastic_reset(ep_n, al_n)
    given = gp.element_state_plastic(nodes, el, other, EA, dim, EY, kappa, ep_n, al_n)
    eng.gl_state_plastic(dev(other), dev(ey), dev(kappa))
    assert np.array_equal(eng.gl_plastic_state()[2], given[5]) and eng.gl_plastic_counts() == (int(given[5].sum()), int(given[5].sum()))
    eng.gl_plastic_reset()
    eng.gl_state_plastic(dev(u), dev(ey), dev(kappa))
    assert _bytes(*eng.gl_plastic_state()[:2]) == _bytes(ep, al)
    with pytest.raises(ValueError, match="gl_state_plastic: kappa has 3 entries"):
        eng.gl_state_plastic(dev(u), dev(ey), dev(kappa[:3]))


# ---------------------------------------------------------------------------------------------------------------------
# 7. - 11. the solves
# ---------------------------------------------------------------------------------------------------------------------
def _cases():
    T = gp.ThreeBar()
    nodes, el, loads, fixed, tip = gp.warren_first_yield()
    e0 = np.random.default_rng(5).uniform(-2e-4, 2e-4, len(el))
    return {"three-bar": (T.nodes, T.el, T.loads, T.fixed, 0.0, gp.THREE_BAR_PROGRAM, None),
            "warren": (nodes, el, loads, fixed, gp.WARREN_KAPPA, gp.WARREN_PROGRAM, None),
            "warren with e0": (nodes, el, loads, fixed, gp.WARREN_KAPPA, gp.WARREN_PROGRAM, e0)}


@pytest.fixture(scope="module")
def programs():
    """case -> (the case, the restatement's load program with the direct solve, the same with scipy's Jacobi-CG): computed
    once, shared, unchanged."""
    out = {}
    for name, case in _cases().items():
        nodes, el, loads, fixed, kappa, program, e0 = case
        direct = gp.load_program(nodes, el, loads, fixed, EA, 2, EY, kappa, program, e0=e0)
        cg = gp.load_program(nodes, el, loads, fixed, EA, 2, EY, kappa, program, e0=e0, linear_solve=gl.jacobi_cg(RTOL))
        assert all(o["converged"] for o in direct) and all(o["converged"] for o in cg)
        out[name] = (case, direct, cg)
    return out


def _axial_tolerance(bound, scale):
    """N = E A (e - e0 - ep): the strain is off by 2 bound max |u| at most and ep by 4 bound max |u| + 8 * 2^-53
    (_check_increment), and the product and its two subtractions round a few times at strains below 1e-2: 8 * 2^-53 more."""
    return EA * (6.0 * bound * scale + 16 * U53)


def _check_increment(label, res, want, want_cg, want_n=None):
    """One converged device increment against the restatement's: displacements within the bound, the yielding set exactly.
    ep and alpha follow the strain: two nodes off by bound * max |u| each move a strain by 2 bound max |u| / l0 at most, and
    the shortest element here has l0 = 1; the return map passes that on with a factor <= 1 into this increment's ep and
    alpha and carries the increment before's with a factor kappa / (1 + kappa) < 1, so 4 bound max |u| covers the sum (and
    8 * 2^-53 the round-off of the closing evaluation at strains of 1e-3)."""
    u, scale = res.displacements.reshape(-1), np.max(np.abs(want["u"]))
    err_ref = np.max(np.abs(want_cg["u"] - want["u"])) / scale
    bound = max(10.0 * err_ref, SAME_SOLUTION)
    err = np.max(np.abs(u - want["u"])) / scale
    err_ep = max(np.max(np.abs(res.plastic_strain - want["ep"])), np.max(np.abs(res.accumulated_plastic_strain - want["al"])))
    print(f"{label}: {int(res.history[-1]['iterations'])} iterations (restatement {want['iterations']}), "
          f"{int(res.yielding.sum())} yielding, error {err:.2e} (scipy-CG Newton {err_ref:.2e}, bound {bound:.2e}), "
          f"ep / alpha off by {err_ep:.2e}")
    assert res.converged and err <= bound
    assert np.array_equal(res.yielding, want["yielding"]) and res.history[-1]["yielding_elements"] == float(want["yielding"].sum())
    assert err_ep <= 4.0 * bound * scale + 8 * U53
    if want_n is not None:
        err_n = np.max(np.abs(res.axial_forces - want_n))
        print(f"{label}: axial forces off by {err_n:.2e} (tolerance {_axial_tolerance(bound, scale):.2e})")
        assert err_n <= _axial_tolerance(bound, scale)
    return bound


def _axial(nodes, el, kappa, e0, increment):
    """The restatement's N = E A (e - e0 - ep) at an increment's end, from its committed state."""
    return gp.element_state_plastic(nodes, el, increment["u"], EA, 2, EY, kappa, increment["ep"], increment["al"], e0)[6]["n"]


@pytest.mark.parametrize("preconditioner", ["jacobi", "two-level-updated"])
@pytest.mark.parametrize("case", ["three-bar", "warren", "warren with e0"])
def test_load_programs_through_solve_and_solve_nr(programs, case, preconditioner):
    """solve() with load_factors walks the whole program; the chain of solve_nr calls that hands the state on is what it
    does inside, increment by increment, so every increment is compared with the restatement's, and the two ends agree."""
    from pinn_fem_amd.fem.solver import solve, solve_nr
    (nodes, el, loads, fixed, kappa, program, e0), direct, cg = programs[case]
    model = truss_model(nodes, el, loads, fixed)
    config = dict(yield_strain=EY, hardening_ratio=kappa, initial_strain=e0, nr_preconditioner=preconditioner, method="nr")
    u, state, res = None, None, None
    for k, lam in enumerate(program):
        res = solve_nr(model, gl_config(**config), lam, u_initial=u, plastic_state=state)
        _check_increment(f"{case}, {preconditioner}, {lam}", res, direct[k], cg[k], _axial(nodes, el, kappa, e0, direct[k]))
        u, state = torch.from_numpy(res.displacements.reshape(-1).copy()), (res.plastic_strain, res.accumulated_plastic_strain)
    whole = solve(model, gl_config(load_factors=program, **config))
    _check_increment(f"{case}, {preconditioner}, solve()", whole, direct[-1], cg[-1], _axial(nodes, el, kappa, e0, direct[-1]))
    assert _bytes(whole.displacements, whole.plastic_strain, whole.accumulated_plastic_strain) == _bytes(
        res.displacements, res.plastic_strain, res.accumulated_plastic_strain)
    path = whole.load_path
    print(f"{case}, {preconditioner}: load_path {[(p['load_factor'], int(p['iterations']), int(p['yielding_elements'])) for p in path]}")
    assert [p["load_factor"] for p in path] == [float(v) for v in program]
    assert [p["yielding_elements"] for p in path] == [float(o["yielding"].sum()) for o in direct]
    assert [int(p["iterations"]) for p in path] == [o["iterations"] for o in direct]
    if case == "three-bar":
        assert whole.yielding.tolist() == [False, True, False]
    else:
        tip = nodes.size - 1
        assert whole.displacements.reshape(-1)[tip] < -0.1 and not whole.yielding.any()      # a permanent set, unloaded


def test_state_handed_back_equals_the_two_step_solve(programs):
    from pinn_fem_amd.fem.solver import solve, solve_nr
    (nodes, el, loads, fixed, kappa, _, _), _, _ = programs["warren"]
    model = truss_model(nodes, el, loads, fixed)
    config = dict(yield_strain=EY, hardening_ratio=kappa, method="nr")
    one = solve_nr(model, gl_config(**config), 1.6)
    two = solve_nr(model, gl_config(**config), 0.4, u_initial=torch.from_numpy(one.displacements.reshape(-1).copy()),
                   plastic_state=(one.plastic_strain, one.accumulated_plastic_strain))
    both = solve(model, gl_config(load_factors=[1.6, 0.4], **config))
    ref = gp.load_program(nodes, el, loads, fixed, EA, 2, EY, kappa, [1.6, 0.4])
    ref_cg = gp.load_program(nodes, el, loads, fixed, EA, 2, EY, kappa, [1.6, 0.4], linear_solve=gl.jacobi_cg(RTOL))
    scale = np.max(np.abs(ref[-1]["u"]))
    bound = max(10.0 * np.max(np.abs(ref_cg[-1]["u"] - ref[-1]["u"])) / scale, SAME_SOLUTION)
    miss = np.max(np.abs(two.displacements.reshape(-1) - ref[-1]["u"])) / scale
    print(f"1.6 then 0.4: {int(one.yielding.sum())} yielding at 1.6, miss to the restatement {miss:.2e} (bound {bound:.2e})")
    assert one.converged and two.converged and both.converged and one.yielding.sum() == 6 and not two.yielding.any()
    assert _bytes(two.displacements, two.plastic_strain, two.accumulated_plastic_strain) == _bytes(
        both.displacements, both.plastic_strain, both.accumulated_plastic_strain)
    assert _bytes(two.plastic_strain, two.accumulated_plastic_strain) == _bytes(one.plastic_strain, one.accumulated_plastic_strain)
    assert miss <= bound


def test_hybrid_with_plasticity_always_ends_in_the_plastic_newton_phase(programs, monkeypatch):
    """solve_hybrid hands plastic_state to its Newton phase, and a GD phase that reports tight convergence (stubbed here: it
    is the linear elastic answer) is not returned in its place: the result is solve_nr's, from the GD answer as the start."""
    from pinn_fem_amd.fem import solver
    (nodes, el, loads, fixed, kappa, _, _), direct, cg = programs["three-bar"]
    model = truss_model(nodes, el, loads, fixed)
    config = dict(yield_strain=EY, hardening_ratio=kappa, method="hybrid")
    want, want_cg = direct[6], cg[6]                                     # load factor 0.97 from the state of 0.9
    state = (direct[5]["ep"], direct[5]["al"])
    res = solver.solve_hybrid(model, gl_config(**config), target_load_factor=0.97,
                              u_initial=torch.from_numpy(direct[5]["u"].copy()), plastic_state=state)
    _check_increment("hybrid, no GD phase", res, want, want_cg, _axial(nodes, el, kappa, None, want))
    elastic = gl.newton(nodes, el, loads, fixed, EA, 2, lam=0.97)[0]
    gd = solver.SolverResult(displacements=elastic.reshape(-1, 2), reactions=np.zeros((4, 2)), converged=True,
                             history=[{"iteration": 7.0, "residual_norm": 0.0}])
    monkeypatch.setattr(solver, "solve_gd", lambda *a, **k: gd)
    res = solver.solve_hybrid(model, gl_config(preconditioning=True, **config), target_load_factor=0.97, plastic_state=state)
    _check_increment("hybrid, a GD phase that converged tightly", res, want, want_cg, _axial(nodes, el, kappa, None, want))
    assert res.plastic_strain is not None and res.yielding.tolist() == [False, True, False]
    # without yield_strain the early return stands as it was
    assert solver.solve_hybrid(model, gl_config(preconditioning=True, method="hybrid"), target_load_factor=0.97) is gd


def test_without_yield_strain_the_answer_is_the_elastic_one(programs):
    from pinn_fem_amd.fem.solver import solve, solve_nr
    (nodes, el, loads, fixed, _, _, _), direct, _ = programs["three-bar"]
    model = truss_model(nodes, el, loads, fixed)
    res = solve_nr(model, gl_config(), 0.97)
    u_bar, _, ok = gl.newton(nodes, el, loads, fixed, EA, 2, lam=0.97)
    miss = np.max(np.abs(res.displacements.reshape(-1) - u_bar)) / np.max(np.abs(u_bar))
    away = abs(res.displacements.reshape(-1)[7] / direct[6]["u"][7] - 1.0)
    print(f"without yield_strain at 0.97: {miss:.2e} from the elastic restatement, {away:.2f} of the plastic answer away from it")
    assert ok and res.converged and miss <= SAME_SOLUTION and away > 0.2
    assert res.plastic_strain is None and res.accumulated_plastic_strain is None and res.yielding is None and res.load_path is None
    assert "yielding_elements" not in res.history[-1] and res.axial_forces is None
    # load_factors alone: the elastic walk, with its load_path
    walk = solve(model, gl_config(load_factors=[0.5, 0.97, 0.25], method="nr"))
    u_low, _, ok = gl.newton(nodes, el, loads, fixed, EA, 2, lam=0.25)
    assert ok and walk.converged and walk.plastic_strain is None
    assert [(p["load_factor"], p["yielding_elements"]) for p in walk.load_path] == [(0.5, 0.0), (0.97, 0.0), (0.25, 0.0)]
    # elastic: the path does not matter
    assert np.max(np.abs(walk.displacements.reshape(-1) - u_low)) <= SAME_SOLUTION * np.max(np.abs(u_low))


def test_a_plastic_mechanism_is_refused():
    """A 1-D bar without hardening at -1.2 N_y: the second iteration's state has the tangent diagonal -N_y / l0."""
    from pinn_fem_amd.fem.solver import solve_nr
    x, el, fixed = gp.bar_1d(2.0)
    model = truss_model(x, el, np.array([0.0, -1.2 * EA * EY]), fixed, dim=1)
    with pytest.raises(RuntimeError, match=r"Newton iteration 2: its diagonal is -0\.5 at free dof 1, which only yielding elements "
                                           r"hold \(a plastic mechanism, collapse"):
        solve_nr(model, gl_config(yield_strain=EY), 1.0)
    assert solve_nr(model, gl_config(yield_strain=EY, hardening_ratio=0.1), 1.0).converged


def test_cli_on_the_plastic_inputs(tmp_path, programs):
    for input_name, case in (("three_bar_plastic", "three-bar"), ("warren_plastic_cycle", "warren")):
        out = run_cli(tmp_path, input_name)
        (nodes, el, _, _, kappa, _, e0), direct, cg = programs[case]
        want, scale = direct[-1], np.max(np.abs(direct[-1]["u"]))
        bound = max(10.0 * np.max(np.abs(cg[-1]["u"] - want["u"])) / scale, SAME_SOLUTION)
        miss = np.max(np.abs(np.array(out["displacements"]).reshape(-1) - want["u"])) / scale
        print(f"CLI, {input_name}: yielding {out['yielding_elements']}, miss {miss:.2e} (bound {bound:.2e}), "
              f"load_path {[(p['load_factor'], int(p['yielding_elements'])) for p in out['load_path']]}")
        assert out["converged"] and miss <= bound and out["yielding_elements"] == np.flatnonzero(want["yielding"]).tolist()
        assert np.allclose(out["plastic_strain"], want["ep"], rtol=0.0, atol=4.0 * bound * scale + 8 * U53)
        assert np.allclose(out["accumulated_plastic_strain"], want["al"], rtol=0.0, atol=4.0 * bound * scale + 8 * U53)
        assert [p["yielding_elements"] for p in out["load_path"]] == [float(o["yielding"].sum()) for o in direct]
        assert np.max(np.abs(np.array(out["axial_forces"]) - _axial(nodes, el, kappa, e0, want))) <= _axial_tolerance(bound, scale)
        assert out["history"][-1]["yielding_elements"] == float(want["yielding"].sum())
