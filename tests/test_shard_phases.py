"""The sharded iteration, phase by phase, with all W ranks of a partition in ONE process (tests/shard_driver.py) against the
numpy oracle on the whole, unsharded mesh.

The five C entry points behind HipShardBackend (pf_shard_forward / _backward / _update_interior / _update_shared /
_flush, i.e. k_shard_pack, k_shard_update, k_shard_flush and the own_only / skip_shared modes of the node kernels) run
exactly as dist._run_iterations calls them; the all-reduce between them is a float32 sum on the host, so every buffer
of an iteration can be compared before and after it.

Reference: oracle/pinn_oracle.py.  Its per-element arithmetic is float32 in the reference's operation order by
design; every sum over elements / dofs is taken in float64 here (loss_and_grads(acc64=True)), so the oracle's own
summation error is ~2^-53 and a difference measures the kernels.  The single HipEngine is a second comparator.

Tolerances (stated where they are used):
  * what the project already holds a single engine to against this oracle keeps that number: grad_u 5e-5 max|grad_u|,
    grad_theta 5e-4, loss_physics (sum r^2) 1e-4, loss_data (sum d^2) 1e-5 (test_oracle_parity_chain_sizes);
  * what sharding alone adds, and one Adam step, are bounded from 2^-24 and operation counts;
  * identities that must hold bit for bit (copies of a dof, replicas of theta, history and state across ranks, no
    change after the stop) are compared as bytes.
Every measured error / bound ratio is printed in front of its assertion ("shard-ratio ..." lines; a recorded set is
profiles/shard_phase_ratios.txt).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from shard_driver import ShardWorld, mesh_case, orc

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
EPS32 = 2.0 ** -24
LAM, LR_T, ALPHA_P, ALPHA_D = 0.7, 5e-4, 1.0, 100.0
B1, B2, ADAM_EPS = 0.9, 0.999, 1e-8
ORACLE_WG = [3, 1]        # as tests/test_hip_parity.py: the engine the product ships (MFMA32) and one cross-check engine

# key: (mesh, world, wg_mode, fe_mode)
CASES = {
    "A-w3": ("A", 3, 3, 0),
    "A-w3-delta": ("A", 3, 3, 1),             # fe_mode=1 <-> the oracle's cancellation-free "delta" form
    "B-w2": ("B", 2, 3, 0),
    "C-w3": ("C", 3, ORACLE_WG[0], 0),
    "C-w3-delta": ("C", 3, ORACLE_WG[0], 1),
    "C-w5": ("C", 5, 3, 0),
    "C-w3-mfma": ("C", 3, ORACLE_WG[1], 0),   # not MFMA32: theta is read back from global memory (__threadfence_block)
    "C-w3-mfma44": ("C", 3, 2, 0),
    "D-w4": ("D", 4, 3, 0),                   # DIM == 1, scalar E and A: n_theta_active == 0
    "AE-w3": ("A-E", 3, 3, 0),                # E net only
}
LR_U = {"A": 1e-3, "B": 1e-3, "A-E": 1e-3, "C": 1e-4, "D": 1e-3}

_worlds, _cases, _singles = {}, {}, {}


def _ratio(check, key, what, err, bound):
    r = float(err) / float(bound) if bound > 0 else (0.0 if err == 0 else np.inf)
    print(f"shard-ratio check={check} case={key} {what}: err {float(err):.3e} bound {float(bound):.3e} ratio {r:.3f}")
    return r


def _case(key):
    name = CASES[key][0]
    if name not in _cases:
        _cases[name] = mesh_case(name)
    return _cases[name]


def _theta0(case):
    return np.concatenate([t.reshape(-1) for t in case.theta]).astype(f32) if case.theta else np.zeros(0, f32)


def _world(key) -> ShardWorld:
    """The W backends of a case (built once) with the fixture's theta put back: a run trains theta in place."""
    name, world, wg, fe = CASES[key]
    case = _case(key)
    if key not in _worlds:
        _worlds[key] = ShardWorld(case.make_model, case.mv, case.md, world, wg_mode=wg, fe_mode=fe)
    w = _worlds[key]
    th = torch.from_numpy(_theta0(case))
    for be in w.backends:
        if be.eng.n_theta:
            be.eng.theta.flat.copy_(th)
    return w


def _single(key):
    from pinn_fem_amd.engine import HipEngine
    name, _, wg, fe = CASES[key]
    case = _case(key)
    k = (name, wg, fe)
    if k not in _singles:
        _singles[k] = HipEngine(case.make_model(), case.mv, case.md, wg_mode=wg, fe_mode=fe)
    eng = _singles[k]
    if eng.n_theta:
        eng.theta.flat.copy_(torch.from_numpy(_theta0(case)))
    return eng


def _config(key, max_iterations=40, tolerance=0.0):
    from pinn_fem_amd.fem.solver import SolverConfig
    return SolverConfig(max_iterations=max_iterations, tolerance=tolerance, learning_rate_u=LR_U[CASES[key][0]],
                        learning_rate_theta=LR_T, alpha_physics=ALPHA_P, alpha_data=ALPHA_D)


def _oracle_config(key, max_iterations, tolerance=0.0):
    return orc.SolverConfig(max_iterations=max_iterations, tolerance=tolerance, learning_rate_u=LR_U[CASES[key][0]],
                            learning_rate_theta=LR_T, alpha_physics=ALPHA_P, alpha_data=ALPHA_D)


def _u0(key, fixed_start=False):
    """A random start; fixed_start: the fixed dofs start non-zero (0.3 on the interface, 0.2 in the interior)."""
    name, world = CASES[key][0], CASES[key][1]
    case = _case(key)
    rng = np.random.default_rng(7)
    u = (rng.standard_normal(case.n_dofs) * (1e-3 if name == "C" else 1e-2)).astype(f32)
    u[case.fixed] = 0.0
    if fixed_start:
        L = case.layout(world)
        on_iface = np.isin(case.fixed, L.slot_dof)
        u[case.fixed[on_iface]] = 0.3
        u[case.fixed[~on_iface]] = 0.2
    return u


def _fe(key):
    return "delta" if CASES[key][3] else "reference"


def _pb_with_theta(case, flat):
    pb = case.problem()
    off = 0
    for t in pb.theta_list():
        t[...] = np.asarray(flat[off:off + t.size], dtype=f32).reshape(t.shape)
        off += t.size
    return pb


def _oracle_step(case, u, theta_flat, key):
    pb = _pb_with_theta(case, theta_flat)
    ref = orc.loss_and_grads(pb, orc.element_geometry(pb), u, LAM, ALPHA_P, ALPHA_D, fe_mode=_fe(key), acc64=True)
    gt = [g.reshape(-1) for g in ref.grad_theta if g is not None]
    return pb, ref, (np.concatenate(gt).astype(f64) if gt else np.zeros(0))


def _slot_map(w: ShardWorld):
    slot_dof = -np.ones(w.n_iface, dtype=np.int64)
    for be in w.backends:
        slot_dof[be.shard.shared_slot] = be.dofs_global[be.shard.shared_dofs]
    assert np.all(slot_dof >= 0)
    return slot_dof


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def _assert_copies_identical(w, names=("u", "m_u", "v_u")):
    for name in names:
        vals, held = w.copies(name)
        first = np.argmax(held, axis=0)
        ref = _bits(vals)[first, np.arange(w.n_iface)]
        same = (_bits(vals) == ref[None, :]) | ~held
        assert same.all(), f"{name}: {np.count_nonzero(~same)} copies of interface dofs differ between ranks"
    for name in ("theta", "m_t", "v_t"):
        b = [w.theta_bytes(r, name) for r in range(w.world)]
        assert all(x == b[0] for x in b), f"{name} differs between ranks"


# ---------------------------------------------------------------------------------------------------
# check 1: the collective buffer after backward, before any reduction
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(CASES))
def test_backward_fills_the_collective_buffer(key):
    case, w = _case(key), _world(key)
    u0 = _u0(key)
    w.begin(u0, LAM, _config(key))
    w.fill_bufs(7.0)
    w.forward()
    w.backward()
    w.reduce()
    n_if, n_t = w.n_iface, w.n_theta_active
    assert w.n_buf == n_if + n_t + 3
    for r, be in enumerate(w.backends):
        part = w.parts[r]
        assert part.size == w.n_buf and not np.any(part == 7.0), "an entry of buf was not written"
        held = np.zeros(n_if, dtype=bool)
        held[be.shard.shared_slot] = True
        assert np.all(part[:n_if][~held] == 0.0), "a slot of a dof the rank does not hold is not exactly 0"
        assert part[n_if + n_t + 2] == 0.0                     # u2 of the previous iteration: none yet
    pb, ref, ref_t = _oracle_step(case, u0, _theta0(case), key)
    slot_dof = _slot_map(w)
    s = w.sum64
    gmax = np.max(np.abs(ref.grad_u))
    # interface gradient, summed over the ranks: the single engine's number against this oracle
    err = np.max(np.abs(s[:n_if] - ref.grad_u[slot_dof].astype(f64)))
    r_gu = _ratio(1, key, "grad_u on the interface vs oracle", err, 5e-5 * gmax)
    assert r_gu < 1
    if n_t:
        err = np.max(np.abs(s[n_if:n_if + n_t] - ref_t)) / np.max(np.abs(ref_t))
        assert _ratio(1, key, "grad_theta vs oracle", err, 5e-4) < 1
    free = np.ones(case.n_dofs, dtype=bool)
    free[case.fixed] = False
    sum_r2 = float(np.sum(ref.r.astype(f64) ** 2))
    d = (case.mv.astype(f32) - u0[case.md]).astype(f32)
    sum_d2 = float(np.sum(d.astype(f64) ** 2))
    # each free dof's r^2 and each measured dof's d^2 exactly once (no double count on shared nodes, no data term twice)
    assert _ratio(1, key, "sum r^2 vs oracle", abs(s[n_if + n_t] - sum_r2), 1e-4 * sum_r2) < 1
    assert _ratio(1, key, "sum d^2 vs oracle", abs(s[n_if + n_t + 1] - sum_d2), 1e-5 * sum_d2) < 1
    # second comparator, and what sharding alone adds.  Both paths gather one dof's gradient as a float32 sum of the
    # same terms, one per incident element (ke_e^T g_f, the same float32 inputs and code on a rank and on the single
    # engine) and the data term: the single engine in one chain, the ranks in at most W chains over their own
    # elements, which the test then adds exactly.  A chain of n terms is off by at most (n - 1) 2^-24 sum|terms| to
    # first order and the W partial sums carry one rounding each, so the two differ by at most
    #     (incident elements [+ 1 with a data term] + W) 2^-24 sum|terms|,
    # the term magnitudes taken from the oracle's float32 element stiffness and residual.
    eng = _single(key)
    _, gu1, _ = eng.loss_and_grads(torch.from_numpy(u0), LAM, ALPHA_P, ALPHA_D)
    gu1 = gu1.cpu().numpy().astype(f64)
    geo = orc.element_geometry(pb)
    g_f = np.zeros(case.n_dofs, dtype=f64)
    g_f[free] = ALPHA_P * ref.r.astype(f64)
    ke = ref.stiffness.astype(f64)[:, None, None] * geo.pattern.astype(f64)
    mag = np.zeros(case.n_dofs)
    np.add.at(mag, geo.dofs.reshape(-1), np.abs(np.einsum("eab,eb->ea", ke, g_f[geo.dofs])).reshape(-1))
    mag[case.md] += np.abs((ALPHA_D / len(case.mv)) * 2.0 * d.astype(f64))
    n_terms = np.zeros(case.n_dofs)
    np.add.at(n_terms, geo.dofs.reshape(-1), 1.0 / case.dim)      # incident elements of the dof's node
    n_terms[case.md] += 1.0
    bound = (n_terms + w.world) * EPS32 * mag
    dif = np.abs(s[:n_if] - gu1[slot_dof])
    nz = bound[slot_dof] > 0
    assert np.all(dif[~nz] == 0)
    rr = float(np.max(dif[nz] / bound[slot_dof][nz]))
    print(f"shard-ratio check=1 case={key} interface grad_u, sum of shards vs single engine (2^-24 count): ratio {rr:.3f}; "
          f"single engine vs oracle: {np.max(np.abs(gu1 - ref.grad_u)) / (5e-5 * gmax):.3f} of its bound")
    assert rr < 1


# ---------------------------------------------------------------------------------------------------
# check 2: one whole iteration (interior update, reduction, interface update), iterations 1 and 2
# ---------------------------------------------------------------------------------------------------
def _adam_f32(p, m, v, g, lr, t):
    """torch.optim.Adam's single-tensor step as the oracle states it (float32), from a given state."""
    p = np.array(p, dtype=f32, copy=True)
    st = orc.AdamState(lr=lr, step={0: t - 1}, m={0: np.array(m, dtype=f32, copy=True)},
                       v={0: np.array(v, dtype=f32, copy=True)})
    st.update([p], [np.asarray(g, dtype=f32)])
    return p, st.m[0], st.v[0]


def _adam_exact_bounds(p0, m0, v0, g, p1, m1, v1, lr, t):
    """Bounds on |kernel - oracle| of one Adam step from the SAME float32 inputs, counting the kernel's own operations
    (no contraction, PF_NO_CONTRACT): m = m + b1w (g - m): 3 roundings + the constant's: 4; v = v b2 + (b2w g) g: 4 + 2
    constants: 6; u = u - step (m / (sqrt(v) / bc2s + eps)): sqrt, div, add, div, mul, add and three constants: 9, plus
    the moments' own errors carried through m / denom."""
    p0, m0, v0, g, p1, m1, v1 = (np.asarray(x, dtype=f64) for x in (p0, m0, v0, g, p1, m1, v1))
    step = lr / (1.0 - B1 ** t)
    bc2s = np.sqrt(1.0 - B2 ** t)
    tol_m = 4 * EPS32 * (np.abs(m0) + np.abs(g))
    tol_v = 6 * EPS32 * (np.abs(v0) + g * g)
    sq = np.sqrt(v1)
    denom = sq / bc2s + ADAM_EPS
    d_denom = np.where(sq > 0, tol_v / (2.0 * np.where(sq > 0, sq, 1.0)) / bc2s, 0.0)
    ratio = np.abs(m1) / denom
    tol_p = 9 * EPS32 * (np.abs(p0) + step * ratio) + step * (tol_m / denom + ratio * d_denom / denom)
    return tol_p, tol_m, tol_v


def _adam_interval(p, m, v, g, dg, lr, t):
    """Where one Adam step from the state (p, m, v) can land when the gradient is only known to +-dg (float64).
    m' and v' are monotone in g and |g|.  The step is -step F(g), F = m'(g) / (sqrt(v'(g)) / bc2s + eps), the SAME g in
    both: with a = b1 m, c = 1 - b1, b = b2 v, e = 1 - b2, F' = 0 (eps aside) only at g* = c b / (e a), so F has at most
    one extremum inside [g - dg, g + dg]; its range is taken over the end points, g* and 0 where they lie inside, and 17
    even samples (they cover what eps = 1e-8 moves), widened by 1e-3 of itself.  Returns centre and half width for p, m,
    v; the half widths include the rounding of the step itself (_adam_exact_bounds' counts)."""
    p, m, v, g = (np.asarray(x, dtype=f64) for x in (p, m, v, g))
    dg = np.broadcast_to(np.asarray(dg, dtype=f64), g.shape)
    glo, ghi = g - dg, g + dg
    m_of = lambda x: m + (1 - B1) * (x - m)
    v_of = lambda x: B2 * v + (1 - B2) * x * x
    step = lr / (1.0 - B1 ** t)
    bc2s = np.sqrt(1.0 - B2 ** t)
    F = lambda x: m_of(x) / (np.sqrt(v_of(x)) / bc2s + ADAM_EPS)
    with np.errstate(divide="ignore", invalid="ignore"):
        gstar = np.nan_to_num(((1 - B1) * B2 * v) / ((1 - B2) * B1 * m), nan=0.0, posinf=0.0, neginf=0.0)
    cand = [glo + (ghi - glo) * k / 16.0 for k in range(17)] + [np.clip(gstar, glo, ghi), np.clip(0.0, glo, ghi)]
    vals = np.stack([F(x) for x in cand])
    r_lo, r_hi = vals.min(axis=0), vals.max(axis=0)
    grow = 1e-3 * (r_hi - r_lo)
    r_lo, r_hi = r_lo - grow, r_hi + grow
    p_lo, p_hi = p - step * r_hi, p - step * r_lo
    m_lo, m_hi = m_of(glo), m_of(ghi)
    g2_hi = np.maximum(glo * glo, ghi * ghi)
    g2_lo = np.where((glo <= 0) & (ghi >= 0), 0.0, np.minimum(glo * glo, ghi * ghi))
    v_lo, v_hi = B2 * v + (1 - B2) * g2_lo, B2 * v + (1 - B2) * g2_hi
    rmax = np.maximum(np.abs(r_lo), np.abs(r_hi))
    slack_p = 16 * EPS32 * (np.abs(p) + step * rmax)
    slack_m = 4 * EPS32 * (np.abs(m) + np.abs(g) + dg)
    slack_v = 6 * EPS32 * (np.abs(v) + g2_hi)
    return ((0.5 * (p_lo + p_hi), 0.5 * (p_hi - p_lo) + slack_p), (0.5 * (m_lo + m_hi), 0.5 * (m_hi - m_lo) + slack_m),
            (0.5 * (v_lo + v_hi), 0.5 * (v_hi - v_lo) + slack_v))


def _inside(got, centre_half):
    centre, half = centre_half
    dif = np.abs(np.asarray(got, dtype=f64) - centre)
    ok = half > 0
    assert np.all(dif[~ok] == 0)
    return float(np.max(dif[ok] / half[ok])) if ok.any() else 0.0


@pytest.mark.parametrize("key", list(CASES))
def test_iterations_one_and_two_against_the_oracle_adam_step(key):
    from pinn_fem_amd import _capi
    case, w = _case(key), _world(key)
    name = CASES[key][0]
    lr_u = LR_U[name]
    u0 = _u0(key, fixed_start=True)
    assert np.count_nonzero(u0[case.fixed]) == case.fixed.size
    w.begin(u0, LAM, _config(key))
    n_if, n_t = w.n_iface, w.n_theta_active
    fixed_g = np.zeros(case.n_dofs, dtype=bool)
    fixed_g[case.fixed] = True
    u2_prev = [f32(0.0)] * w.world
    for it in (1, 2):        # the first step uses k_reset's Adam scalars, the second finalize_body's
        pre = {n: w.global_vector(n) for n in ("u", "m_u", "v_u")}
        pre_loc = [{n: w.local(r, n) for n in ("u", "m_u", "v_u")} for r in range(w.world)]
        pre_t = {n: w.local(0, n) for n in ("theta", "m_t", "v_t")}
        w.forward()
        w.backward()
        w.update_interior()
        w.reduce()
        tail = w.n_buf - 3
        for r in range(w.world):     # the lagging u-norm: every rank sends its own sum of the previous iteration
            assert _bits(w.parts[r][tail + 2]) == _bits(u2_prev[r])
        w.update_shared()

        # (a) bit-identical replicas
        _assert_copies_identical(w)
        # (b) fixed dofs are exactly 0 on every copy (they started at 0.3 / 0.2), their moments untouched
        for r in range(w.world):
            fx = (w.flags(r) & _capi.PF_DOF_FIXED) != 0
            assert np.all(w.local(r, "u")[fx] == 0.0)
            assert np.all(w.local(r, "m_u")[fx] == 0.0) and np.all(w.local(r, "v_u")[fx] == 0.0)

        # (c) the interface dofs and theta from the very gradient the kernel was given (the reduced buffer): the
        # oracle's float32 Adam step from the same state, within the operation count
        worst = 0.0
        for r, be in enumerate(w.backends):
            sd, ss = be.shard.shared_dofs, be.shard.shared_slot
            fr = (w.flags(r)[sd] & _capi.PF_DOF_FIXED) == 0
            sd, ss = sd[fr], ss[fr]
            g = w.sum32[ss]
            p0, m0, v0 = (pre_loc[r][n][sd] for n in ("u", "m_u", "v_u"))
            p1, m1, v1 = _adam_f32(p0, m0, v0, g, lr_u, it)
            tols = _adam_exact_bounds(p0, m0, v0, g, p1, m1, v1, lr_u, it)
            for nm, want, tol in zip(("u", "m_u", "v_u"), (p1, m1, v1), tols):
                dif = np.abs(w.local(r, nm)[sd].astype(f64) - want.astype(f64))
                assert np.all(dif[tol == 0] == 0)
                if (tol > 0).any():
                    worst = max(worst, float(np.max(dif[tol > 0] / tol[tol > 0])))
        assert _ratio(2, key, f"it {it}: interface Adam step from the reduced gradient (2^-24 count)", worst, 1.0) < 1
        if n_t:
            g = w.sum32[n_if:n_if + n_t]
            p1, m1, v1 = _adam_f32(pre_t["theta"], pre_t["m_t"], pre_t["v_t"], g, LR_T, it)
            tols = _adam_exact_bounds(pre_t["theta"], pre_t["m_t"], pre_t["v_t"], g, p1, m1, v1, LR_T, it)
            worst = 0.0
            for nm, want, tol in zip(("theta", "m_t", "v_t"), (p1, m1, v1), tols):
                dif = np.abs(w.local(0, nm).astype(f64) - want.astype(f64))
                assert np.all(dif[tol == 0] == 0)
                worst = max(worst, float(np.max(dif[tol > 0] / tol[tol > 0])))
            assert _ratio(2, key, f"it {it}: theta Adam step from the reduced gradient (2^-24 count)", worst, 1.0) < 1

        # (d) the gathered global state against the oracle's step from the same state.  The oracle's gradient is what
        # the kernels are held to within dg = 5e-5 max|grad_u| (5e-4 max|grad_theta|); where |g| is not resolved to
        # that, Adam's first steps are lr * sign(g) and the last bits decide the sign.  So the bound is the interval
        # the step can reach for a gradient within +-dg of the oracle's, plus the step's own rounding.
        pb, ref, ref_t = _oracle_step(case, pre["u"], pre_t["theta"][:n_t], key)
        dg = 5e-5 * np.max(np.abs(ref.grad_u))
        iv = _adam_interval(pre["u"], pre["m_u"], pre["v_u"], ref.grad_u, dg, lr_u, it)
        free = ~fixed_g
        got = {n: w.global_vector(n) for n in ("u", "m_u", "v_u")}
        assert np.all(got["u"][fixed_g] == 0.0)
        for nm, cw in zip(("u", "m_u", "v_u"), iv):
            rr = _inside(got[nm][free], (cw[0][free], cw[1][free]))
            assert _ratio(2, key, f"it {it}: global {nm} vs the oracle's Adam step", rr, 1.0) < 1
        # the bound is not vacuous: for most dofs the interval is a small part of one step
        assert np.median(iv[0][1][free]) < 0.1 * lr_u
        if n_t:
            dgt = 5e-4 * np.max(np.abs(ref_t))
            ivt = _adam_interval(pre_t["theta"], pre_t["m_t"], pre_t["v_t"], ref_t, dgt, LR_T, it)
            for nm, cw in zip(("theta", "m_t", "v_t"), ivt):
                rr = _inside(w.local(0, nm)[:n_t], cw)
                assert _ratio(2, key, f"it {it}: {nm} vs the oracle's Adam step", rr, 1.0) < 1

        # (e) every rank's u2 = sum u_free^2 over the dofs it OWNS (float32 products, summed in float32 per block and in
        # double across blocks: at most n_local 2^-24 relative), so the ranks' sum counts every dof once
        total = 0.0
        for r, be in enumerate(w.backends):
            fl = w.flags(r)
            mine = ((fl & _capi.PF_DOF_FIXED) == 0) & ((fl & _capi.PF_DOF_GHOST) == 0)
            want = float(np.sum(w.local(r, "u")[mine].astype(f64) ** 2))
            u2_prev[r] = w.u2(r)
            total += float(u2_prev[r])
            assert abs(float(u2_prev[r]) - want) <= (fl.size + 2) * EPS32 * want, (r, u2_prev[r], want)
        want = float(np.sum(got["u"][free].astype(f64) ** 2))
        assert _ratio(2, key, f"it {it}: sum of the ranks' u2 vs sum u_free^2", abs(total - want),
                      (case.n_dofs + 2) * EPS32 * want) < 1
        st = [w.state(r) for r in range(w.world)]
        assert all(s.iter == it and s.done == 0 for s in st)


# ---------------------------------------------------------------------------------------------------
# check 3: history and state after 14 iterations in chunks of 5 + 9
# ---------------------------------------------------------------------------------------------------
HIST = ("loss_total", "loss_physics", "loss_data", "u_norm", "residual_norm", "theta_norm")
STATE_FIELDS = ("iter", "done", "converged", "step_size_u", "step_size_t", "bc2_sqrt", "loss_total", "loss_physics",
                "loss_data", "u_norm", "residual_norm", "theta_norm")


def _oracle_history(res):
    return np.array([[h.get(k, 0.0) for k in HIST] for h in res.history], dtype=f64)


def _state_tuple(s):
    return tuple(_bits(getattr(s, f)).item() if isinstance(getattr(s, f), float) else getattr(s, f) for f in STATE_FIELDS)


@pytest.mark.parametrize("key", ["A-w3", "A-w3-delta", "B-w2", "C-w5", "C-w3-mfma", "D-w4", "AE-w3"])
def test_history_and_state_in_two_chunks(key):
    case, w = _case(key), _world(key)
    u0 = _u0(key)
    n = 14
    w.begin(u0, LAM, _config(key))
    for _ in range(5):
        w.iteration()
    h = w.history(0, 5)
    assert h[4, 3] == 0.0 and np.all(h[:4, 3] > 0)      # the u-norm travels one iteration late ...
    w.flush()
    u2_sum = f32(0.0)
    for r in range(w.world):
        u2_sum = f32(u2_sum + w.u2(r))
    h = w.history(0, 5)
    assert _bits(h[4, 3]) == _bits(np.sqrt(u2_sum))     # ... and the flush completes the chunk's last row
    w.iterate(9)
    hist = [w.history(r, n) for r in range(w.world)]
    for r in range(1, w.world):
        assert hist[r].tobytes() == hist[0].tobytes(), "history differs between ranks"
    st = [_state_tuple(w.state(r)) for r in range(w.world)]
    assert all(s == st[0] for s in st), st
    assert st[0][:3] == (n, 0, 0)
    _assert_copies_identical(w)

    res = orc.solve_gd(_pb_with_theta(case, _theta0(case)), _oracle_config(key, n), LAM, u_initial=u0, fe_mode=_fe(key))
    want = _oracle_history(res)
    eng = _single(key)
    eng.begin(torch.from_numpy(u0), LAM, _config(key))
    eng.iterate(n, use_graph=False)
    one = eng.history(n).astype(f64)
    got = hist[0].astype(f64)
    assert got.shape == want.shape == one.shape == (n, 6)
    col_err = lambda a, b, c: float(np.max(np.abs(a[:, c] - b[:, c])) / max(np.max(np.abs(b[:, c])), 1e-300))
    # loss_physics 1e-4, loss_data 1e-5: the single engine's numbers; loss_total is their weighted sum, so it carries
    # the larger; the residual norm is a square root of sum r^2 and carries half of loss_physics'
    stated = {"loss_total": 1e-4, "loss_physics": 1e-4, "loss_data": 1e-5, "residual_norm": 5e-5}
    for c, nm in enumerate(HIST):
        if not np.any(want[:, c]):
            assert not np.any(got[:, c]) and not np.any(one[:, c])
            continue
        e_one = col_err(one, want, c)
        if nm in stated:
            bound = stated[nm]
        else:
            # u_norm, theta_norm: no number of the project's; twice the single engine's own distance from the oracle on
            # this input, plus the float32 summation both norms go through (n terms: at most n 2^-24 relative)
            n_terms = case.n_dofs if nm == "u_norm" else max(w.n_theta_active, 1)
            bound = 2.0 * e_one + (n_terms + w.world) * EPS32
        assert _ratio(3, key, f"history {nm} vs oracle (single engine: {e_one:.3e})", col_err(got, want, c), bound) < 1
        assert _ratio(3, key, f"history {nm} vs single engine", col_err(got, one, c), bound) < 1
    so = eng.state()
    assert (so.iter, so.done, so.converged) == st[0][:3]


# ---------------------------------------------------------------------------------------------------
# check 4: the stop inside a chunk
# ---------------------------------------------------------------------------------------------------
def _snapshot(w):
    out = []
    for r in range(w.world):
        out.append(tuple(w.local(r, n).tobytes() for n in ("u", "m_u", "v_u", "theta", "m_t", "v_t")) +
                   (w.history(r, w.backends[r].eng.hist_rows).tobytes(),))
    return out


def _check_stopped(key, w, n_stop, converged, res, eng):
    st = [w.state(r) for r in range(w.world)]
    so = eng.state()
    for s in st + [so]:
        assert (s.iter, s.done, s.converged) == (n_stop, 1, int(converged))
    assert len(res.history) == n_stop and bool(res.converged) == bool(converged)
    # from the stop on nothing moves, and the ranks send zeros
    before = _snapshot(w)
    w.fill_bufs(7.0)
    w.iteration()
    assert all(not np.any(p) for p in w.parts), "buf after backward is not all zeros once done"
    assert _snapshot(w) == before
    assert [(s.iter, s.done, s.converged) for s in (w.state(r) for r in range(w.world))] == [(n_stop, 1, int(converged))] * w.world
    # the flush after the chunk still writes the final row's u_norm
    assert w.history(0, n_stop)[n_stop - 1, 3] == 0.0
    w.flush()
    u2_sum = f32(0.0)
    for r in range(w.world):
        u2_sum = f32(u2_sum + w.u2(r))
    for r in range(w.world):
        h = w.history(r, n_stop)
        assert _bits(h[n_stop - 1, 3]) == _bits(np.sqrt(u2_sum)) and h[n_stop - 1, 3] > 0
        assert np.all(h[:, 3] > 0)
    want = res.history[-1]["u_norm"]
    one = float(eng.history(n_stop)[n_stop - 1, 3])
    case = _case(key)
    bound = 2.0 * abs(one - want) / want + (case.n_dofs + w.world) * EPS32
    assert _ratio(4, key, "final row u_norm vs oracle", abs(float(h[n_stop - 1, 3]) - want) / want, bound) < 1


@pytest.mark.parametrize("key", ["A-w3", "C-w5"])
def test_stop_by_tolerance_inside_a_chunk(key):
    case, w = _case(key), _world(key)
    u0 = _u0(key)
    pb = lambda: _pb_with_theta(case, _theta0(case))
    free_run = orc.solve_gd(pb(), _oracle_config(key, 20), LAM, u_initial=u0, fe_mode=_fe(key))
    q = np.array([min(h["residual_norm"], h["loss_total"]) for h in free_run.history])
    # the stop test runs from the 12th iteration on (it > 10, 0-based): the first it in 12..19 (0-based) whose value
    # lies clearly below every earlier tested one: by 2e-4 on either side of the tolerance, twice the bound the loss and
    # four times the bound the residual norm are held to (check 3), so that the kernels stop where the oracle does
    tol = None
    for it in range(12, 20):
        lo, hi = q[it], np.min(q[11:it])
        if lo * (1 + 2e-4) < hi * (1 - 2e-4):
            tol = float(np.sqrt(lo * hi))
            break
    assert tol is not None
    res = orc.solve_gd(pb(), _oracle_config(key, 40, tol), LAM, u_initial=u0, fe_mode=_fe(key))
    n_stop = len(res.history)
    assert res.converged and 12 <= n_stop <= 20 and n_stop == it + 1
    cfg = _config(key, 40, tol)
    eng = _single(key)
    eng.begin(torch.from_numpy(u0), LAM, cfg)
    eng.iterate(25, use_graph=False)
    w.begin(u0, LAM, cfg)
    for _ in range(25):                     # one chunk; the stop falls inside it
        w.iteration()
    _check_stopped(key, w, n_stop, True, res, eng)


@pytest.mark.parametrize("key", ["A-w3", "D-w4"])
def test_stop_by_max_iterations_inside_a_chunk(key):
    case, w = _case(key), _world(key)
    u0 = _u0(key)
    res = orc.solve_gd(_pb_with_theta(case, _theta0(case)), _oracle_config(key, 7), LAM, u_initial=u0, fe_mode=_fe(key))
    cfg = _config(key, 7)
    eng = _single(key)
    eng.begin(torch.from_numpy(u0), LAM, cfg)
    eng.iterate(10, use_graph=False)
    w.begin(u0, LAM, cfg)
    for _ in range(10):
        w.iteration()
    _check_stopped(key, w, 7, False, res, eng)


# ---------------------------------------------------------------------------------------------------
# check 5: the result does not depend on the split
# ---------------------------------------------------------------------------------------------------
def _oracle_reach(case, key, u0, k):
    """(u, theta) of the oracle after k iterations from u0 and the reach B_k of the docstring below, per dof."""
    lr_u = LR_U[CASES[key][0]]
    pb = _pb_with_theta(case, _theta0(case))
    geo = orc.element_geometry(pb)
    theta = pb.theta_list()
    free = np.ones(case.n_dofs, dtype=bool)
    free[case.fixed] = False
    u = u0.copy()
    opt_u, opt_t = orc.AdamState(lr=lr_u), orc.AdamState(lr=LR_T)
    B = np.zeros(case.n_dofs)
    data_w = np.zeros(case.n_dofs)
    data_w[case.md] = 2.0 * ALPHA_D / len(case.mv)
    for t in range(1, k + 1):
        ref = orc.loss_and_grads(pb, geo, u, LAM, ALPHA_P, ALPHA_D, acc64=True)
        ka = np.abs(ref.stiffness.astype(f64)[:, None, None] * geo.pattern.astype(f64))
        kb = np.zeros(case.n_dofs)
        np.add.at(kb, geo.dofs.reshape(-1), np.einsum("eab,eb->ea", ka, B[geo.dofs]).reshape(-1))       # |K| B
        kb[~free] = 0.0
        kkb = np.zeros(case.n_dofs)
        np.add.at(kkb, geo.dofs.reshape(-1), np.einsum("eab,eb->ea", ka, kb[geo.dofs]).reshape(-1))     # |K|^T |K| B
        dg = 5e-5 * np.max(np.abs(ref.grad_u)) + ALPHA_P * kkb + data_w * B
        m = opt_u.m.get(0, np.zeros(case.n_dofs, f32))
        v = opt_u.v.get(0, np.zeros(case.n_dofs, f32))
        iv = _adam_interval(u, m, v, ref.grad_u, dg, lr_u, t)
        B = B + iv[0][1]
        opt_u.update([u], [ref.grad_u])
        opt_t.update(theta, ref.grad_theta)
        u[~free] = 0.0
    B[~free] = 0.0
    th_ref = np.concatenate([x.reshape(-1) for x in theta]).astype(f64)
    return u, th_ref, B, free


def test_split_invariance_world_3_5_and_single():
    """Mesh C after 10 iterations at world 3, world 5 and on one engine.  Bound: check 2's interval, grown over the
    iterations.  Along the oracle's own trajectory the reach B_t of a run that started from the same state is
        B_t = B_{t-1} + (half width of the Adam interval of iteration t for a gradient within +-dg_t),
        dg_t = 5e-5 max|g_t| + |dg/du| B_{t-1},   |dg/du| = alpha_p |K|^T |K| + 2 alpha_d / m on the measured dofs:
    the kernels' gradient error as in check 2, plus (first order) what the displacement difference so far does to the
    gradient.  Each run stays within B_10 of the oracle, so two runs within 2 B_10 of each other; theta is held to the
    2e-5 the project's sharded-vs-single tests use."""
    k = 10
    key = "C-w3"
    case = _case(key)
    lr_u = LR_U["C"]
    u0 = _u0(key)
    runs = {}
    for kk in ("C-w3", "C-w5"):
        w = _world(kk)
        w.begin(u0, LAM, _config(kk))
        w.iterate(k)
        _assert_copies_identical(w)
        runs[kk] = (w.global_vector("u").astype(f64), w.local(0, "theta").astype(f64))
    eng = _single(key)
    eng.begin(torch.from_numpy(u0), LAM, _config(key))
    eng.iterate(k, use_graph=False)
    torch.cuda.synchronize()
    runs["single"] = (eng.u.cpu().numpy().astype(f64), eng.theta.flat.cpu().numpy().astype(f64))

    u, th_ref, B, free = _oracle_reach(case, key, u0, k)
    names = list(runs)
    for a in names:
        dif = np.abs(runs[a][0] - u.astype(f64))
        assert np.all(dif[~free] == 0)
        assert _ratio(5, a, f"u after {k} iterations vs oracle, B_{k}", np.max(dif[free] / B[free]), 1.0) < 1
        assert _ratio(5, a, "theta vs oracle", np.max(np.abs(runs[a][1] - th_ref)) / np.max(np.abs(th_ref)), 2e-5) < 1
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            dif = np.abs(runs[a][0] - runs[b][0])
            assert _ratio(5, f"{a}|{b}", f"u after {k} iterations, 2 B_{k}", np.max(dif[free] / (2 * B[free])), 1.0) < 1
            assert _ratio(5, f"{a}|{b}", "theta", np.max(np.abs(runs[a][1] - runs[b][1])) / np.max(np.abs(th_ref)),
                          2e-5) < 1
    print(f"shard-ratio check=5 median B_{k} / lr_u = {np.median(B[free]) / lr_u:.3e}, max = {np.max(B[free]) / lr_u:.3e}")


# ---------------------------------------------------------------------------------------------------
# check 6: argument errors are refusals (nothing launches)
# ---------------------------------------------------------------------------------------------------
def test_argument_errors_refuse_without_launching():
    from pinn_fem_amd import _capi
    key = "C-w3"
    w = _world(key)
    w.begin(_u0(key), LAM, _config(key))
    w.iteration()                                  # a live state: a launch would change it
    be = w.backends[1]                             # the middle rank: own_lo > 0
    e, lib = be.eng, be.eng.lib
    buf, u2 = be.bufs
    buf.fill_(7.0)
    torch.cuda.synchronize()
    s = e._stream()
    watched = lambda: tuple(t.cpu().numpy().tobytes() for t in (buf, u2, e.u, e.m_u, e.v_u, e.theta.flat, e.m_t, e.v_t,
                                                                  e.state_t, e.hist, e.g_f, e.partials))
    before = watched()

    def record(**changes):
        q = _capi.PfProblem()
        C.memmove(C.byref(q), C.byref(e.P), C.sizeof(_capi.PfProblem))
        for k, v in changes.items():
            setattr(q, k, v)
        return q

    P = e.P
    assert P.n_shared > 0 and P.own_lo > 0 and P.n_theta_active > 0
    four = {
        "pf_shard_forward": lambda q: lib.pf_shard_forward(C.byref(q), s),
        "pf_shard_backward": lambda q: lib.pf_shard_backward(C.byref(q), buf.data_ptr(), u2.data_ptr(), s),
        "pf_shard_update_interior": lambda q: lib.pf_shard_update_interior(C.byref(q), s),
        "pf_shard_update_shared": lambda q: lib.pf_shard_update_shared(C.byref(q), buf.data_ptr(), u2.data_ptr(), s),
    }
    bad_records = [
        (dict(n_iface=P.n_shared - 1), "bad interface sizes"),
        (dict(n_shared=-1), "bad interface sizes"),
        (dict(shared_dofs=None), "null interface maps"),
        (dict(shared_slot=None), "null interface maps"),
        (dict(own_hi=P.mesh.n_elems + 1), "bad own element range"),
        (dict(own_hi=P.own_lo - 1), "bad own element range"),
        (dict(own_lo=-1), "bad own element range"),
    ]
    calls = [(name, fn, record(**ch), msg) for ch, msg in bad_records for name, fn in four.items()]
    good = record()
    calls += [
        ("pf_shard_backward", four["pf_shard_backward"], record(grad_theta=buf.data_ptr() + 4 * (P.n_iface + 1)),
         "p->grad_theta must point at buf + n_iface"),
        ("pf_shard_backward", four["pf_shard_backward"], record(grad_theta=e.grad_theta.data_ptr()),
         "p->grad_theta must point at buf + n_iface"),
        ("pf_shard_backward", lambda q: lib.pf_shard_backward(C.byref(q), None, u2.data_ptr(), s), good, "null buf / u2_local"),
        ("pf_shard_backward", lambda q: lib.pf_shard_backward(C.byref(q), buf.data_ptr(), None, s), good, "null buf / u2_local"),
        ("pf_shard_update_shared", lambda q: lib.pf_shard_update_shared(C.byref(q), None, u2.data_ptr(), s), good, "null buffer"),
        ("pf_shard_update_shared", lambda q: lib.pf_shard_update_shared(C.byref(q), buf.data_ptr(), None, s), good, "null buffer"),
        ("pf_shard_update_shared", four["pf_shard_update_shared"], record(m_u=None), "null buffer"),
        ("pf_shard_update_shared", four["pf_shard_update_shared"], record(m_t=None), "null Adam moments for theta"),
        ("pf_shard_update_interior", four["pf_shard_update_interior"], record(v_u=None), "null Adam moments for u"),
        ("pf_shard_flush", lambda q: lib.pf_shard_flush(C.byref(q), None, s), good, "null u2"),
        ("pf_shard_flush", lambda q: lib.pf_shard_flush(C.byref(q), u2.data_ptr(), s), record(state=None), "null state/workspace"),
    ]
    for name, fn, q, msg in calls:
        rc = fn(q)
        assert rc == _capi.PF_ERR_ARG, (name, msg, rc)
        assert msg in lib.pf_last_error().decode(), (name, msg, lib.pf_last_error())
    torch.cuda.synchronize()
    assert watched() == before, "a refused call touched a buffer"
    # and the Python seam refuses foreign collective buffers
    other = torch.zeros_like(buf)
    with pytest.raises(ValueError, match="own collective buffers"):
        be.backward(other, u2)
    with pytest.raises(ValueError, match="own collective buffers"):
        be.update_shared(other, u2)
    assert watched() == before
