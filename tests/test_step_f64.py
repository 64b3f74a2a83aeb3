"""The mesh kernels of the float32 gradient-descent iteration, each on its own, per entry against float64.

k_node_residual (both walks), k_elem_adjoint, k_node_gradu with and without the fused Adam step, k_finalize, k_reset,
k_adam, k_diag_k and k_coo_k are called through the C entry points themselves on the engine's stream, with the per-element
fields the nets would have written INJECTED into prop_e, prop_a and elem_k (decade-wide, near-uniform, or with a soft
zone), so that nothing but the mesh kernels stands between the inputs and what is compared.  HipEngine.internal_force() and
diag_k() are not used: they re-evaluate the nets over the injection.

Reference, stand-in, bounds and meshes: tests/step_reference.py.  Every bound is a rounding count times 2^-24 times the
magnitudes the roundings act on; the test asserts error / bound <= 1 per entry.  Each check prints
"step-ratio case=... quantity=... err ... bound ... ratio ..." (and the float32 stand-in's ratio on the same case, the
yardstick) in front of its assertion; a recorded run is profiles/step_kernel_ratios.txt.
"""

import numpy as np
import pytest
import torch

import step_reference as sr
from helpers import load_npz, product_model, theta_from

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
LAM, LR_U, LR_T = 0.7, 1e-3, 3e-4

# engine key -> (dimension, wg_mode, fixture, widths, scales)
ENGINES = {
    "wg3": (2, 3, "step_warren_EA.npz", (20, 15, None), (2.0, 0.5, 1.0)),     # MFMA32: the node kernels read elem_k
    "wg1": (2, 1, "step_warren_EA.npz", (20, 15, None), (2.0, 0.5, 1.0)),     # no records: ke from prop_e, prop_a, egeo
    "1d": (1, 3, "step_bar1d_E.npz", (20, None, None), (3.0, 2.0, 1.0)),      # E net only: A is the scalar `scale`
}

# case key -> (mesh maker, engine, field, fe_mode, alpha_physics, alpha_data, with measurements)
CASES = {}
for _n in sr.SMALL_SIZES:
    CASES[f"grid{_n}-wg3"] = ((lambda n=_n: sr.grid_case(n)), "wg3", "decades", 0, 1.0, 100.0, True)
    CASES[f"chain2d{_n}-wg3"] = ((lambda n=_n: sr.chain_case(n, 2)), "wg3", "decades", 0, 1.0, 100.0, True)
    CASES[f"chain1d{_n}"] = ((lambda n=_n: sr.chain_case(n, 1)), "1d", "decades", 0, 1.0, 100.0, True)
for _n in (3, 257, 513):
    CASES[f"grid{_n}-wg1"] = ((lambda n=_n: sr.grid_case(n)), "wg1", "decades", 0, 1.0, 100.0, True)
CASES.update({
    "hub-wg3": (sr.hub_case, "wg3", "decades", 0, 1.0, 100.0, True),
    "hub-wg3-delta": (sr.hub_case, "wg3", "decades", 1, 1.0, 100.0, True),
    "hub-wg1": (sr.hub_case, "wg1", "decades", 0, 1.0, 100.0, True),
    "hub-wg1-delta": (sr.hub_case, "wg1", "decades", 1, 1.0, 100.0, True),
    "hub-wg3-uniform": (sr.hub_case, "wg3", "uniform", 0, 1.0, 100.0, True),
    "hub-wg3-softzone": (sr.hub_case, "wg3", "softzone", 0, 1.0, 100.0, True),
    "hub-wg3-alpha3-nodata": (sr.hub_case, "wg3", "decades", 0, 3.0, 0.0, True),      # measured dofs, alpha_data = 0
    "hub-wg3-alpha3": (sr.hub_case, "wg3", "decades", 0, 3.0, 100.0, True),
    "hub-wg3-nomeas": (sr.hub_case, "wg3", "decades", 0, 1.0, 100.0, False),          # no measurements at all
    "chain1d513-delta": ((lambda: sr.chain_case(513, 1)), "1d", "decades", 1, 1.0, 100.0, True),
    "chain1d513-ramp": ((lambda: sr.chain_case(513, 1, ramp=True)), "1d", "decades", 0, 1.0, 100.0, True),
    "chain1d513-ramp-delta": ((lambda: sr.chain_case(513, 1, ramp=True)), "1d", "decades", 1, 1.0, 100.0, True),
    "chain2d513-ramp": ((lambda: sr.chain_case(513, 2, ramp=True)), "wg3", "decades", 0, 1.0, 100.0, True),
    # 1024 blocks x 256 threads x 2 nodes = 524 288 per trip of the paired walk: a second trip, whose second node 77 threads have
    "chain1d-long-ramp": ((lambda: sr.chain_case(sr.LONG_NODES, 1, ramp=True)), "1d", "decades", 0, 1.0, 100.0, True),
    "chain2d-long": ((lambda: sr.chain_case(sr.LONG_NODES, 2)), "wg3", "decades", 0, 1.0, 100.0, True),
})
YARDSTICK_MAX_NODES = 10_000       # the stand-in's ratios are printed beside the device's up to this size (larger: the host test's)

_engines = {}


def _engine(case, engine_key, with_meas):
    from pinn_fem_amd.engine import HipEngine
    key = (case.name, engine_key, with_meas)
    if key not in _engines:
        dim, wg, fixture, widths, scales = ENGINES[engine_key]
        assert dim == case.dim
        model = product_model(case.nodes, case.elements, case.loads, case.fixed, dim, widths, scales, theta_from(load_npz(fixture)))
        if len(_engines) >= 6:                     # the long chains hold ~100 MB each: keep only the last few engines
            _engines.pop(next(iter(_engines)))
        _engines[key] = HipEngine(model, case.meas_vals if with_meas else None, case.meas_dofs if with_meas else None,
                                  wg_mode=wg)
    return _engines[key]


def _dev(eng, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


def _host(t):
    return t.detach().cpu().numpy().copy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def _call(eng, name, *args):
    from pinn_fem_amd import _capi
    _capi.check(getattr(eng.lib, name)(eng._ref(), *args, eng._stream()), name)


class _Report:
    """Prints a step-ratio line per check and keeps the failures: a case runs all its checks, then asserts once."""

    def __init__(self, case):
        self.case, self.failed = case, []

    def ratio(self, quantity, err, bound, standin=None):
        err, bound = np.abs(np.asarray(err, dtype=f64)).reshape(-1), np.asarray(bound, dtype=f64).reshape(-1)
        r = sr.worst_ratio(err, bound)
        k = int(np.argmax(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0)))) if err.size else 0
        extra = "" if standin is None else f" standin {standin:.3f}"
        print(f"step-ratio case={self.case} quantity={quantity} err {err[k] if err.size else 0.0:.3e} bound "
              f"{bound[k] if err.size else 0.0:.3e} ratio {r:.3f}{extra}")
        if not r <= 1.0:
            self.failed.append(f"{quantity}: ratio {r:.3f}")
        return r

    def same(self, quantity, ok, detail=""):
        print(f"step-ratio case={self.case} quantity={quantity} identical {int(bool(ok))} {detail}")
        if not ok:
            self.failed.append(f"{quantity}: not identical {detail}")


def _configure(eng, fe, alpha_p, alpha_d, max_iter=5000):
    eng.fe_mode = fe
    eng.configure(lam=LAM, alpha_physics=alpha_p, alpha_data=alpha_d, lr_u=LR_U, lr_t=LR_T, tol=0.0, max_iter=max_iter,
                  want_history=False, want_grad_u=True)
    _call(eng, "pf_reset")
    eng._clear_done()


def _inject(eng, mesh, E, A, rec, u):
    ne = mesh.n_elems
    eng.prop_e[:ne].copy_(_dev(eng, E))
    eng.prop_a[:ne].copy_(_dev(eng, A))
    if eng.elem_k is not None:
        img = sr.record_image(mesh, rec)
        eng.elem_k[: img.size].copy_(_dev(eng, img))
    eng.u.copy_(_dev(eng, u))


def _state(eng):
    return eng.state()


@pytest.mark.parametrize("key", list(CASES))
def test_step_kernels_per_entry(key):
    make, engine_key, kind, fe, alpha_p, alpha_d, with_meas = CASES[key]
    case = make()
    eng = _engine(case, engine_key, with_meas)
    mesh = sr.mesh_from_plan(eng.plan)
    E, A = sr.fields(kind, mesh.n_elems)
    # a property without a net is the scalar the record holds (the 1-D engine's area)
    E_ref = E if eng.specs[0].enabled else f32(eng.specs[0].scale)
    A_ref = A if eng.specs[1].enabled else f32(eng.specs[1].scale)
    rec = sr.records(mesh, E_ref, A_ref)
    u = case.u
    use_data = bool(with_meas and alpha_d > 0)
    rep = _Report(key)
    yard = (sr.standin_ratios(mesh, rec, u, LAM, alpha_p, alpha_d, use_data, fe) if mesh.n_nodes <= YARDSTICK_MAX_NODES else {})
    nd = mesh.n_dofs
    with eng.on_stream():
        _configure(eng, fe, alpha_p, alpha_d)
        assert int(eng.P.use_data) == int(use_data)
        _inject(eng, mesh, E, A, rec, u)
        new = lambda n, dt=torch.float32: torch.full((n,), 7, dtype=dt, device=eng.device)

        # ---- f_int per dof: pf_internal_force takes the one-node walk ---------------------------------------------------
        f_out = new(nd)
        _call(eng, "pf_internal_force", eng.u.data_ptr(), f_out.data_ptr())
        f_dev = _host(f_out)
        f, S = sr.gather64(mesh, rec, u)
        rep.ratio("f_int", f_dev - f, sr.gather_bound(mesh, S), yard.get("f_int"))

        # ---- g_f from both walks -----------------------------------------------------------------------------------------
        eng.g_f.fill_(7.0)
        _call(eng, "pf_node_residual", None)                       # NULL f_int_out: the paired walk where elem_k exists
        g_pair = _host(eng.g_f)
        eng.g_f.fill_(7.0)
        f_out2 = new(nd)
        _call(eng, "pf_node_residual", f_out2.data_ptr())          # the one-node walk
        g_one = _host(eng.g_f)
        rep.same("g_f paired walk == one-node walk (bytes)", np.array_equal(_bits(g_pair), _bits(g_one)),
                 f"{np.count_nonzero(_bits(g_pair) != _bits(g_one))} differ")
        rep.same("f_int of pf_node_residual == pf_internal_force (bytes)", np.array_equal(_bits(_host(f_out2)), _bits(f_dev)))
        _, g64 = sr.residual64(mesh, f, LAM, alpha_p)
        g_b = sr.residual_bound(mesh, f, S, LAM, alpha_p)
        rep.ratio("g_f (paired walk)", g_pair - g64, g_b, yard.get("g_f"))
        rep.ratio("g_f (one-node walk)", g_one - g64, g_b, yard.get("g_f"))
        rep.same("g_f exactly 0 on fixed dofs", not np.any(g_pair[mesh.fixed]) and not np.any(g_one[mesh.fixed]))
        g_dev = g_one

        # ---- loss sums and monitors: pf_finalize from the residual's block partials -------------------------------------------
        _call(eng, "pf_finalize")
        st = _state(eng)
        lt = sr.loss_terms64(mesh, g_dev, u, use_data, alpha_p, alpha_d)
        # alpha_physics != 1: g_f / alpha gives r back only to one rounding, twice in a square
        rel = sr.sum_bound(mesh) + (0.0 if alpha_p == 1.0 else 2.0 * sr.EPS32)
        rep.ratio("loss_physics", st.loss_physics - lt["loss_physics"], rel * lt["loss_physics"])
        rep.ratio("residual_norm", st.residual_norm - lt["residual_norm"], rel * lt["residual_norm"])
        rep.ratio("loss_data", st.loss_data - lt["loss_data"], rel * lt["loss_data"])
        rep.ratio("loss_total", st.loss_total - lt["loss_total"],
                  sr.total_bound(mesh, lt, use_data, alpha_p, alpha_d) + (rel - sr.sum_bound(mesh)) * abs(lt["loss_total"]))
        rep.same("iter advanced to 1", st.iter == 1 and st.done == 0)

        # ---- g_ea per element ------------------------------------------------------------------------------------------
        eng.g_ea.fill_(7.0)
        _call(eng, "pf_elem_adjoint")
        ge, ge_b = sr.gea64(mesh, g_dev, u)
        rep.ratio("g_ea", _host(eng.g_ea)[: mesh.n_elems] - ge, ge_b, yard.get("g_ea"))

        # ---- grad_u per dof, from the device's own g_f -------------------------------------------------------------------
        eng.grad_u.fill_(7.0)
        _call(eng, "pf_node_gradu", 0)
        gu_dev = _host(eng.grad_u)
        gu, gu_b = sr.grad_u64(mesh, rec, g_dev, u, use_data, alpha_d)
        rep.ratio("grad_u", gu_dev - gu, gu_b, yard.get("grad_u"))
        rep.same("u untouched by the unfused launch", np.array_equal(_bits(_host(eng.u)), _bits(u)))

        # ---- the fused step ----------------------------------------------------------------------------------------------
        rng = np.random.default_rng(11)
        m0 = (0.1 * rng.standard_normal(nd)).astype(f32)
        v0 = (0.01 * rng.random(nd)).astype(f32)
        eng.m_u.copy_(_dev(eng, m0))
        eng.v_u.copy_(_dev(eng, v0))
        eng.grad_u.fill_(7.0)
        step, bc2s = f32(st.step_size_u), f32(st.bc2_sqrt)          # the state's own scalars (step 2: finalize has run once)
        _call(eng, "pf_node_gradu", 1)
        u1, m1, v1 = _host(eng.u), _host(eng.m_u), _host(eng.v_u)
        rep.same("grad_u of the fused launch == unfused (bytes)", np.array_equal(_bits(_host(eng.grad_u)), _bits(gu_dev)))
        p64, m64, v64, bp, bm, bv = sr.adam64(u, m0, v0, gu_dev, step, bc2s)
        free = ~mesh.fixed
        ps, ms, vs = sr.adam32(u, m0, v0, gu_dev, step, bc2s)      # the stand-in from the same state and gradient
        rep.ratio("adam m_u", (m1 - m64)[free], bm[free], sr.worst_ratio((ms - m64)[free], bm[free]))
        rep.ratio("adam v_u", (v1 - v64)[free], bv[free], sr.worst_ratio((vs - v64)[free], bv[free]))
        rep.ratio("adam u", (u1 - p64)[free], bp[free], sr.worst_ratio((ps - p64)[free], bp[free]))
        rep.same("fixed dofs are 0 after the step", not np.any(u1[mesh.fixed]))
        rep.same("moments of fixed dofs untouched (bytes)", np.array_equal(_bits(m1[mesh.fixed]), _bits(m0[mesh.fixed]))
                 and np.array_equal(_bits(v1[mesh.fixed]), _bits(v0[mesh.fixed])))
        _call(eng, "pf_finalize")
        st2 = _state(eng)
        un = float(np.sqrt(np.sum(u1.astype(f64)[free] ** 2)))
        rep.ratio("u_norm", st2.u_norm - un, sr.sum_bound(mesh) * un)

        # ---- diag(K) and K in coordinate format, from the injected fields -----------------------------------------------------
        d_out = new(nd)
        _call(eng, "pf_diag_k", d_out.data_ptr())
        dk, dk_b = sr.diag64(mesh, rec)
        rep.ratio("diag_k", _host(d_out) - dk, dk_b)
        if mesh.n_nodes <= YARDSTICK_MAX_NODES:
            n_coo = mesh.n_elems * (2 * mesh.dim) ** 2
            rows, cols, vals = new(n_coo, torch.int64), new(n_coo, torch.int64), new(n_coo)
            _call(eng, "pf_coo_k", rows.data_ptr(), cols.data_ptr(), vals.data_ptr())
            r64, c64, v64c = sr.coo64(mesh, rec)
            rep.same("coo_k rows and cols", np.array_equal(_host(rows), r64) and np.array_equal(_host(cols), c64))
            rep.ratio("coo_k vals", _host(vals) - v64c, 4.0 * sr.EPS32 * np.abs(v64c))     # 4 ulp per value, as the entry is a record entry

        # ---- pf_loss_and_grads: the same sums behind the whole single-step entry point.  It evaluates the nets over the injection,
        # which the reference does not mind: it sums the device's own g_f (alpha_physics = 1: r to the bit) ----------------------
        if alpha_p == 1.0:
            eng.u.copy_(_dev(eng, u))
            _call(eng, "pf_pack_theta")
            _call(eng, "pf_loss_and_grads")
            st3 = _state(eng)
            lt3 = sr.loss_terms64(mesh, _host(eng.g_f), u, use_data, alpha_p, alpha_d)
            rel = sr.sum_bound(mesh)
            rep.ratio("loss_physics (pf_loss_and_grads)", st3.loss_physics - lt3["loss_physics"], rel * lt3["loss_physics"])
            rep.ratio("residual_norm (pf_loss_and_grads)", st3.residual_norm - lt3["residual_norm"], rel * lt3["residual_norm"])
            rep.ratio("loss_data (pf_loss_and_grads)", st3.loss_data - lt3["loss_data"], rel * lt3["loss_data"])
            rep.ratio("loss_total (pf_loss_and_grads)", st3.loss_total - lt3["loss_total"],
                      sr.total_bound(mesh, lt3, use_data, alpha_p, alpha_d))
    assert not rep.failed, f"{key}: " + "; ".join(rep.failed)


# ---------------------------------------------------------------------------------------------------
# Adam scalars: k_reset and finalize_body
# ---------------------------------------------------------------------------------------------------
def test_adam_scalars_after_reset_and_finalize():
    """After pf_reset the scalars ARE the double formulas cast to float; after pf_finalize has advanced iter to 1, 10 and
    1000 they agree to 1 float32 ulp (the device's double pow)."""
    case = sr.grid_case(3)
    eng = _engine(case, "wg3", True)
    rep = _Report("adam-scalars")
    with eng.on_stream():
        _configure(eng, 0, 1.0, 100.0, max_iter=5000)
        st = _state(eng)
        for name, lr, got in (("step_size_u", LR_U, st.step_size_u), ("step_size_t", LR_T, st.step_size_t)):
            rep.same(f"{name} after reset", f32(got) == sr.adam_scalars(lr, 1)[0], f"{got!r}")
        rep.same("bc2_sqrt after reset", f32(st.bc2_sqrt) == sr.adam_scalars(LR_U, 1)[1], f"{st.bc2_sqrt!r}")
        rep.same("iter, done, converged 0 after reset", (st.iter, st.done, st.converged) == (0, 0, 0))
        done = 0
        for k in (1, 10, 1000):
            for _ in range(k - done):
                _call(eng, "pf_finalize")
            done = k
            st = _state(eng)
            rep.same(f"iter == {k}", st.iter == k and st.done == 0)
            for name, lr, got, which in (("step_size_u", LR_U, st.step_size_u, 0), ("step_size_t", LR_T, st.step_size_t, 0),
                                         ("bc2_sqrt", LR_U, st.bc2_sqrt, 1)):
                want = sr.adam_scalars(lr, k + 1)[which]             # the NEXT step's scalars: t = iter + 1
                rep.ratio(f"{name} at iter {k}", float(got) - float(want), sr.ulp32(want))
    assert not rep.failed, "; ".join(rep.failed)


@pytest.mark.parametrize("which", ["n_theta > n_dofs", "n_dofs > n_theta"])
def test_reset_zeroes_every_moment(which):
    case = sr.grid_case(3) if which == "n_theta > n_dofs" else sr.hub_case()
    eng = _engine(case, "wg3", True)
    assert (eng.n_theta > eng.plan.n_dofs) == (which == "n_theta > n_dofs") and eng.n_theta != eng.plan.n_dofs
    with eng.on_stream():
        _configure(eng, 0, 1.0, 100.0)
        for t in (eng.m_u, eng.v_u, eng.m_t, eng.v_t):
            t.fill_(7.0)
        eng.state_t[0] = 5
        _call(eng, "pf_reset")
        for name in ("m_u", "v_u", "m_t", "v_t"):
            a = _host(getattr(eng, name))
            n = eng.plan.n_dofs if name.endswith("_u") else eng.n_theta
            assert a.size >= n and not np.any(a[:n]), f"{name}: {np.count_nonzero(a[:n])} of {n} entries not zeroed"
        assert _state(eng).iter == 0


# ---------------------------------------------------------------------------------------------------
# pf_adam: exported, called by nothing
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [1, 1000])
@pytest.mark.parametrize("n", [1, 255, 257, 100_001])
def test_pf_adam(n, step):
    from pinn_fem_amd import _capi
    lib = _capi.load()
    rng = np.random.default_rng(100 * n + step)
    p0, g = rng.standard_normal(n).astype(f32), rng.standard_normal(n).astype(f32)
    m0, v0 = (0.1 * rng.standard_normal(n)).astype(f32), (0.01 * rng.random(n)).astype(f32)
    dev = torch.device("cuda", torch.cuda.current_device())
    tp, tg, tm, tv = (torch.from_numpy(a.copy()).to(dev) for a in (p0, g, m0, v0))
    lr = 1e-3
    _capi.check(lib.pf_adam(tp.data_ptr(), tg.data_ptr(), tm.data_ptr(), tv.data_ptr(), n, step, lr, sr.B1, sr.B2, sr.ADAM_EPS,
                            torch.cuda.current_stream(dev).cuda_stream), "pf_adam")
    torch.cuda.synchronize(dev)
    # k_adam takes lr as a double: step_size = (float)(lr / bc1)
    step_size, bc2s = f32(lr / (1.0 - sr.B1 ** step)), f32(np.sqrt(1.0 - sr.B2 ** step))
    p64, m64, v64, bp, bm, bv = sr.adam64(p0, m0, v0, g, step_size, bc2s)
    ps, ms, vs = sr.adam32(p0, m0, v0, g, step_size, bc2s)
    rep = _Report(f"pf_adam-n{n}-t{step}")
    rep.ratio("m", _host(tm) - m64, bm, sr.worst_ratio(ms - m64, bm))
    rep.ratio("v", _host(tv) - v64, bv, sr.worst_ratio(vs - v64, bv))
    rep.ratio("p", _host(tp) - p64, bp, sr.worst_ratio(ps - p64, bp))
    rep.same("the gradient is untouched", np.array_equal(_bits(_host(tg)), _bits(g)))
    assert not rep.failed, "; ".join(rep.failed)


# ---------------------------------------------------------------------------------------------------
# the device comparison can fail
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine_key", ["wg3", "wg1"])
def test_device_comparison_rejects_two_swapped_soft_elements(engine_key):
    """What tests/test_step_host.py shows of the stand-in, once on the device: the fields of two soft-zone elements that
    meet at a node are handed to the kernel SWAPPED (records for wg_mode 3, E and A for wg_mode 1) while the reference keeps
    the true ones.  The per-dof check must reject f_int; max|a - b| / max|b| < 5e-5 does not notice."""
    from helpers import rel_err
    case = sr.hub_case()
    eng = _engine(case, engine_key, True)
    mesh = sr.mesh_from_plan(eng.plan)
    E, A = sr.fields("softzone", mesh.n_elems)
    rec, u = sr.records(mesh, E, A), case.u
    f, S = sr.gather64(mesh, rec, u)
    Bf = sr.gather_bound(mesh, S)
    s = E.astype(f64) * A.astype(f64) / mesh.egeo[:, 3]
    soft = s <= np.quantile(s, 0.1)
    pair = np.flatnonzero((mesh.inc_node[:-1] == mesh.inc_node[1:]) & soft[mesh.inc_elem[:-1]] & soft[mesh.inc_elem[1:]])
    chosen = None
    for i in pair:
        a, b = mesh.inc_elem[i], mesh.inc_elem[i + 1]
        E2, A2 = E.copy(), A.copy()
        E2[[a, b]], A2[[a, b]] = E[[b, a]], A[[b, a]]
        # wg_mode 3 reads the record, geometry included; wg_mode 1 forms it from the swapped E, A and the element's own geometry
        rec2 = rec.copy()
        if engine_key == "wg3":
            rec2[[a, b]] = rec[[b, a]]
        else:
            rec2 = sr.records(mesh, E2, A2)
        f2, _ = sr.gather64(mesh, rec2, u)
        if sr.worst_ratio(f2 - f, Bf) > 4.0:          # as in the host test: only where the effect is four times the bound
            chosen = (E2, A2, rec2)
            break
    assert chosen is not None, "no pair of soft elements at a node whose swap shows above 4x the bound"
    E2, A2, rec2 = chosen
    with eng.on_stream():
        _configure(eng, 0, 1.0, 100.0)
        _inject(eng, mesh, E2, A2, rec2, u)
        out = torch.full((mesh.n_dofs,), 7, dtype=torch.float32, device=eng.device)
        _call(eng, "pf_internal_force", eng.u.data_ptr(), out.data_ptr())
        f_dev = _host(out)
    r = sr.worst_ratio(f_dev - f, Bf)
    re = rel_err(f_dev, f)
    print(f"step-ratio case=hub-{engine_key}-softzone-swapped quantity=f_int against the unswapped reference (must exceed 1) "
          f"ratio {r:.3f}; max|a-b|/max|b| {re:.2e} (< 5e-5: {re < 5e-5})")
    assert r > 1.0, "the per-dof check misses two swapped soft elements"
    assert re < 5e-5, "the whole-vector tolerance was expected to miss it"
