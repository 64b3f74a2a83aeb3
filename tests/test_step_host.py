"""The float64 restatement of the step kernels (tests/step_reference.py) checked on the host: against the numpy oracle,
against its own float32 stand-in on every mesh the device test uses, and against mutants of that stand-in, which the
per-dof comparison must reject.  No GPU.

Every measured ratio is printed ("step-host ..." lines; run with -s to see them)."""
import numpy as np
import pytest

import step_reference as sr
from helpers import load_npz, mesh_problem, orc, rel_err

f32, f64 = np.float32, np.float64
LAM = 0.7


# ---------------------------------------------------------------------------------------------------
# 1. the restatement agrees with the oracle
# ---------------------------------------------------------------------------------------------------
def _oracle_cases():
    rec = load_npz("step_warren_EA.npz")
    yield "warren-nets", mesh_problem(rec, (20, 15, None), (2.0, 0.5, 1.0)), rec["u"].astype(f32), float(rec["lam"])
    c = sr.grid_case(257)
    pb = orc.Problem(nodes=c.nodes, elements=c.elements, loads=c.loads, fixed_dofs=c.fixed, dimension=2, young=3.0, area=0.5,
                     density=1.0, measured_vals=c.meas_vals, measured_dofs=c.meas_dofs)
    yield "grid257-scalar", pb, c.u, LAM


@pytest.mark.parametrize("alpha_p,alpha_d", [(1.0, 100.0), (3.0, 0.0)])
@pytest.mark.parametrize("fe", [0, 1])
def test_restatement_agrees_with_the_oracle(fe, alpha_p, alpha_d):
    """f_int, g_f, grad_u per dof and the loss terms of oracle.loss_and_grads(acc64=True) lie within the per-dof bounds of
    the float64 restatement fed the oracle's own E and A as fields: the oracle is a float32 evaluation of the same
    operations (without fma: 7 roundings in a row where the kernel has 4, still inside degree + 8)."""
    from pinn_fem_amd.plan import build_host_plan
    for name, pb, u, lam in _oracle_cases():
        geo = orc.element_geometry(pb)
        ref = orc.loss_and_grads(pb, geo, u, lam, alpha_p, alpha_d, fe_mode="delta" if fe else "reference", acc64=True)
        mesh = sr.mesh_from_plan(build_host_plan(pb.nodes, pb.elements, pb.loads, pb.fixed_dofs, pb.dimension,
                                                 pb.measured_vals, pb.measured_dofs))
        rec = sr.records(mesh, ref.young, ref.area)
        assert np.array_equal(rec[:, 0], (ref.stiffness * geo.pattern[:, 0, 0]).astype(f32)), "records differ from the oracle's ke"
        f, S = sr.gather64(mesh, rec, u)
        r_f = sr.worst_ratio(ref.f_int - f, sr.gather_bound(mesh, S))
        free = ~mesh.fixed
        g_o = np.zeros(mesh.n_dofs, dtype=f32)
        g_o[free] = (f32(alpha_p) * ref.r).astype(f32)
        _, g = sr.residual64(mesh, f, lam, alpha_p)
        r_g = sr.worst_ratio(g_o - g, sr.residual_bound(mesh, f, S, lam, alpha_p))
        use_data = alpha_d > 0
        gu, gu_b = sr.grad_u64(mesh, rec, g_o, u, use_data, alpha_d)
        r_gu = sr.worst_ratio(ref.grad_u - gu, gu_b)
        lt = sr.loss_terms64(mesh, g_o, u, use_data, alpha_p, alpha_d)
        rel = sr.sum_bound(mesh)
        r_l = max(abs(ref.loss_physics - lt["loss_physics"]) / (rel * lt["loss_physics"]),
                  abs(ref.residual_norm - lt["residual_norm"]) / (rel * lt["residual_norm"]),
                  abs(ref.loss_total - lt["loss_total"]) / sr.total_bound(mesh, lt, use_data, alpha_p, alpha_d))
        if use_data:
            r_l = max(r_l, abs(ref.loss_data - lt["loss_data"]) / (rel * lt["loss_data"]))
        print(f"step-host oracle case={name} fe={fe} alpha_p={alpha_p}: f_int {r_f:.3f} g_f {r_g:.3f} grad_u {r_gu:.3f} losses {r_l:.3f}")
        assert max(r_f, r_g, r_gu, r_l) <= 1.0


def test_internal_force_of_the_oracle():
    """oracle.internal_force on the hub mesh with a decade-wide field, per dof."""
    c = sr.hub_case()
    mesh = c.mesh()
    E, A = sr.fields("decades", mesh.n_elems)
    pb = orc.Problem(nodes=c.nodes, elements=c.elements, loads=c.loads, fixed_dofs=c.fixed, dimension=2, young=1.0, area=1.0,
                     density=1.0)
    geo = orc.element_geometry(pb)
    s = ((E * A).astype(f32) / geo.l0).astype(f32)
    f, S = sr.gather64(mesh, sr.records(mesh, E, A), c.u)
    for fe in ("reference", "delta"):
        r = sr.worst_ratio(orc.internal_force(geo, s, c.u, mesh.n_dofs, fe) - f, sr.gather_bound(mesh, S))
        print(f"step-host oracle internal_force hub600 {fe}: ratio {r:.3f}")
        assert r <= 1.0


# ---------------------------------------------------------------------------------------------------
# 2. the float32 stand-in passes every bound on every mesh
# ---------------------------------------------------------------------------------------------------
def _all_cases():
    for n in sr.SMALL_SIZES:
        yield (lambda n=n: sr.grid_case(n)), "decades"
        yield (lambda n=n: sr.chain_case(n, 1)), "decades"
        yield (lambda n=n: sr.chain_case(n, 2)), "decades"
    for kind in ("decades", "uniform", "softzone"):
        yield sr.hub_case, kind
    yield (lambda: sr.chain_case(513, 2, ramp=True)), "decades"
    yield (lambda: sr.chain_case(sr.LONG_NODES, 1, ramp=True)), "decades"
    yield (lambda: sr.chain_case(sr.LONG_NODES, 2)), "decades"


def test_hub_mesh_has_what_it_is_for():
    c = sr.hub_case()
    mesh = c.mesh()
    deg = mesh.degree
    assert mesh.n_nodes == 600 and deg[c.notes["lonely"]] == 0
    for n, d in c.notes["degrees"].items():
        assert deg[n] == d
    pa, pb = c.notes["twin"]
    twins = [tuple(e) for e in c.elements if set(e) == {pa, pb}]
    assert sorted(twins) == sorted([(pa, pb), (pb, pa)])
    assert sr.terms_per_thread(sr.chain_case(sr.LONG_NODES, 1).mesh()) == 4
    fixed_meas = mesh.fixed & mesh.measured
    assert fixed_meas.any() and np.all(c.u[mesh.fixed] != 0) and np.all(mesh.f_ext[mesh.fixed] != 0)


def test_standin_passes_every_bound_on_every_mesh():
    worst = {}
    for make, kind in _all_cases():
        c = make()
        for with_meas, alpha_p, alpha_d in ((True, 1.0, 100.0), (True, 3.0, 0.0), (False, 1.0, 100.0)):
            if c.nodes.shape[0] > 10_000 and not (with_meas and alpha_p == 1.0):
                continue
            mesh = c.mesh(with_meas)
            rec = sr.records(mesh, *sr.fields(kind, mesh.n_elems))
            for fe in (0, 1):
                use_data = with_meas and alpha_d > 0
                rr = sr.standin_ratios(mesh, rec, c.u, LAM, alpha_p, alpha_d, use_data, fe)
                print(f"step-host standin case={c.name} field={kind} meas={int(with_meas)} alpha_p={alpha_p} alpha_d={alpha_d} fe={fe}: "
                      + " ".join(f"{k} {v:.3f}" for k, v in rr.items()))
                for k, v in rr.items():
                    worst[k] = max(worst.get(k, 0.0), v)
                    assert v <= 1.0, (c.name, kind, fe, k, v)
    print("step-host standin worst ratio per quantity: " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))


# ---------------------------------------------------------------------------------------------------
# 3. the comparison can fail: mutants of the stand-in
# ---------------------------------------------------------------------------------------------------
MUTANTS = ("swap", "next-record", "negate-end", "cs-for-s2", "drop-last-odd", "fixed-leak", "data-without-use_data")


def _rows64(mesh, rec, v, rec_of=None, s2_as_cs=False):
    """The rows of every incidence in float64, optionally reading another element's record / cs for s2."""
    k = rec.astype(f64)[mesh.inc_elem if rec_of is None else rec_of]
    vi, vj = sr._ends(mesh, v, f64)
    sg = np.where(mesh.inc_end == 1, -1.0, 1.0)
    s2 = k[:, 1] if s2_as_cs else k[:, 2]
    return np.stack([sg * (k[:, 0] * (vi[:, 0] - vj[:, 0]) + k[:, 1] * (vi[:, 1] - vj[:, 1])),
                     sg * (k[:, 1] * (vi[:, 0] - vj[:, 0]) + s2 * (vi[:, 1] - vj[:, 1]))], axis=1)


def _pick(effect, bound4, allowed, prefer=None):
    """The incidence (row of `effect`, [n, dim]) where a mutant goes: its effect exceeds four times the bound at a dof of
    its node; among those the preferred ones first, and of them the one with the SMALLEST effect (the best hidden one).
    None where no such place exists."""
    ok = np.any(effect > bound4, axis=1) & allowed
    if not ok.any():
        return None, False
    pref = ok & prefer if prefer is not None and (ok & prefer).any() else ok
    idx = np.flatnonzero(pref)
    return int(idx[np.argmin(np.max(effect[idx], axis=1))]), prefer is not None and bool((ok & prefer).any())


def _mutation_cases():
    for n in sr.SMALL_SIZES:
        yield f"grid{n}", (lambda n=n: sr.grid_case(n)), "decades"
        yield f"chain2d{n}", (lambda n=n: sr.chain_case(n, 2)), "decades"
    yield "hub600", sr.hub_case, "decades"
    yield "hub600-softzone", sr.hub_case, "softzone"
    yield "grid513-softzone", (lambda: sr.grid_case(513)), "softzone"
    yield "chain2d-long", (lambda: sr.chain_case(sr.LONG_NODES, 2)), "decades"


def _possible(mesh):
    """Which mutants the mesh has a place for at all (a one-element mesh has no two elements at a node, a mesh whose nodes
    all have even degree has no odd one): structure only, no magnitudes."""
    deg = mesh.degree
    return {"swap": bool(np.any(deg >= 2)), "next-record": mesh.n_elems >= 2, "negate-end": True, "cs-for-s2": True,
            "drop-last-odd": bool(np.any(deg % 2 == 1)), "fixed-leak": bool(mesh.fixed.any()),
            "data-without-use_data": bool(mesh.measured.any())}


@pytest.mark.parametrize("label", [c[0] for c in _mutation_cases()])
def test_every_mutant_is_rejected(label):
    _, make, kind = next(c for c in _mutation_cases() if c[0] == label)
    c = make()
    mesh = c.mesh()
    E, A = sr.fields(kind, mesh.n_elems)
    rec = sr.records(mesh, E, A)
    u = c.u
    f, S = sr.gather64(mesh, rec, u)
    Bf = sr.gather_bound(mesh, S)
    s = (E.astype(f64) * A.astype(f64)) / mesh.egeo[:, 3]
    soft = s <= np.quantile(s, 0.1)                       # the softest tenth of the field
    own = _rows64(mesh, rec, u)
    B4 = 4.0 * Bf.reshape(mesh.n_nodes, 2)[mesh.inc_node]
    n_inc = mesh.inc_elem.size
    everywhere = np.ones(n_inc, dtype=bool)
    possible = _possible(mesh)
    fmax = np.max(np.abs(f))
    assert sr.worst_ratio(sr.gather32(mesh, rec, u) - f, Bf) <= 1.0       # the unmutated stand-in passes

    def report(name, place, both_soft, got, ref, bound):
        ratio = sr.worst_ratio(got - ref, bound)
        hidden = rel_err(got, ref) < 5e-5
        print(f"step-host mutant case={label} mutant={name} place={place} soft={int(both_soft)}: per-dof ratio {ratio:.3g} "
              f"-> {'rejected' if ratio > 1 else 'PASSED'}; rel_err < 5e-5 would have {'passed' if hidden else 'rejected'} it")
        assert ratio > 1.0, f"mutant {name} survives the per-dof check"
        return hidden

    for name in MUTANTS:
        inc = sr.incidences(mesh)
        if not possible[name]:
            print(f"step-host mutant case={label} mutant={name}: the mesh has no place for it (structure)")
            assert mesh.n_nodes <= 3, f"{label} should have a place for {name}"
            continue
        if name == "swap":
            same = np.zeros(n_inc, dtype=bool)
            same[:-1] = mesh.inc_node[:-1] == mesh.inc_node[1:]
            nxt = np.roll(mesh.inc_elem, -1)
            alt_a = _rows64(mesh, rec, u, rec_of=nxt)                       # incidence idx reading idx + 1's record
            alt_b = _rows64(mesh, rec, u, rec_of=np.roll(mesh.inc_elem, 1))  # incidence idx reading idx - 1's record
            eff = np.abs((alt_a - own) + np.roll(alt_b - own, -1, axis=0))
            place, both = _pick(eff, B4, same, soft[mesh.inc_elem] & soft[nxt])
            if place is not None and not both:
                place, _ = _pick(eff, B4, same & (soft[mesh.inc_elem] | soft[nxt]))
            assert place is not None, "no node where swapping two elements' stiffness shows above 4x the bound"
            inc.rec_of[place], inc.rec_of[place + 1] = mesh.inc_elem[place + 1], mesh.inc_elem[place]
        elif name == "next-record":
            nxt = (mesh.inc_elem + 1) % mesh.n_elems
            eff = np.abs(_rows64(mesh, rec, u, rec_of=nxt) - own)
            place, both = _pick(eff, B4, soft[mesh.inc_elem], soft[nxt])
            assert place is not None, "no soft element whose neighbour's record shows above 4x the bound"
            inc.rec_of[place] = nxt[place]
        elif name == "negate-end":
            place, both = _pick(2.0 * np.abs(own), B4, everywhere)
            assert place is not None
            inc.sign[place] = -1.0
        elif name == "cs-for-s2":
            place, both = _pick(np.abs(_rows64(mesh, rec, u, s2_as_cs=True) - own), B4, everywhere)
            assert place is not None
            inc.s2_as_cs[place] = True
        elif name == "drop-last-odd":
            last = np.zeros(n_inc, dtype=bool)
            odd = np.flatnonzero(mesh.degree % 2 == 1)
            last[mesh.adj_ptr[odd + 1] - 1] = True
            place, both = _pick(np.abs(own), B4, last)
            assert place is not None
            inc.keep[place] = False
        if name in MUTANTS[:5]:
            hidden = report(name, place, both, sr.gather32(mesh, rec, u, 0, inc), f, Bf)
            if kind == "softzone" and name in ("swap", "next-record") and both:
                assert hidden, "a soft-zone mutant the whole-vector tolerance was expected to miss"
            continue
        f32_ = sr.gather32(mesh, rec, u)
        if name == "fixed-leak":
            r64, g64 = sr.residual64(mesh, f, LAM, 1.0)
            leak = np.abs(f - f64(f32(LAM)) * mesh.f_ext)
            cand = np.flatnonzero(mesh.fixed & (leak > 4.0 * Bf))
            assert cand.size, "no fixed dof with a residual to leak"
            place = int(cand[np.argmin(leak[cand])])
            _, g32 = sr.residual32(mesh, f32_, LAM, 1.0, leak_fixed=place)
            report(name, place, False, g32, g64, sr.residual_bound(mesh, f, S, LAM, 1.0))
        else:
            _, g32 = sr.residual32(mesh, f32_, LAM, 1.0)
            gu, gu_b = sr.grad_u64(mesh, rec, g32, u, False, 0.0)
            term = np.abs(sr.data_term64(mesh, u, True, 100.0))
            cand = np.flatnonzero(mesh.measured & (term > 4.0 * gu_b))
            assert cand.size, "no measured dof whose data term shows above 4x the bound"
            place = int(cand[np.argmin(term[cand])])
            got = sr.grad_u32(mesh, rec, g32, u, False, 100.0, force_data_on=place)
            report(name, place, False, got, gu, gu_b)
