#!/usr/bin/env python3
"""The bits of the numpy / scipy restatements of the Green-Lagrange family (tests/*_reference.py) on fixed seeded inputs.

    reference_bits.py [--save FILE.npz] [--against FILE.npz]

One line per call: case, call, variant, sha256 of the raw output bytes; Levenberg-Marquardt runs also print their
evaluation count, stop and accepted / damping sequences in clear.  Two versions of the restatements compute the same bits
exactly when this file prints the same lines for both (profiles/r16_reference_bits.txt).  --save keeps every hashed array;
--against prints, for every array whose bytes differ from a saved run, the largest entry-by-entry difference relative to
the entry in units of 2^-53 and the largest absolute difference.  CPU only: no torch, no engine.

Covered: the element functions at E*A scalar and per element, the initial strain absent, scalar and per element, in 1-D and
2-D; the Newton loop on the closed-form structures; the misfit with its gradient, the residuals with their Jacobian (also
without the Jacobian and at given states) and the Levenberg-Marquardt run of every case the tests share, each with the
direct solve and with Jacobi-preconditioned CG; both covariance forms."""
import argparse, hashlib, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gl_reference as gl
import gl_e0_reference as g0
import identify_reference as ir
import identify_strain_reference as sr
import identify_prestress_reference as pr

SAVED = {}


# ---- the call spellings: the only part that follows the modules ---------------------------------------------------------
def element_state(nodes, el, u, ea, e0, dim):
    return gl.element_state(nodes, el, u, ea, dim, e0=e0)


def f_int(nodes, el, u, ea, e0, dim):
    return gl.f_int(nodes, el, u, ea, dim, e0=e0)


def f_int_scale(nodes, el, u, ea, e0, dim):
    return gl.f_int_scale(nodes, el, u, ea, dim, e0=e0)


def k_t(nodes, el, u, ea, e0, dim):
    return gl.k_t(nodes, el, u, ea, dim, e0=e0)


def energy(nodes, el, u, ea, e0, dim):
    return gl.energy(nodes, el, u, ea, dim, e0=e0)


def axial_forces(nodes, el, u, ea, e0, dim):
    return gl.axial_forces(nodes, el, u, ea, dim, e0=e0)


def element_sensitivity(nodes, el, u, a, e0, dim):
    return gl.element_sensitivity(nodes, el, u, a, dim, e0=e0)


def sensitivity_scale(nodes, el, u, a, e0, dim):
    return gl.sensitivity_scale(nodes, el, u, a, dim, e0=e0)


def newton(nodes, el, loads, fixed, ea, e0, dim, **kw):
    return gl.newton(nodes, el, loads, fixed, ea, dim, e0=e0, **kw)


def incremental(nodes, el, loads, fixed, ea, dim, n_inc):
    return gl.incremental(nodes, el, loads, fixed, ea, dim, n_inc)


def group_rhs(nodes, el, u, ea, dim, groups, n_groups, fixed):
    return gl.group_rhs(nodes, el, u, ea, dim, groups, n_groups, fixed)


prestress_rhs, prestress_rhs_scale = gl.prestress_rhs, gl.prestress_rhs_scale
strains, bt_c, bt_c_scale, b_v, b_v_scale = gl.strains, gl.bt_c, gl.bt_c_scale, gl.b_v, gl.b_v_scale
TautString, cable_chain, heated_bar = g0.TautString, g0.cable_chain, g0.heated_bar


def misfit_and_gradient(kind, case, ea, e0, **kw):
    return ir.misfit_and_gradient(case.nodes, case.el, case.loads, case.fixed, ea, 2, case.levels, case.gauges, e0, **kw)


def residuals_and_jacobian(kind, case, q, t, e0, **kw):
    return ir.case_residuals(case, q, e0=e0, t=t, **kw)


def levenberg_marquardt(kind, case, e0, **kw):
    return ir.identify_prestress(case, **kw) if kind == "prestress" else ir.identify_factors(case, e0=e0, **kw)


def cases():
    """(label, kind, case, e0 of the model, arguments of the run the tests share)."""
    sharp = dict(misfit_tolerance=1e-15)
    yield "ir.warren_case(8)", "gn", ir.warren_case(8), None, sharp
    yield "gn.case_with_groups(8)", "gn", ir.case_with_groups(8), None, sharp
    yield "gn.noisy_case()", "gn", ir.noisy_case(), None, {}
    case = g0.warren_case()
    yield "g0.warren_case() with e0", "e0", case, case.e0, sharp
    yield "g0.warren_case() e0 left out", "e0", case, 0.0, sharp
    for G in (4, 8):
        for tip in (False, True):
            yield f"sr.strain_case({G}, tip={tip})", "strain", sr.strain_case(G, tip=tip), None, sharp
    for name in pr.CASES:
        yield f"pr.CASES[{name}]", "prestress", pr.CASES[name](), None, sharp
    yield "pr.noisy_case()", "prestress", pr.noisy_case(), None, {}
    yield ("pr.cable_case() with refused trials", "prestress", pr.cable_case(), None,
           dict(t0=np.array([-3e-2]), damping=1e-9, misfit_tolerance=1e-15))


# ---- the fixed part ------------------------------------------------------------------------------------------------------
def show(case, call, variant, *arrays, clear=""):
    h = hashlib.sha256()
    for k, a in enumerate(arrays):
        a = np.ascontiguousarray(a.toarray() if hasattr(a, "toarray") else a, dtype=np.float64)
        h.update(a.tobytes())
        SAVED[f"{case} {call} [{variant}] {k}"] = a
    print(f"{case} {call} [{variant}] {h.hexdigest()}{clear}", flush=True)


def element_lines(name, nodes, el, u, dim, rng):
    ne, n = len(el), len(u)
    a, coef = rng.standard_normal(n), rng.standard_normal(ne)
    groups = rng.integers(0, 3, ne)
    pgroups = np.where(rng.random(ne) < 0.2, -1, groups)
    picks = rng.permutation(ne)[: max(1, ne // 3)]
    fixed = np.array([0, n - 1])
    for ea_tag, ea in (("ea scalar", 750.0), ("ea per element", np.exp2(rng.uniform(-3.0, 3.0, ne)))):
        for e0_tag, e0 in (("e0 absent", None), ("e0 scalar", -2e-3), ("e0 per element", 1e-3 * rng.standard_normal(ne))):
            tag = f"{ea_tag}, {e0_tag}"
            strain, fe, B, t = element_state(nodes, el, u, ea, e0, dim)
            show(name, "element_state", tag, strain, fe, B, t["n"])
            show(name, "f_int", tag, f_int(nodes, el, u, ea, e0, dim))
            show(name, "f_int_scale", tag, f_int_scale(nodes, el, u, ea, e0, dim))
            show(name, "k_t", tag, k_t(nodes, el, u, ea, e0, dim))
            show(name, "energy", tag, np.float64(energy(nodes, el, u, ea, e0, dim)))
            show(name, "axial_forces", tag, axial_forces(nodes, el, u, ea, e0, dim))
        show(name, "f_int", f"{ea_tag}, absolute", gl.f_int(nodes, el, u, ea, dim, absolute=True))
        show(name, "k_t", f"{ea_tag}, absolute", gl.k_t(nodes, el, u, ea, dim, absolute=True))
        show(name, "group_rhs", ea_tag, group_rhs(nodes, el, u, ea, dim, groups, 3, fixed))
        for map_tag, pg in (("", groups), (", map with -1", pgroups)):
            show(name, "prestress_rhs", ea_tag + map_tag, prestress_rhs(nodes, el, u, ea, pg, 3, dim))
            show(name, "prestress_rhs_scale", ea_tag + map_tag, prestress_rhs_scale(nodes, el, u, ea, pg, 3, dim))
    for e0_tag, e0 in (("e0 absent", None), ("e0 scalar", -2e-3), ("e0 per element", 1e-3 * rng.standard_normal(ne))):
        show(name, "element_sensitivity", e0_tag, element_sensitivity(nodes, el, u, a, e0, dim))
        show(name, "sensitivity_scale", e0_tag, sensitivity_scale(nodes, el, u, a, e0, dim))
    show(name, "strains", "", strains(nodes, el, u, dim))
    show(name, "bt_c", "", bt_c(nodes, el, u, coef, dim))
    show(name, "bt_c_scale", "", bt_c_scale(nodes, el, u, coef, dim))
    show(name, "b_v", "", b_v(nodes, el, u, picks, a, dim))
    show(name, "b_v_scale", "", b_v_scale(nodes, el, u, picks, a, dim))


def newton_lines():
    tb = gl.TwoBar(a=10.0, h=1.0, ea=1000.0)
    ts = TautString()
    cn, cel, cloads, cfixed = cable_chain(16)
    runs = (("TwoBar half limit load", tb.nodes, tb.el, tb.loads(0.5 * tb.p_lim), tb.fixed, tb.ea, None),
            ("TautString", ts.nodes, ts.el, ts.loads(ts.load(0.05)), ts.fixed, ts.ea, ts.e0),
            ("cable_chain(16)", cn, cel, cloads, cfixed, 1000.0, -1e-2))
    for name, nodes, el, loads, fixed, ea, e0 in runs:
        for tag, kw in (("direct", {}), ("jacobi_cg", dict(linear_solve=gl.jacobi_cg(1e-13)))):
            u, it, ok = newton(nodes, el, loads, fixed, ea, e0, 2, **kw)
            show(name, "newton", tag, u, clear=f" iterations {it} converged {ok}")
    u, its = incremental(tb.nodes, tb.el, tb.loads(0.9 * tb.p_lim), tb.fixed, tb.ea, 2, 4)
    show("TwoBar 0.9 limit load", "incremental", "4 increments", u, clear=f" iterations {its}")


def identification_lines():
    for label, kind, case, e0, run_kw in cases():
        rng = np.random.default_rng(len(label))
        n_q = case.n_q if kind == "prestress" else case.n_groups
        q = 0.1 * rng.standard_normal(n_q)
        t = case.t0 + 1e-4 * rng.standard_normal(case.n_t) if kind == "prestress" else None
        for tag, kw in (("direct", {}), ("jacobi_cg", dict(linear_solve=gl.jacobi_cg(1e-13)))):
            if kind != "prestress":
                J, grad, us, its = misfit_and_gradient(kind, case, case.ea(q), e0, **kw)
                show(label, "misfit_and_gradient", tag, np.float64(J), grad, *us, clear=f" iterations {its}")
            rho, A, us, its = residuals_and_jacobian(kind, case, q, t, e0, **kw)
            show(label, "residuals_and_jacobian.rho", tag, rho, clear=f" iterations {its}")
            show(label, "residuals_and_jacobian.A", tag, A)
            show(label, "residuals_and_jacobian.states", tag, *us)
            rho_only, none, _, _ = residuals_and_jacobian(kind, case, q, t, e0, jacobian=False, **kw)
            assert none is None
            show(label, "residuals_and_jacobian.rho", tag + ", jacobian=False", rho_only)
            rho_s, A_s, _, its_s = residuals_and_jacobian(kind, case, q, t, e0, states=us, **kw)
            assert its_s == []
            show(label, "residuals_and_jacobian.rho", tag + ", states given", rho_s)
            show(label, "residuals_and_jacobian.A", tag + ", states given", A_s)
            run = levenberg_marquardt(kind, case, e0, **run_kw, **kw)
            seq = " ".join(f"{'a' if h['accepted'] else 'r'}{h['damping']:.0e}" for h in run["history"])
            show(label, "levenberg_marquardt.q", tag, run["q"], *([run["t"]] if "t" in run else []),
                 clear=f" evaluations {run['evaluations']} stop {run['stop']} steps {seq}")
            show(label, "levenberg_marquardt.rho", tag, run["rho"], np.float64(run["misfit"]), run["factors"])
            show(label, "levenberg_marquardt.jacobian", tag, run["jacobian"])
            show(label, "levenberg_marquardt.states", tag, *run["states"])
            show(label, "levenberg_marquardt.history", tag, np.array([np.nan if h["misfit"] is None else h["misfit"]
                                                                      for h in run["history"]]))
        show(label, "gn.covariance", "", ir.covariance(A, float(rho @ rho)))
        show(label, "pr.covariance", "", pr.covariance(A, float(rho @ rho)))


def against(path):
    old = np.load(path)
    print(f"# arrays that differ from {os.path.basename(path)}: worst |new - old| / |old| in units of 2^-53, worst |new - old|")
    for key, new in SAVED.items():
        if key not in old.files:
            print(f"# {key}: not in the saved run")
        elif old[key].shape != new.shape:
            print(f"# {key}: shape {old[key].shape} -> {new.shape}")
        elif old[key].tobytes() != new.tobytes():
            diff = np.abs(new - old[key])
            with np.errstate(divide="ignore", invalid="ignore"):
                rel = np.where(diff > 0.0, diff / np.abs(old[key]), 0.0)
            print(f"# {key}: {np.max(rel) / 2.0 ** -53:.3g} units, {np.max(diff):.3g}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--save")
    ap.add_argument("--against")
    args = ap.parse_args()
    rng = np.random.default_rng(257)
    nodes, el = gl.irregular_truss(257, rng)
    l0 = np.linalg.norm(nodes[el[:, 1]] - nodes[el[:, 0]], axis=1).mean()
    element_lines("irregular_truss(257)", nodes, el, 0.15 * l0 * rng.standard_normal(nodes.size), 2, rng)
    x, el1, _ = heated_bar(5)
    element_lines("chain(5)", x, el1, 0.15 * 0.75 * rng.standard_normal(len(x)), 1, rng)
    newton_lines()
    identification_lines()
    if args.save:
        np.savez(args.save, **SAVED)
    if args.against:
        against(args.against)


if __name__ == "__main__":
    main()
