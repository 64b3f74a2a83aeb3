#!/usr/bin/env python3
"""The bits of every Green-Lagrange kernel of pf_nl.hip (and of kt_diag and one tangent CG solve) on fixed seeded inputs, the
explicit step and its energies last, after every other line (bars, then tension-only elements; --bars leaves the tension-only
lines out, for a build from before they existed), and behind them the step under load and support-motion histories
(--no-history leaves those out, for a build from before they existed).

    gl_kernel_bits.py [--bars] [--no-history]

One line per engine call: mesh, call, variant, sha256 of the raw output bytes.  Two builds of the library compute the same
bits exactly when a run of this file in a fresh process prints the same lines for both (profiles/r14_gl_once_compare.txt).

Meshes, the smallest that reach every branch: Warren girders of 1 and of 130 panels (261 nodes and 519 elements: one past a
256-thread block in both; node degrees 2, 3 and 4, so a last odd incidence occurs) and 1-D chains of 1 and 257 elements.
Variants: ea and e0 absent and given, accumulate 0 and 1, g0 > 0 with m below the group count, a prestress map that holds
-1 (not on the one-element chain, whose only element must stay in a group), and |du| / l0 of about 0.3 and about 1e-9."""
import hashlib, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("PINNFEM_QUIET", "1")
from pinn_fem_amd.engine import HipEngine
from pinn_fem_amd.fem.model import FEMModel, Material
from pinn_fem_amd.plan import warren_mesh
import torch

N_GROUPS = 5


def meshes():
    for panels in (1, 130):
        nodes, el, loads, fixed, _, _ = warren_mesh(panels)
        yield f"warren_{panels}", FEMModel(nodes=nodes, elements=el, material=Material(2.0, 0.5, 1.0), loads=loads,
                                           fixed_dofs=fixed, dimension=2)
    for n in (1, 257):
        x = np.concatenate([[0.0], np.cumsum(np.random.default_rng(n).uniform(0.5, 1.5, n))])
        el = np.stack([np.arange(n), np.arange(1, n + 1)], axis=1)
        loads = np.zeros(n + 1)
        loads[-1] = 1.0
        yield f"chain_{n}", FEMModel(nodes=x, elements=el, material=Material(2.0, 0.5, 1.0), loads=loads,
                                     fixed_dofs=np.array([0]), dimension=1)


def main():
    late = []                                   # the explicit dynamics' lines: printed after every mesh's other lines
    last = []                                   # the time histories' lines: printed after those
    for name, model in meshes():
        eng = HipEngine(model)
        ne, n = eng.plan.n_elems, eng.plan.n_dofs
        rng = np.random.default_rng(ne)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(eng.device)

        def show(call, variant, t, out=None):
            torch.cuda.synchronize()
            line = f"{name} {call} [{variant}] {hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()}"
            print(line, flush=True) if out is None else out.append(line)

        ea, e0 = dev(np.exp2(rng.uniform(-3.0, 3.0, ne))), dev(1e-3 * rng.standard_normal(ne))
        a, coef = dev(rng.standard_normal(n)), dev(rng.standard_normal(ne))
        V = dev(rng.standard_normal((3, n)))
        groups = rng.integers(0, N_GROUPS, ne)
        pg = groups.copy()
        if ne > 1:
            pg[rng.permutation(ne)[: max(1, ne // 7)]] = -1
        gauges = rng.permutation(ne)[: max(1, ne // 3)]
        field = rng.standard_normal(n)
        for size, amplitude in (("0.3", 0.15), ("1e-9", 5e-10)):
            u = dev(amplitude * field)
            for variant, kw in (("", {}), ("ea", dict(ea=ea)), ("e0", dict(e0=e0)), ("ea e0", dict(ea=ea, e0=e0))):
                tag = f"du {size} {variant}".strip()
                show("gl_state.strain", tag, eng.gl_state(u, **kw))
                show("gl_state.fe", tag, eng._gl[2])
                show("gl_state.kt", tag, eng._gl[1])
                show("gl_fint", tag, eng.gl_fint())
                show("kt_diag", tag, eng.kt_diag())
                show("gl_group_rhs", tag, eng.gl_group_rhs(groups))
                show("gl_group_rhs", tag + " g0 1 m 2", eng.gl_group_rhs(groups, g0=1, m=2))
            for variant, z in (("", None), ("e0", e0)):
                tag = f"du {size} {variant}".strip()
                s = eng.gl_sensitivity(u, a, e0=z)
                show("gl_sensitivity", tag, s)
                show("gl_sensitivity", tag + " accumulate", eng.gl_sensitivity(u, a, out=s, e0=z))
            show("group_sum", f"du {size} weights", eng.group_sum(eng.gl_sensitivity(u, a), ea, groups))
            show("group_sum", f"du {size}", eng.group_sum(eng.gl_sensitivity(u, a), None, groups))
            for variant, ee in (("", None), ("ea", ea)):
                tag = f"du {size} {variant}".strip()
                show("gl_prestress_rhs", tag, eng.gl_prestress_rhs(u, ee, groups))
                show("gl_prestress_rhs", tag + " map with -1", eng.gl_prestress_rhs(u, ee, pg))
                show("gl_prestress_rhs", tag + " map with -1 g0 1 m 2", eng.gl_prestress_rhs(u, ee, pg, g0=1, m=2))
            r = eng.gl_strain_rhs(u, coef)
            show("gl_strain_rhs", f"du {size}", r)
            show("gl_strain_rhs", f"du {size} accumulate", eng.gl_strain_rhs(u, coef, out=r))
            show("gl_strain_jvp", f"du {size}", eng.gl_strain_jvp(u, gauges, V))
        eng.gl_state(u, ea, e0)                 # the small field: the tangent is positive definite there
        x = eng.pcg_solve(eng.gl_group_rhs(groups)[0] + dev(model.loads).reshape(-1), tangent=True, u=u)[0]
        show("pcg_solve", "tangent, du 1e-9 ea e0", x)
        # the explicit step and its energies, bars and then tension-only elements (every third element flagged); 33 steps
        # from the large field, the half kick first, eager and as a graph
        minv, v0 = dev(np.exp2(rng.uniform(-1.0, 1.0, n))), dev(0.1 * rng.standard_normal(n))
        cable = np.arange(ne) % 3 == 0
        u_large = dev(0.15 * field)
        for tag, more in (("", {}), ("cable", dict(cable=cable)))[: 1 if "--bars" in sys.argv[1:] else 2]:
            for variant, kw in (("", {}), ("ea e0", dict(ea=ea, e0=e0))):
                for graph in (False, True):
                    eng.dyn_begin(u_large, v0, minv, 1e-3, 0.5, 0.25, 1.5, 0.02, start=True, **kw, **more)
                    eng.dyn_steps(32, use_graph=graph)
                    label = " ".join(x for x in (tag, variant, "graph" if graph else "eager") if x)
                    uu, vv, _ = eng.dyn_state()
                    show("dyn_steps.u", label, uu, late)
                    show("dyn_steps.v", label, vv, late)
                show("dyn_energy", " ".join(x for x in (tag, variant) if x), torch.tensor(eng.dyn_energy(), dtype=torch.float64), late)
                if more:
                    late.append(f"{name} dyn_slack_count [{' '.join(x for x in (tag, variant) if x)}] {eng.dyn_slack_count()}")
        if "--no-history" in sys.argv[1:] or "--bars" in sys.argv[1:]:
            continue
        # the same 33 steps under seeded histories of 20 samples (the last steps hold the last one): a load history, a
        # support history (amplitudes on every other fixed dof), both; bars and tension-only elements, eager and as a graph
        lam, sup = rng.uniform(0.25, 1.5, 20), rng.standard_normal(20)
        amp = np.zeros(n)
        amp[np.asarray(model.fixed_dofs, dtype=np.int64)[::2]] = 0.01
        for tag, more in (("", {}), ("cable", dict(cable=cable))):
            for variant, hist in (("load", dict(load_samples=lam)), ("support", dict(support=(amp, sup))),
                                  ("load support", dict(load_samples=lam, support=(amp, sup)))):
                for graph in (False, True):
                    eng.dyn_begin(u_large, v0, minv, 1e-3, 0.5, 0.25, 1.5, 0.02, ea=ea, e0=e0, start=True, **hist, **more)
                    eng.dyn_steps(32, use_graph=graph)
                    label = " ".join(x for x in (tag, "history", variant, "graph" if graph else "eager") if x)
                    uu, vv, _ = eng.dyn_state()
                    show("dyn_steps.u", label, uu, last)
                    show("dyn_steps.v", label, vv, last)
    print("\n".join(late + last), flush=True)


if __name__ == "__main__":
    main()
