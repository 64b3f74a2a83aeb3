#!/usr/bin/env python3
"""Microseconds per explicit time step of a Green-Lagrange truss: the fused step (pf_gl_dyn_steps, one launch per step)
against the composition the entry points before it allow (pf_gl_state_e0, pf_gl_fint and a torch update: six launches and
two round trips through fe per step), each issued launch by launch ("eager") and as a replayed hipGraph.

    dyn_scale.py [--steps 200] [--rounds 5] [--chains 1000 100000 1000000] [--warren 250 25000 250000] [--cable | --history]

Meshes: collinear chains (plan.chain_mesh: only ux is free) and Warren girders (plan.warren_mesh), every element with the
pretension e0 = -1e-3, E*A = 1000, rho A = 0.5, the mesh's own loads scaled to 1e-3, alpha = 0.1, dt = half the bound at
rest.  Both paths advance the same scheme from rest; the composition's update is four in-place torch kernels on precomputed
vectors (r = lam F - f_int; v *= c1; v += r * (g minv) on the free dofs; u += dt v), the fewest this formulation needs.  Its
eager form pays one Python call per launch, as a caller of those entry points would; the graph forms carry no host work.
After a warm-up of every variant, `rounds` rounds time `steps` steps of each variant between two events, the variants
alternated inside a round.  One JSON line per mesh: median, minimum and maximum microseconds per step of each variant, the
ratios of the medians, and the largest difference between the two paths' displacements after the first `steps` steps.

--cable times the tension-only step (pf_gl_dyn_steps_cable) against the bar step instead, on the same meshes, loads and dt,
eager and as a graph, three runs alternated in the same way: bar (no flags), taut (every element flagged with the pretension
e0 = -1e-3: the chains end the run without a slack element; the girders shorten, swing through and end with about half
their elements slack) and half (every element flagged, e0 = +1e-3 on the odd elements, which are slack from the first step
on).  The JSON line holds the slack counts at the end and the ratios of the medians to the bar's.  The rule is a select,
so a step does the same work whatever is slack.

--history times the step under time histories (pf_gl_dyn_steps_hist) against the bar step, on the same meshes, loads and dt,
eager and as a graph, four runs alternated in the same way: bar (no history), load (a load history around 1), support (every
fixed dof moved by 1e-4 times a history; the load factor is the bar's) and both.  The histories hold a sample for every step
the run takes.  The JSON line holds the ratios of the medians to the bar's."""
import argparse, ctypes as C, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("PINNFEM_QUIET", "1")
from pinn_fem_amd import _capi
from pinn_fem_amd.engine import HipEngine
from pinn_fem_amd.fem.dynamics import lumped_mass, omega_bound
from pinn_fem_amd.fem.model import FEMModel, Material
from pinn_fem_amd.plan import chain_mesh, warren_mesh
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--chains", type=int, nargs="*", default=[1000, 100_000, 1_000_000])
ap.add_argument("--warren", type=int, nargs="*", default=[250, 25_000, 250_000])
ap.add_argument("--cable", action="store_true")
ap.add_argument("--history", action="store_true")
args = ap.parse_args()
E0, ALPHA = -1e-3, 0.1


def measure(name, mesh):
    nodes, el, loads, fixed = mesh[:4]
    model = FEMModel(nodes=nodes, elements=el, material=Material(2000.0, 0.5, 1.0), loads=1e-3 * loads, fixed_dofs=fixed,
                     dimension=2)
    eng = HipEngine(model)
    dev, nd, ne, K = eng.device, model.ndof, model.nelm, args.steps
    mass = lumped_mass(model)
    e0_np = np.full(ne, E0)
    dt = 0.5 * 2.0 / omega_bound(model, np.zeros(ne), e0_np, mass)
    f64 = dict(dtype=torch.float64, device=dev)
    free = torch.ones(nd, **f64)
    free[torch.from_numpy(np.asarray(fixed, dtype=np.int64)).to(dev)] = 0.0
    minv = torch.from_numpy(np.repeat(1.0 / mass, 2)).to(dev)
    e0, zero = torch.from_numpy(e0_np).to(dev), torch.zeros(nd, **f64)
    h = 0.5 * ALPHA * dt
    c1, g = (1.0 - h) / (1.0 + h), dt / (1.0 + h)

    # the composition, on buffers of its own
    u, v, r, f_int = (torch.zeros(nd, **f64) for _ in range(4))
    lam_f = torch.from_numpy(np.asarray(model.loads, dtype=np.float64)).to(dev)
    gm = g * minv * free
    rec = eng._gl_buffers()[4]

    def composed_step():
        s = eng._stream()
        _capi.check(eng.lib.pf_gl_state_e0(eng._ref(), C.byref(rec), None, e0.data_ptr(), u.data_ptr(), s), "pf_gl_state_e0")
        _capi.check(eng.lib.pf_gl_fint(eng._ref(), C.byref(rec), f_int.data_ptr(), s), "pf_gl_fint")
        torch.sub(lam_f, f_int, out=r)
        v.mul_(c1)
        v.addcmul_(r, gm)
        u.add_(v, alpha=dt)

    def composed_eager():
        with eng.on_stream():
            for _ in range(K):
                composed_step()

    graph = torch.cuda.CUDAGraph()

    def composed_capture():
        with eng.on_stream():
            composed_step()                         # torch's lazy set-up happens outside the capture
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=eng.stream):
            for _ in range(K):
                composed_step()

    def composed_graph():
        with eng.on_stream():
            graph.replay()

    def reset():
        u.zero_(); v.zero_()
        eng.dyn_begin(zero, zero, minv, dt, ALPHA, 1.0, 1.0, 0.0, None, e0, start=False)

    variants = {"fused_eager": lambda: eng.dyn_steps(K, use_graph=False), "fused_graph": lambda: eng.dyn_steps(K, use_graph=True),
                "composed_eager": composed_eager, "composed_graph": composed_graph}
    # the two paths compute the same thing: K steps of each from rest
    reset()
    eng.dyn_steps(K, use_graph=False)
    composed_eager()
    torch.cuda.synchronize()
    difference = float((eng.dyn_state()[0] - u).abs().max())
    size = float(u.abs().max())
    composed_capture()
    reset()
    for fn in variants.values():                    # warm-up: every variant once (the fused graph is captured here)
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with eng.on_stream():
                a.record(eng.stream)
            fn()
            with eng.on_stream():
                b.record(eng.stream)
            torch.cuda.synchronize()
            times[k].append(1e3 * a.elapsed_time(b) / K)
    assert bool(torch.isfinite(u).all()) and bool(torch.isfinite(eng.dyn_state()[0]).all())
    row = {"mesh": name, "nodes": model.nnode, "elements": ne, "steps_per_region": K, "rounds": args.rounds, "dt": dt,
           "max_abs_u": size, "max_difference_of_the_paths": difference}
    for k, t in times.items():
        row[k + "_us"] = {"median": float(np.median(t)), "min": float(np.min(t)), "max": float(np.max(t))}
    med = lambda k: row[k + "_us"]["median"]
    row["composed_over_fused_eager"] = med("composed_eager") / med("fused_eager")
    row["composed_over_fused_graph"] = med("composed_graph") / med("fused_graph")
    print(json.dumps(row), flush=True)
    eng._drop_dyn_graphs()
    del graph, eng
    torch.cuda.empty_cache()


def measure_cable(name, mesh):
    nodes, el, loads, fixed = mesh[:4]
    model = FEMModel(nodes=nodes, elements=el, material=Material(2000.0, 0.5, 1.0), loads=1e-3 * loads, fixed_dofs=fixed,
                     dimension=2)
    nd, ne, K = model.ndof, model.nelm, args.steps
    mass = lumped_mass(model)
    taut_e0 = np.full(ne, E0)
    half_e0 = np.where(np.arange(ne) % 2 == 1, -E0, E0)
    flags = np.ones(ne, dtype=bool)
    dt = 0.5 * 2.0 / omega_bound(model, np.zeros(ne), taut_e0, mass)
    runs = {"bar": (taut_e0, None), "taut": (taut_e0, flags), "half": (half_e0, flags)}
    engines = {k: HipEngine(model) for k in runs}           # a run's state lives on its engine
    dev = engines["bar"].device
    minv = torch.from_numpy(np.repeat(1.0 / mass, 2)).to(dev)
    zero = torch.zeros(nd, dtype=torch.float64, device=dev)
    for k, (e0, cable) in runs.items():
        engines[k].dyn_begin(zero, zero, minv, dt, ALPHA, 1.0, 1.0, 0.0, None, torch.from_numpy(e0).to(dev), start=False,
                             cable=cable)
    variants = {}
    for k in runs:
        variants[k + "_eager"] = lambda k=k: engines[k].dyn_steps(K, use_graph=False)
        variants[k + "_graph"] = lambda k=k: engines[k].dyn_steps(K, use_graph=True)
    for fn in variants.values():                    # warm-up: every variant once (the graphs are captured here)
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            eng = engines[k.split("_")[0]]
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with eng.on_stream():
                a.record(eng.stream)
            fn()
            with eng.on_stream():
                b.record(eng.stream)
            torch.cuda.synchronize()
            times[k].append(1e3 * a.elapsed_time(b) / K)
    row = {"mesh": name, "nodes": model.nnode, "elements": ne, "steps_per_region": K, "rounds": args.rounds, "dt": dt}
    for k, eng in engines.items():
        assert bool(torch.isfinite(eng.dyn_state()[0]).all())
        eng.dyn_energy()
        row[k + "_slack_elements"] = eng.dyn_slack_count()
    for k, t in times.items():
        row[k + "_us"] = {"median": float(np.median(t)), "min": float(np.min(t)), "max": float(np.max(t))}
    med = lambda k: row[k + "_us"]["median"]
    for k in ("taut", "half"):
        row[k + "_over_bar_eager"] = med(k + "_eager") / med("bar_eager")
        row[k + "_over_bar_graph"] = med(k + "_graph") / med("bar_graph")
    print(json.dumps(row), flush=True)
    for eng in engines.values():
        eng._drop_dyn_graphs()
    del engines
    torch.cuda.empty_cache()


def measure_history(name, mesh):
    nodes, el, loads, fixed = mesh[:4]
    model = FEMModel(nodes=nodes, elements=el, material=Material(2000.0, 0.5, 1.0), loads=1e-3 * loads, fixed_dofs=fixed,
                     dimension=2)
    nd, ne, K = model.ndof, model.nelm, args.steps
    mass = lumped_mass(model)
    e0_np = np.full(ne, E0)
    dt = 0.5 * 2.0 / omega_bound(model, np.zeros(ne), e0_np, mass)
    n_samples = K * (2 * args.rounds + 2) + 2           # warm-up and rounds, eager and graph, on one clock
    t = np.arange(n_samples) * dt
    lam, sup = 1.0 + 0.1 * np.sin(3.0 * t), np.sin(5.0 * t)
    amp = np.zeros(nd)
    amp[np.asarray(fixed, dtype=np.int64)] = 1e-4
    runs = {"bar": {}, "load": dict(load_samples=lam), "support": dict(support=(amp, sup)),
            "both": dict(load_samples=lam, support=(amp, sup))}
    engines = {k: HipEngine(model) for k in runs}           # a run's state lives on its engine
    dev = engines["bar"].device
    minv = torch.from_numpy(np.repeat(1.0 / mass, 2)).to(dev)
    zero = torch.zeros(nd, dtype=torch.float64, device=dev)
    for k, hist in runs.items():
        engines[k].dyn_begin(zero, zero, minv, dt, ALPHA, 1.0, 1.0, 0.0, None, torch.from_numpy(e0_np).to(dev), start=False, **hist)
    variants = {}
    for k in runs:
        variants[k + "_eager"] = lambda k=k: engines[k].dyn_steps(K, use_graph=False)
        variants[k + "_graph"] = lambda k=k: engines[k].dyn_steps(K, use_graph=True)
    for fn in variants.values():                    # warm-up: every variant once (the graphs are captured here)
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            eng = engines[k.split("_")[0]]
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with eng.on_stream():
                a.record(eng.stream)
            fn()
            with eng.on_stream():
                b.record(eng.stream)
            torch.cuda.synchronize()
            times[k].append(1e3 * a.elapsed_time(b) / K)
    row = {"mesh": name, "nodes": model.nnode, "elements": ne, "fixed_dofs": int(len(fixed)), "steps_per_region": K,
           "rounds": args.rounds, "dt": dt, "samples": n_samples}
    for k, eng in engines.items():
        u, _, n = eng.dyn_state()
        assert bool(torch.isfinite(u).all()) and n == n_samples - 2
        row[k + "_max_abs_u"] = float(u.abs().max())
    for k, t_us in times.items():
        row[k + "_us"] = {"median": float(np.median(t_us)), "min": float(np.min(t_us)), "max": float(np.max(t_us))}
    med = lambda k: row[k + "_us"]["median"]
    for k in ("load", "support", "both"):
        row[k + "_over_bar_eager"] = med(k + "_eager") / med("bar_eager")
        row[k + "_over_bar_graph"] = med(k + "_graph") / med("bar_graph")
    print(json.dumps(row), flush=True)
    for eng in engines.values():
        eng._drop_dyn_graphs()
    del engines
    torch.cuda.empty_cache()


run = measure_cable if args.cable else measure_history if args.history else measure
for n in args.chains:
    run(f"chain_{n}", chain_mesh(n))
for n in args.warren:
    run(f"warren_{n}", warren_mesh(n))
