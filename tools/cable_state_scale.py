#!/usr/bin/env python3
"""Time the element state with tension-only (cable) elements on counter-braced girders.

    cable_state_scale.py [--regions 11] [--calls 200] [--variants bar,workaround,cable] [panels ...]
                                                                           (default: 64 1000 100000)

The girder: nodes (i, 0) and (i, 1), per panel two chords, a vertical and two diagonals, the diagonals flagged
(5 * panels elements).  At a seeded random displacement field (about half of the flagged elements slack) it times, as
the median over `regions` regions of `calls` calls each, in microseconds per call:
  bar         HipEngine.gl_state(u): the bar state alone (device events around a region)
  workaround  what solve_dynamic's closing state does: gl_state(u), the strains read back, an E*A array with zeros on the
              slack elements built on the host and sent, gl_state(u, ea) (host clock; the read-back synchronises)
  cable       gl_state_cable(u, flags) and the read of the two counts (host clock; the read synchronises); only where the
              engine has it, so the same file runs on a commit before pf_gl_state_cable
--variants picks among them: what a process times beside the bar state moves the bar's own figure (the host issues it), so a
comparison of two commits runs the same variants on both.
One JSON line per size, with the spread (min, max) of every median's regions."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("PINNFEM_QUIET", "1")
from pinn_fem_amd.engine import HipEngine
from pinn_fem_amd.fem.model import FEMModel, Material
import torch
ap = argparse.ArgumentParser()
ap.add_argument("--regions", type=int, default=11)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--variants", default="bar,workaround,cable")
ap.add_argument("panels", nargs="*", type=int, default=[64, 1000, 100000])
args = ap.parse_args()
EA = 1000.0


def girder(n):
    nodes = np.zeros((2 * (n + 1), 2))
    nodes[0::2, 0] = nodes[1::2, 0] = np.arange(n + 1)
    nodes[1::2, 1] = 1.0
    b0 = 2 * np.arange(n)
    el = np.stack([np.stack(p, axis=1) for p in ((b0, b0 + 2), (b0 + 1, b0 + 3), (b0 + 2, b0 + 3), (b0, b0 + 3), (b0 + 1, b0 + 2))],
                  axis=1).reshape(-1, 2)
    return nodes, el, np.tile([False, False, False, True, True], n)


def summary(samples):
    return {"median": float(np.median(samples)), "min": float(np.min(samples)), "max": float(np.max(samples))}


for panels in args.panels:
    nodes, el, cable = girder(panels)
    model = FEMModel(nodes=nodes, elements=el, material=Material(2000.0, 0.5, 1.0), loads=np.zeros(nodes.size),
                     fixed_dofs=np.array([0, 1, 2, 3]), dimension=2)
    eng = HipEngine(model)
    rng = np.random.default_rng(panels)
    u = torch.from_numpy(1e-3 * rng.standard_normal(nodes.size)).to(eng.device)
    flags = torch.from_numpy(cable.astype(np.uint8)).to(eng.device)
    has_cable = hasattr(HipEngine, "gl_state_cable")

    def bar():
        eng.gl_state(u)

    def workaround():
        strain = eng.gl_state(u).cpu().numpy()
        slack = cable & (strain < 0.0)
        eng.gl_state(u, torch.from_numpy(np.where(slack, 0.0, EA)).to(eng.device))
        return int(slack.sum())

    def with_cable():
        eng.gl_state_cable(u, flags)
        return eng.gl_slack_counts()[0]

    def events(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with eng.on_stream():
            a.record(eng.stream)
            for _ in range(args.calls):
                fn()
            b.record(eng.stream)
        torch.cuda.synchronize()
        return 1e3 * a.elapsed_time(b) / args.calls

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            fn()
        torch.cuda.synchronize()
        return 1e6 * (time.perf_counter() - t0) / args.calls

    variants = [("bar", bar, events), ("workaround", workaround, clock)] + ([("cable", with_cable, clock)] if has_cable else [])
    variants = [v for v in variants if v[0] in args.variants.split(",")]
    samples = {name: [] for name, _, _ in variants}
    for name, fn, _ in variants:                 # warm-up: every shape the timed regions use
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    for _ in range(args.regions):                # the variants alternate region by region
        for name, fn, timer in variants:
            samples[name].append(timer(fn))
    row = {"panels": panels, "elements": len(el), "slack": workaround(), "regions": args.regions, "calls": args.calls,
           "microseconds_per_call": {name: summary(s) for name, s in samples.items()}}
    if has_cable:
        assert with_cable() == row["slack"], (with_cable(), row["slack"])
    print(json.dumps(row), flush=True)
    del eng, model
    torch.cuda.empty_cache()
