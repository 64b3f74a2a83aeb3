#!/usr/bin/env python3
"""Time the elastoplastic element state against the bar state with an initial strain, on counter-braced girders.

    plastic_state_scale.py [--regions 11] [--calls 200] [--kernel-panels 800000] [panels ...]   (default: 64 1000 100000)

The girder is tools/cable_state_scale.py's: nodes (i, 0) and (i, 1), per panel two chords, a vertical and two diagonals
(5 * panels elements).  At a seeded random displacement field with strains of a few 1e-3 against a yield strain of 1e-3 and a
seeded committed state (a good third of the elements plastic) it times, as the median over `regions` regions of `calls` calls
each, in microseconds per call:
  e0        HipEngine.gl_state(u, e0=...): pf_gl_state_e0, the yardstick (device events around a region)
  plastic   gl_state_plastic(u, ey, kappa) and the read of the two counts, what a Newton iteration does (host clock; the
            read synchronises)
On these sizes the call rate decides, not the kernel.  On the mesh of --kernel-panels panels (4e6 elements by default; 0
skips it) both variants are `calls` back-to-back launches between device events, without the count read: the kernels' own
time.  By bytes per 2-D element the plastic kernel moves about 162 (conn 8, d0 16, u 32, e0 8, ey, kappa, ep_n, al_n 32,
flag in and out 2; strain 8, fe 16, kt 24, ep, al 16) against the bar's 112, a ratio of 1.45.
The variants alternate region by region in one process.  One JSON line per size, with the spread (min, max) of every
median's regions."""
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
ap.add_argument("--kernel-panels", type=int, default=800000)
ap.add_argument("panels", nargs="*", type=int, default=[64, 1000, 100000])
args = ap.parse_args()
EY = 1e-3


def girder(n):
    nodes = np.zeros((2 * (n + 1), 2))
    nodes[0::2, 0] = nodes[1::2, 0] = np.arange(n + 1)
    nodes[1::2, 1] = 1.0
    b0 = 2 * np.arange(n)
    el = np.stack([np.stack(p, axis=1) for p in ((b0, b0 + 2), (b0 + 1, b0 + 3), (b0 + 2, b0 + 3), (b0, b0 + 3), (b0 + 1, b0 + 2))],
                  axis=1).reshape(-1, 2)
    return nodes, el


def summary(samples):
    return {"median": float(np.median(samples)), "min": float(np.min(samples)), "max": float(np.max(samples))}


for panels, kernel_only in [(p, False) for p in args.panels] + ([(args.kernel_panels, True)] if args.kernel_panels else []):
    nodes, el = girder(panels)
    model = FEMModel(nodes=nodes, elements=el, material=Material(2000.0, 0.5, 1.0), loads=np.zeros(nodes.size),
                     fixed_dofs=np.array([0, 1, 2, 3]), dimension=2)
    eng = HipEngine(model)
    rng = np.random.default_rng(panels)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)
    u = dev(2e-3 * rng.standard_normal(nodes.size))
    e0 = dev(rng.uniform(-3e-4, 3e-4, len(el)))
    ey, kappa = dev(np.full(len(el), EY)), dev(rng.uniform(0.0, 0.5, len(el)))
    ep_n = rng.uniform(-0.8, 0.8, len(el)) * EY
    eng.gl_plastic_reset(ep_n, np.abs(ep_n) + rng.uniform(0.0, 0.5, len(el)) * EY)

    def bar():
        eng.gl_state(u, e0=e0)

    def launch():
        eng.gl_state_plastic(u, ey, kappa, e0=e0)

    def with_counts():
        eng.gl_state_plastic(u, ey, kappa, e0=e0)
        return eng.gl_plastic_counts()[0]

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

    variants = [("e0", bar, events), ("plastic", launch, events) if kernel_only else ("plastic", with_counts, clock)]
    samples = {name: [] for name, _, _ in variants}
    for name, fn, _ in variants:                 # warm-up: every shape the timed regions use
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    for _ in range(args.regions):                # the variants alternate region by region
        for name, fn, timer in variants:
            samples[name].append(timer(fn))
    med = {name: summary(s) for name, s in samples.items()}
    row = {"panels": panels, "elements": len(el), "plastic": with_counts(), "regions": args.regions, "calls": args.calls,
           "timed": "launches between device events" if kernel_only else "e0: device events; plastic: host clock with the count read",
           "microseconds_per_call": med, "ratio_of_medians": med["plastic"]["median"] / med["e0"]["median"]}
    print(json.dumps(row), flush=True)
    del eng, model
    torch.cuda.empty_cache()
