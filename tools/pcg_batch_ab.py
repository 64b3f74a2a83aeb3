#!/usr/bin/env python3
"""Two tangent CG solves one after the other against one batched solve of the same two right-hand sides.

    pcg_batch_ab.py --baseline-root DIR [--pairs 3] [panels ...]          the A/B run: alternates child processes
    pcg_batch_ab.py --side sequential|batch [--root DIR] [panels ...]     one side (what the children run)

The system is the simply supported Warren girder of tools/nr_scale.py --kinematics green-lagrange at the converged state
of its load; the right-hand sides are the loads on the free dofs and a seeded random vector; the preconditioner is
Jacobi.  "sequential" is two pcg_solve(tangent=True) calls and uses nothing a checkout of the commit before the batched
solve lacks, so --baseline-root can point at one (with its own built library); "batch" is one pcg_solve_batch.  Each
side is timed with a host clock around calls that end in a synchronise, after a warm-up solve.  Every measurement is a
fresh process (one package tree per process), run alternately: baseline, candidate, baseline, ...  Prints one JSON line
per measurement and a summary per size: iterations, seconds of each side and the ratio with its spread."""
import argparse, json, os, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--side", choices=["sequential", "batch"])
ap.add_argument("--root", default=ROOT, help="package tree to import (a checkout of the baseline for --side sequential)")
ap.add_argument("--baseline-root")
ap.add_argument("--pairs", type=int, default=3)
ap.add_argument("panels", nargs="*", type=int)
args = ap.parse_args()
panels_list = args.panels or [100, 300, 1000]


def one_side():
    sys.path.insert(0, os.path.abspath(args.root))
    os.environ.setdefault("PINNFEM_QUIET", "1")
    import numpy as np
    import torch
    from pinn_fem_amd.fem.model import FEMModel, Material
    from pinn_fem_amd.fem.solver import SolverConfig, solve_nr
    from pinn_fem_amd.plan import warren_mesh
    for panels in panels_list:
        nodes, el, loads, fixed, _, _ = warren_mesh(panels)
        model = FEMModel(nodes=nodes, elements=el, material=Material(2.0, 0.5, 1.0), loads=loads, fixed_dofs=fixed, dimension=2)
        lam = (panels / 100.0) * 384.0 * 0.5 / (5.0 * float(panels) ** 4)      # as tools/nr_scale.py
        res = solve_nr(model, SolverConfig(max_iterations=25, tolerance=1e-10, kinematics="green-lagrange"), lam)
        assert res.converged
        eng = model._pf_engine_cache[1]
        n = model.ndof
        free = np.ones(n, dtype=bool)
        free[np.asarray(fixed, dtype=int)] = False
        f = np.where(free, np.asarray(loads, dtype=float).reshape(-1), 0.0)
        g = np.where(free, np.random.default_rng(7).standard_normal(n), 0.0)
        B = torch.from_numpy(np.stack([f, g])).to(eng.device)
        eng.gl_state(torch.from_numpy(res.displacements.reshape(-1).copy()).to(eng.device))

        def run():
            if args.side == "sequential":
                return [eng.pcg_solve(B[k], tangent=True)[1:3] for k in range(2)]
            return [r[:2] for r in eng.pcg_solve_batch(B)[1]]
        run()                                                   # warm-up
        torch.cuda.synchronize(); t0 = time.perf_counter()
        reports = run()
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        print(json.dumps({"side": args.side, "panels": panels, "dofs": n, "iterations": [int(r[0]) for r in reports],
                          "converged": [bool(r[1]) for r in reports], "seconds": dt}), flush=True)


def ab():
    import statistics
    rows = []
    for pair in range(args.pairs):
        for side, root in (("sequential", args.baseline_root), ("batch", ROOT)):
            cmd = [sys.executable, os.path.abspath(__file__), "--side", side, "--root", root] + [str(p) for p in panels_list]
            out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300).stdout
            for line in out.splitlines():
                if line.startswith("{"):
                    rows.append(dict(json.loads(line), pair=pair))
                    print(line, flush=True)
    for panels in panels_list:
        seq = [r for r in rows if r["panels"] == panels and r["side"] == "sequential"]
        bat = [r for r in rows if r["panels"] == panels and r["side"] == "batch"]
        ratios = [b["seconds"] / s["seconds"] for s, b in zip(seq, bat)]
        print(json.dumps({"panels": panels, "iterations_sequential": seq[0]["iterations"], "iterations_batch": bat[0]["iterations"],
                          "sequential_seconds": [round(r["seconds"], 6) for r in seq],
                          "batch_seconds": [round(r["seconds"], 6) for r in bat],
                          "ratio_median": statistics.median(ratios), "ratio_min": min(ratios), "ratio_max": max(ratios)}),
              flush=True)


if args.side:
    one_side()
elif args.baseline_root:
    ab()
else:
    ap.error("give --baseline-root DIR (the A/B run) or --side")
