#!/usr/bin/env python3
"""solve_nr (matrix-free float64 K v + preconditioned CG on the device) on Warren girders of growing size; for the
smaller ones also the oracle's dense float64 restatement of the reference (np.linalg.solve) on the host.

    nr_scale.py [--preconditioner jacobi|two-level|two-level-updated] [--aggregates N]
                [--kinematics linear|green-lagrange] [--initial-strain X] [panels ...]

The timed solve includes the two-level preconditioner's setup (coarse space, Z^T K Z, its inverse).  With
--kinematics green-lagrange the same girders run the large-displacement element (jacobi or two-level-updated; the dense
comparison is of the linear problem and is left out).  two-level-updated refreshes its coarse space at every Newton
iteration: the row reports the seconds spent there (refresh_seconds) and their parts: host columns, setup launch with
the read-back, Cholesky and inverse, upload.  --initial-strain X (green-lagrange only) gives every element the initial
strain X (X < 0: a pretension; SolverConfig.initial_strain)."""
import argparse, json, os, re, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("PINNFEM_QUIET", "1")
from pinn_fem_amd.fem.model import FEMModel, Material
from pinn_fem_amd.fem.solver import SolverConfig, solve_nr
from pinn_fem_amd.plan import warren_mesh
import torch
ap = argparse.ArgumentParser()
ap._negative_number_matcher = re.compile(r"^-(\d+\.?\d*|\.\d+)([eE][-+]?\d+)?$")    # -1e-3 is a value, not an option
ap.add_argument("--preconditioner", default="jacobi", choices=["jacobi", "two-level", "two-level-updated"])
ap.add_argument("--aggregates", type=int, default=None)
ap.add_argument("--kinematics", default="linear", choices=["linear", "green-lagrange"])
ap.add_argument("--initial-strain", type=float, default=None)
ap.add_argument("panels", nargs="*", type=int)
args = ap.parse_args()
if args.initial_strain is not None and args.kinematics != "green-lagrange":
    ap.error("--initial-strain goes with --kinematics green-lagrange only")
if args.preconditioner == "two-level-updated" and args.kinematics != "green-lagrange":
    ap.error("--preconditioner two-level-updated goes with --kinematics green-lagrange only")
rows = []
for panels in args.panels or [100, 1000, 5000]:
    nodes, el, loads, fixed, mv, md = warren_mesh(panels)
    model = FEMModel(nodes=nodes, elements=el, material=Material(2.0, 0.5, 1.0), loads=loads, fixed_dofs=fixed, dimension=2)
    # green-lagrange: the unit loads would fold a girder of E*A = 1 up; scale them so that the midspan sags about a
    # hundredth of the span (beam theory: 5 q L^4 / (384 EI), EI = E*A*height^2 / 2 = 0.5).  An estimate: that this load
    # keeps the tangent positive definite and the Newton loop inside 25 iterations is what the run itself shows (the row
    # reports `converged`; a non-SPD state raises)
    green_lagrange = args.kinematics == "green-lagrange"
    lam = (panels / 100.0) * 384.0 * 0.5 / (5.0 * float(panels) ** 4) if green_lagrange else 1.0
    cfg = SolverConfig(max_iterations=25 if green_lagrange else 10, tolerance=1e-10,
                       nr_preconditioner=args.preconditioner, nr_aggregates=args.aggregates, kinematics=args.kinematics,
                       initial_strain=args.initial_strain)
    if panels <= 100:                                        # warm-up (library load, allocator) on a model of its own
        solve_nr(FEMModel(nodes=nodes, elements=el, material=Material(2.0, 0.5, 1.0), loads=loads, fixed_dofs=fixed, dimension=2),
                 cfg, lam)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    res = solve_nr(model, cfg, lam)
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    eng = model._pf_engine_cache[1]
    row = {"panels": panels, "elements": len(el), "dofs": 2 * len(nodes), "preconditioner": args.preconditioner,
           "kinematics": args.kinematics, "load_factor": lam,
           "hip_seconds": dt, "converged": bool(res.converged), "nr_iterations": res.history[-1]["iterations"],
           "cg_iterations": eng.pcg_iterations}
    if args.initial_strain is not None:
        row["initial_strain"] = args.initial_strain
    if args.preconditioner == "two-level-updated":
        row["refresh_seconds"] = eng.coarse_refresh_seconds
        row["refresh_parts"] = dict(eng.coarse_refresh_parts)
    if 2 * len(nodes) <= 4100 and args.kinematics == "linear":
        from oracle import pinn_oracle as orc
        pb = orc.Problem(nodes=nodes, elements=el, loads=loads, fixed_dofs=fixed, dimension=2, young=2.0, area=0.5, density=1.0)
        t0 = time.perf_counter(); ref = orc.solve_nr(pb, orc.SolverConfig(max_iterations=10, tolerance=1e-10), 1.0)
        row["dense_numpy_seconds"] = time.perf_counter() - t0
        row["rel_err_u"] = float(np.max(np.abs(res.displacements - ref.displacements)) / np.max(np.abs(ref.displacements)))
    rows.append(row)
    print(json.dumps(row), flush=True)
