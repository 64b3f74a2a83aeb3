#!/usr/bin/env python3
"""Time the H prestress right-hand sides of one load level on the Warren girder of tools/nr_scale.py.

    prestress_rhs_time.py [--path kernel|strain-rhs] [--groups 8] [--repeats 300] [panels]

--path kernel:      one HipEngine.gl_prestress_rhs call (pf_gl_prestress_rhs: all H rows in one launch, the group map cached on
                    the device).
--path strain-rhs:  what that call replaces: per group a coefficient vector built on the host (ea * l0 on the group's
                    elements, 0.0 elsewhere), uploaded, and one gl_strain_rhs call (pf_gl_strain_rhs gives +-(c / l0^2) d).
After a warm-up of 20 sets, `repeats` sets back to back and one device synchronise; a host clock around them.  One JSON
line: microseconds per set of H rows, and the largest difference between the two paths' rows relative to the largest
entry (they differ in the last bits: ea * l0 / l0^2 against ea / l0).  Run each path in a process of its own."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("PINNFEM_QUIET", "1")
from pinn_fem_amd.engine import HipEngine
from pinn_fem_amd.fem.model import FEMModel, Material
from pinn_fem_amd.plan import warren_mesh
import torch
ap = argparse.ArgumentParser()
ap.add_argument("--path", choices=("kernel", "strain-rhs"), default="kernel")
ap.add_argument("--groups", type=int, default=8)
ap.add_argument("--repeats", type=int, default=300)
ap.add_argument("panels", nargs="?", type=int, default=1000)
args = ap.parse_args()
panels, H = args.panels, args.groups
nodes, el, loads, fixed, _, _ = warren_mesh(panels)
model = FEMModel(nodes=nodes, elements=el, material=Material(2.0, 0.5, 1.0), loads=loads, fixed_dofs=fixed, dimension=2)
eng = HipEngine(model)
xc = 0.5 * (nodes[el[:, 0], 0] + nodes[el[:, 1], 0])
groups = np.minimum((H * xc / float(panels)).astype(int), H - 1)
rng = np.random.default_rng(0)
u = torch.from_numpy(1e-3 * rng.standard_normal(2 * len(nodes))).to(eng.device)
ea_np = np.where(groups % 2 == 0, 0.8, 1.25)
ea = torch.from_numpy(ea_np).to(eng.device)
l0 = np.linalg.norm(nodes[el[:, 1]] - nodes[el[:, 0]], axis=1)


def kernel_path():
    return eng.gl_prestress_rhs(u, ea, groups)


def strain_rhs_path():
    rows = []
    for h in range(H):
        coef = np.where(groups == h, ea_np * l0, 0.0)
        rows.append(eng.gl_strain_rhs(u, torch.from_numpy(coef).to(eng.device)))
    return torch.stack(rows)


run = kernel_path if args.path == "kernel" else strain_rhs_path
for _ in range(20):
    run()
torch.cuda.synchronize(); t0 = time.perf_counter()
for _ in range(args.repeats):
    run()
torch.cuda.synchronize(); dt = time.perf_counter() - t0
a, b = kernel_path(), strain_rhs_path()
torch.cuda.synchronize()
print(json.dumps({"path": args.path, "panels": panels, "elements": len(el), "dofs": 2 * len(nodes), "groups": H,
                  "repeats": args.repeats, "microseconds_per_set": 1e6 * dt / args.repeats,
                  "paths_apart_relative": float((a - b).abs().max() / a.abs().max())}), flush=True)
