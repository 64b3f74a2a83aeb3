#!/usr/bin/env python3
"""Time identify_nr (fem/identify.py) on the Warren girder of tools/nr_scale.py --kinematics green-lagrange.

    identify_scale.py [--preconditioner jacobi|two-level-updated] [--aggregates N] [--groups 8] [--levels 2]
                      [--method lbfgs|gauss-newton] [--data displacements|strains] [--evaluations 200]
                      [--relative-misfit 1e-12] [--parameters stiffness|prestress|both] [panels]

The girder (E*A = 1, the load of nr_scale.py) gets one true factor per span group, alternating 0.8 / 1.25; its states at
the load levels k / levels, solved on the device, are the measurements (every free dof), which is also the warm-up
solve.  identify_nr then runs a whole identification from all factors 1 with the chosen method, to its own stop: the
misfit tolerance is `relative-misfit` times the sum over the levels of the mean square of the measurements, the same for
both methods, and `evaluations` is only the cap.  --data strains: the measurements are strain gauges and nothing else,
one per group on the group's lowest-numbered element, with strain_scale L = the span, and the misfit tolerance is
`relative-misfit` times the sum over the levels of L^2 times the mean square of the measured strains; the row then also
holds the singular values' ends of the Jacobian (method gauss-newton) and the launch times of pf_gl_strain_rhs and
pf_gl_strain_jvp.  One JSON line: total seconds, evaluations, the stop, the factor error,
seconds and Newton, CG, adjoint CG and sensitivity CG iterations in total and per evaluation, and the time of single
pf_gl_state (model E*A and per-element E*A), pf_gl_sens, pf_group_sum_f64 and pf_gl_group_rhs launches (mean of 200
back-to-back launches between two events) with the share of an evaluation of the L-BFGS path's own two.
--parameters prestress|both: identify_prestress (fem/prestress.py) in place of identify_nr.  The true structure carries one
prestress strain per span group, alternating -1e-4 / -5e-5 (tensile: with a compressive one of that size the tangent of this
slender, statically determinate girder is indefinite at u = 0, where every element still carries -E*A*e0, and the two-level
preconditioner falls back to Jacobi there), which is identified from t = 0; with `both` the factors above
are identified alongside (from all factors 1), with `prestress` E*A is known and every true factor is 1.  The loop is the
Levenberg-Marquardt one whatever --method says; the row holds the prestress error and the launch time of
pf_gl_prestress_rhs."""
import argparse, dataclasses, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("PINNFEM_QUIET", "1")
from pinn_fem_amd.fem.identify import identify_nr, misfit_and_gradient
from pinn_fem_amd.fem.model import FEMModel, Material
from pinn_fem_amd.fem.prestress import identify_prestress
from pinn_fem_amd.fem.solver import SolverConfig
from pinn_fem_amd.plan import warren_mesh
import torch
ap = argparse.ArgumentParser()
ap.add_argument("--preconditioner", default="jacobi", choices=["jacobi", "two-level-updated"])
ap.add_argument("--aggregates", type=int, default=None)
ap.add_argument("--groups", type=int, default=8)
ap.add_argument("--levels", type=int, default=2)
ap.add_argument("--method", choices=("lbfgs", "gauss-newton"), default="lbfgs")
ap.add_argument("--data", choices=("displacements", "strains"), default="displacements")
ap.add_argument("--evaluations", type=int, default=200)
ap.add_argument("--relative-misfit", type=float, default=1e-12)
ap.add_argument("--parameters", choices=("stiffness", "prestress", "both"), default="stiffness")
ap.add_argument("panels", nargs="?", type=int, default=1000)
args = ap.parse_args()
panels = args.panels
nodes, el, loads, fixed, _, _ = warren_mesh(panels)
lam = (panels / 100.0) * 384.0 * 0.5 / (5.0 * float(panels) ** 4)          # nr_scale.py's: midspan sag about span / 100
model = FEMModel(nodes=nodes, elements=el, material=Material(2.0, 0.5, 1.0), loads=lam * loads, fixed_dofs=fixed, dimension=2)
cfg = SolverConfig(max_iterations=25, tolerance=1e-10, kinematics="green-lagrange", nr_preconditioner=args.preconditioner,
                   nr_aggregates=args.aggregates)
xc = 0.5 * (nodes[el[:, 0], 0] + nodes[el[:, 1], 0])
groups = np.minimum((args.groups * xc / float(panels)).astype(int), args.groups - 1)
true = np.where(np.arange(args.groups) % 2 == 0, 0.8, 1.25)
true_t = None
if args.parameters != "stiffness":
    true_t = np.where(np.arange(args.groups) % 2 == 0, -1e-4, -5e-5)
    if args.parameters == "prestress":
        true = np.ones(args.groups)
true_cfg = cfg if true_t is None else dataclasses.replace(cfg, initial_strain=true_t[groups])
true_e0 = None if true_t is None else true_t[groups]
free = np.ones(2 * len(nodes), dtype=bool)
free[fixed] = False
dofs = np.flatnonzero(free)
factors = [(k + 1) / args.levels for k in range(args.levels)]
# measurements: the states of the true structure (the misfit against zeros is not used); the warm-up solve as well
_, _, states, _ = misfit_and_gradient(model, true_cfg, [(f, dofs, np.zeros(len(dofs))) for f in factors], true[groups])
eng = model._pf_engine_cache[1]
if args.data == "strains":
    gauges = np.array([np.flatnonzero(groups == g)[0] for g in range(args.groups)])
    span = float(panels)
    ea_true = torch.from_numpy(true[groups]).to(eng.device)
    e0_true = None if true_e0 is None else torch.from_numpy(true_e0).to(eng.device)
    levels = [{"load_factor": f, "dofs": [], "u": [], "strain_elements": gauges,
               "strains": eng.gl_state(s, ea_true, e0_true).cpu().numpy()[gauges], "strain_scale": span} for f, s in zip(factors, states)]
    misfit_tolerance = args.relative_misfit * sum(span ** 2 * float(np.mean(lv["strains"] ** 2)) for lv in levels)
else:
    levels = [(f, dofs, s.cpu().numpy()[dofs]) for f, s in zip(factors, states)]
    misfit_tolerance = args.relative_misfit * sum(float(np.mean(lv[2] ** 2)) for lv in levels)
refresh0, refreshes0 = eng.coarse_refresh_seconds, eng.coarse_refreshes
torch.cuda.synchronize(); t0 = time.perf_counter()
if args.parameters == "stiffness":
    res = identify_nr(model, cfg, levels, groups=groups, max_evaluations=args.evaluations, method=args.method,
                      misfit_tolerance=misfit_tolerance)
else:
    res = identify_prestress(model, cfg, levels, groups, groups=groups if args.parameters == "both" else None,
                             max_evaluations=args.evaluations, misfit_tolerance=misfit_tolerance)
torch.cuda.synchronize(); dt = time.perf_counter() - t0


def launch_us(fn, n=200):
    fn(); torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with eng.on_stream():
        a.record(eng.stream)
        for _ in range(n):
            fn()
        b.record(eng.stream)
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / n


u, ea = states[-1], torch.from_numpy(res.ea).to(eng.device)
adj, out = torch.ones_like(u), torch.zeros(len(el), dtype=torch.float64, device=eng.device)
us = {"pf_gl_state": launch_us(lambda: eng.gl_state(u)), "pf_gl_state_ea": launch_us(lambda: eng.gl_state(u, ea)),
      "pf_gl_sens": launch_us(lambda: eng.gl_sensitivity(u, adj, out=out)),
      "pf_group_sum_f64": launch_us(lambda: eng.group_sum(out, ea, groups)),
      "pf_gl_group_rhs": launch_us(lambda: eng.gl_group_rhs(groups))}
if args.parameters != "stiffness":
    us["pf_gl_prestress_rhs"] = launch_us(lambda: eng.gl_prestress_rhs(u, ea, groups))
if args.data == "strains":
    coef, V = torch.ones(len(el), dtype=torch.float64, device=eng.device), torch.ones((2, 2 * len(nodes)), dtype=torch.float64,
                                                                                     device=eng.device)
    rhs_out = torch.zeros(2 * len(nodes), dtype=torch.float64, device=eng.device)
    us["pf_gl_strain_rhs"] = launch_us(lambda: eng.gl_strain_rhs(u, coef, out=rhs_out))
    us["pf_gl_strain_jvp"] = launch_us(lambda: eng.gl_strain_jvp(u, gauges, V))
n = res.evaluations
per_eval = dt / n
row = {"panels": panels, "data": args.data, "elements": len(el), "dofs": 2 * len(nodes), "preconditioner": args.preconditioner,
       "groups": args.groups, "levels": args.levels, "method": args.method, "parameters": args.parameters, "seconds": dt,
       "evaluations": n,
       "stop": res.stop, "converged": res.converged, "misfit_tolerance": misfit_tolerance,
       "factor_error": None if res.factors is None else float(np.max(np.abs(res.factors - true))),
       "seconds_per_evaluation": per_eval,
       "newton_iterations": res.counters["newton_iterations"], "cg_iterations": res.counters["cg_iterations"],
       "adjoint_cg_iterations": res.counters["adjoint_cg_iterations"],
       "sensitivity_cg_iterations": res.counters.get("sensitivity_cg_iterations", 0),
       "jacobians": res.counters.get("jacobians", 0),
       "newton_iterations_per_evaluation": res.counters["newton_iterations"] / n,
       "cg_iterations_per_evaluation": res.counters["cg_iterations"] / n,
       "adjoint_cg_iterations_per_evaluation": res.counters["adjoint_cg_iterations"] / n,
       "misfit_first": res.history[0]["misfit"], "misfit_best": res.misfit, "launch_microseconds": us,
       "share_of_sens_and_group_sum": (args.levels * us["pf_gl_sens"] + us["pf_group_sum_f64"]) * 1e-6 / per_eval}
if true_t is not None:
    row["prestress_error"] = float(np.max(np.abs(res.prestress - true_t)))
    row["prestress_std_max"] = None if res.prestress_std is None else float(np.max(res.prestress_std))
if res.factor_std is not None:
    row["factor_std_max"] = float(np.max(res.factor_std))
if res.singular_values is not None and args.data == "strains":
    row["singular_value_max"], row["singular_value_min"] = float(res.singular_values[0]), float(res.singular_values[-1])
if args.preconditioner == "two-level-updated":
    row["refresh_seconds"] = eng.coarse_refresh_seconds - refresh0
    row["refreshes"] = eng.coarse_refreshes - refreshes0
    row["refresh_seconds_per_evaluation"] = (eng.coarse_refresh_seconds - refresh0) / n
print(json.dumps(row), flush=True)
