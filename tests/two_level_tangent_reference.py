"""The cantilevered Warren girder on which the two-level preconditioner of the Green-Lagrange tangent solve is measured,
and its CPU run: gl_reference's Newton loop with a sparse direct solve, the tangent at every Newton state, and scipy's CG
on each of them with the restated preconditioners of two_level_reference.py.

Test infrastructure only: used on the CPU by tests/test_two_level_tangent_host.py and on the GPU by
tests/test_pcg_two_level_tangent.py.  Each run is computed once per process (functools.lru_cache) and must not be changed
by its users.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np
import scipy.sparse.linalg as spla

import gl_reference as gl
import two_level_reference as tl

YOUNG, AREA = 2.0e6, 0.5                        # E*A = 1e6, exact in float32
EA = YOUNG * AREA


@functools.lru_cache(maxsize=None)
def warren_case(panels=100, n_agg=32, n_inc=4, sag=0.1):
    """gl_reference.cantilever_warren(panels) with E*A = 1e6 and the tip load at which the LINEAR tip deflection is `sag`
    of the span; the strip aggregates of the reference configuration; the direct-solve Newton run in n_inc equal
    increments (tolerance 1e-10) with every Newton state (u, K_t(u)) it passed through."""
    from pinn_fem_amd.coarse import strip_aggregates
    nodes, el, unit, fixed, tip = gl.cantilever_warren(panels)
    n = nodes.size
    free = gl.free_mask(n, fixed)
    idx = np.flatnonzero(free)
    lin = np.zeros(n)
    lin[idx] = spla.spsolve(gl.restrict(gl.k_t(nodes, el, np.zeros(n), EA, 2), free), unit[idx])
    span = float(np.ptp(nodes[:, 0]))
    p_tip = sag * span / abs(lin[tip])
    loads = p_tip * unit
    states = []
    u_ref, its = gl.incremental(nodes, el, loads, fixed, EA, 2, n_inc, tol=1e-10,
                                on_iterate=lambda u, K, fr, rhs: states.append((u.copy(), K)))
    rhs, k = [], 0
    for inc, it in enumerate(its, 1):               # the right-hand side of every state's Newton step
        for _ in range(it):
            u = states[k][0]
            rhs.append(np.where(free, (inc / n_inc) * loads - gl.f_int(nodes, el, u, EA, 2), 0.0))
            k += 1
    return SimpleNamespace(panels=panels, n_agg=n_agg, n_inc=n_inc, nodes=nodes, el=el, unit=unit, loads=loads, fixed=fixed,
                           tip=tip, free=free, mask=~free, n=n, p_tip=p_tip, u_ref=u_ref, its=its, states=states, rhs=rhs,
                           node_agg=strip_aggregates(nodes, 2, n_agg))


def columns(case, u=None):
    """The coarse space on X + u (u None: on X) with the case's aggregation."""
    from pinn_fem_amd.coarse import update_coarse_space
    X = case.nodes if u is None else case.nodes + np.asarray(u).reshape(-1, 2)
    return update_coarse_space(X, 2, case.mask, case.node_agg)


def cg_state(case, k, kind, b=None):
    """scipy's CG at rtol 1e-13 on the tangent of Newton state k, right-hand side b (default: that state's own):
    (x, iterations, info).  kind: "jacobi", "reference" (two-level, columns on X) or "current" (columns on X + u)."""
    u, K = case.states[k]
    b = case.rhs[k] if b is None else np.where(case.mask, 0.0, b)
    if kind == "jacobi":
        Kff, M = tl.ref.restrict_ff(K, case.mask), tl.jacobi_operator(K, case.mask)
    else:
        P = tl.TwoLevel(K, case.mask, columns(case, u if kind == "current" else None))
        Kff, M = P.Kff, P.operator()
    return tl.cg(Kff, b, M, 40 * case.n + 2000)


@functools.lru_cache(maxsize=None)
def cg_counts(panels=100, n_agg=32, n_inc=4, kind="current"):
    """CG iterations per Newton state of warren_case(...) and whether every solve converged."""
    case = warren_case(panels, n_agg, n_inc)
    out = [cg_state(case, k, kind)[1:] for k in range(len(case.states))]
    return [it for it, _ in out], all(info == 0 for _, info in out)


@functools.lru_cache(maxsize=None)
def cg_newton(panels=100, n_agg=32, n_inc=4):
    """The same incremental Newton run with every step solved by scipy's CG and the current-configuration two-level
    preconditioner: (u, Newton iterations per increment, total CG iterations)."""
    case = warren_case(panels, n_agg, n_inc)
    idx = np.flatnonzero(case.free)
    total = [0]
    state = {}

    def on_iterate(u, K, free, rhs):
        state["u"], state["K"] = u, K

    def solve(Kff_small, rhs_small):
        P = tl.TwoLevel(state["K"], case.mask, columns(case, state["u"]))
        b = np.zeros(case.n)
        b[idx] = rhs_small
        y, it, info = tl.cg(P.Kff, b, P.operator(), 40 * case.n + 2000)
        assert info == 0
        total[0] += it
        return y[idx]
    u, its = gl.incremental(case.nodes, case.el, case.loads, case.fixed, EA, 2, n_inc, tol=1e-10, on_iterate=on_iterate,
                            linear_solve=solve)
    return u, its, total[0]
