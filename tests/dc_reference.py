"""Displacement control (Batoz-Dhatt) for the Green-Lagrange truss in numpy / scipy float64, on tests/gl_reference.py:
one free dof c is held at a prescribed value, the load factor lam is an unknown, and every linear solve is with
K' = K_t[F', F'], F' = F \\ {c}.  The loop is the one solve_nr runs in displacement mode, with a sparse direct solve (or,
optionally, gl_reference.jacobi_cg) in place of the device CG; it shares no code with the package.

  R = f_int(u) - lam f,  du_c = ubar - u_c (non-zero in the first iteration only)
  K' a = f[F'],   K' b = -R[F'] - k_c[F'] du_c,   k_c = K_t[:, c]
  dlam = -(R_c + k_c[F'].b + K_cc du_c) / (k_c[F'].a - f_c)
  u[F'] += b + dlam a,  u_c = ubar,  lam += dlam
"""
import numpy as np
import scipy.sparse.linalg as spla

import gl_reference as gl


def arch_warren(n, span, rise, depth):
    """Shallow Warren arch: bottom nodes 2i at x = i span / n on y = 4 rise x (span - x) / span^2, top nodes 2i + 1 at
    the panel mid-points on the same parabola plus depth, the connectivity of gl.cantilever_warren, both end bottom
    nodes pinned, a load of -1 in y on every interior bottom node.  Returns (nodes, el, loads, fixed, control dof): the
    control dof is the y-dof of bottom node 2 (n // 2)."""
    n = int(n)
    arc = lambda x: 4.0 * rise * x * (span - x) / span ** 2
    nodes = np.zeros((2 * n + 1, 2))
    xb = np.arange(n + 1) * span / n
    xt = (np.arange(n) + 0.5) * span / n
    nodes[0::2, 0], nodes[0::2, 1] = xb, arc(xb)
    nodes[1::2, 0], nodes[1::2, 1] = xt, arc(xt) + depth
    el = gl.cantilever_warren(n)[1]
    loads = np.zeros(2 * len(nodes))
    for i in range(1, n):
        loads[2 * (2 * i) + 1] = -1.0
    fixed = np.array([0, 1, 2 * (2 * n), 2 * (2 * n) + 1])
    return nodes, el, loads, fixed, 2 * (2 * (n // 2)) + 1


def initial_factor(nodes, el, loads, fixed, ea, dim, u):
    """lam0 = f[F].f_int(u)[F] / f[F].f[F]: the load factor of a converged state u."""
    f = np.asarray(loads, dtype=np.float64).reshape(-1)
    free = gl.free_mask(len(f), fixed)
    return float(f[free] @ gl.f_int(nodes, el, u, ea, dim)[free]) / float(f[free] @ f[free])


def control_step(nodes, el, loads, fixed, ea, dim, c, ubar, u0=None, tol=1e-10, max_iter=50, min_den=1e-10,
                 on_iterate=None, linear_solve=spla.spsolve):
    """One increment: the control dof c goes to ubar.  Returns (u, lam, iterations, converged).
    on_iterate(u, K, free, free_c) is called with the tangent of every iterate (free_c: the mask of F')."""
    f = np.asarray(loads, dtype=np.float64).reshape(-1)
    n = len(f)
    free = gl.free_mask(n, fixed)
    assert free[c], "the control dof must be free"
    fc = free.copy()
    fc[c] = False
    u = np.zeros(n) if u0 is None else np.where(free, np.asarray(u0, dtype=np.float64).reshape(-1), 0.0)
    lam = initial_factor(nodes, el, loads, fixed, ea, dim, u)
    for it in range(max_iter):
        K = gl.k_t(nodes, el, u, ea, dim)
        if on_iterate is not None:
            on_iterate(u, K, free, fc)
        R = gl.f_int(nodes, el, u, ea, dim) - lam * f
        duc = ubar - u[c]
        kc = np.asarray(K[:, [c]].todense()).reshape(-1)
        Kp = gl.restrict(K, fc)
        a = np.zeros(n)
        if np.any(f[fc] != 0.0):
            a[fc] = linear_solve(Kp, f[fc])
        b = np.zeros(n)
        b[fc] = linear_solve(Kp, -R[fc] - kc[fc] * duc)
        den = kc[fc] @ a[fc] - f[c]
        dlam = -(R[c] + kc[fc] @ b[fc] + kc[c] * duc) / den
        du = b + dlam * a
        du[c] = duc
        u = u + du
        u[c] = ubar
        lam += dlam
        if (np.linalg.norm(du) / max(np.linalg.norm(u), min_den) <= tol
                and abs(dlam) / max(abs(lam), min_den) <= tol):
            return u, lam, it + 1, True
    return u, lam, max_iter, False


def control_path(nodes, el, loads, fixed, ea, dim, c, u_final, n_inc, **kw):
    """solve()'s driver in displacement mode: n_inc equal steps of the control dof to u_final, each started from the
    last.  Returns (u, [lam per increment], [iterations per increment])."""
    u, lams, its = None, [], []
    for k in range(1, n_inc + 1):
        u, lam, it, ok = control_step(nodes, el, loads, fixed, ea, dim, c, (k / n_inc) * u_final, u0=u, **kw)
        assert ok, f"reference displacement control did not converge in increment {k}"
        lams.append(lam)
        its.append(it)
    return u, np.array(lams), its
