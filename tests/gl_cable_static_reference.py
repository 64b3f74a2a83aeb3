"""Tension-only (cable) elements in the static Green-Lagrange Newton solve, in numpy / scipy float64: gl_reference.newton with
the slack rule of the dynamics (gl_cable_reference.py) as an active-set iteration.  A flagged element with e - e0 < 0 is
slack and enters the internal force and the tangent with E A = 0.  Written from the rule's statement on
gl_reference's element; it shares no code with the kernels or with pinn_fem_amd/fem.  tests/test_gl_cable_static_host.py
pins it to gl_reference.newton of the structures without their slack elements and to closed forms.
"""
import numpy as np
import scipy.sparse.linalg as spla

import gl_reference as gl


class Mechanism(Exception):
    """A free dof with a non-positive tangent diagonal: only slack cables hold it.  iteration counts from 1."""

    def __init__(self, iteration, dof, value):
        super().__init__(f"iteration {iteration}: diagonal {value:g} at free dof {dof}")
        self.iteration, self.dof, self.value = iteration, dof, value


def slack_set(nodes, el, u, dim, cable, e0=None):
    """bool [ne]: flagged and e - e0 < 0 (e - 0.0 without an e0), and the margin min |e - e0| over the flagged elements."""
    strain = gl.element_state(nodes, el, u, 1.0, dim)[0]
    se = strain - np.broadcast_to(np.asarray(0.0 if e0 is None else e0, dtype=np.float64), strain.shape)
    cable = np.broadcast_to(np.asarray(cable, dtype=bool), strain.shape)
    return cable & (se < 0.0), (float(np.min(np.abs(se[cable]))) if cable.any() else np.inf)


def newton_cable(nodes, el, loads, fixed, ea, dim, cable, lam=1.0, u0=None, tol=1e-10, max_iter=50, min_den=1e-10,
                 linear_solve=spla.spsolve, e0=None):
    """gl.newton with the rule: every iteration forms slack = cable & (e - e0 < 0) at u and takes the element force and the
    tangent with E A = 0 on it.  It stops when |du| / max(|u|, min_den) <= tol AND the slack set of this iteration's state is
    the one of the state before (the first iteration has no state before it: its set does not count as a change).
    Returns (u, iterations, converged, slack at the final u, the number of iterations whose set differed from the one
    before).  A free dof with a tangent diagonal <= 0 raises Mechanism."""
    n = len(gl._as2d(nodes, dim)) * dim
    free = gl.free_mask(n, fixed)
    f = lam * np.asarray(loads, dtype=np.float64).reshape(-1)
    u = np.zeros(n) if u0 is None else np.where(free, np.asarray(u0, dtype=np.float64).reshape(-1), 0.0)
    ea = np.broadcast_to(np.asarray(ea, dtype=np.float64), (len(el),))
    before, changes, done, it = None, 0, False, 0
    for it in range(1, max_iter + 1):
        slack = slack_set(nodes, el, u, dim, cable, e0)[0]
        changed = before is not None and bool((slack != before).any())
        changes += changed
        before = slack
        ea_now = np.where(slack, 0.0, ea)
        K = gl.k_t(nodes, el, u, ea_now, dim, e0=e0)
        diag = K.diagonal()
        bad = np.flatnonzero(free & ~(diag > 0.0))
        if bad.size:
            raise Mechanism(it, int(bad[0]), float(diag[bad[0]]))
        rhs = f - gl.f_int(nodes, el, u, ea_now, dim, e0=e0)
        du = np.zeros(n)
        du[free] = linear_solve(gl.restrict(K, free), rhs[free])
        u = u + du
        if np.linalg.norm(du) / max(np.linalg.norm(u), min_den) <= tol and not changed:
            done = True
            break
    return u, it, done, slack_set(nodes, el, u, dim, cable, e0)[0], changes


def incremental_cable(nodes, el, loads, fixed, ea, dim, cable, n_inc, **kw):
    """solve()'s driver: n_inc equal load steps, each started from the last with a fresh set.  Returns (u, slack, iterations
    per increment)."""
    u, slack, its = None, None, []
    for k in range(1, n_inc + 1):
        u, it, ok, slack, _ = newton_cable(nodes, el, loads, fixed, ea, dim, cable, lam=k / n_inc, u0=u, **kw)
        assert ok, f"reference active-set Newton did not converge in increment {k}"
        its.append(it)
    return u, slack, its


def xbraced_girder(n_panels):
    """Counter-braced cantilever: nodes (i, 0) (id 2 i) and (i, 1) (id 2 i + 1) for i = 0 .. n, both nodes at i = 0 fixed.  Per
    panel a bottom chord, a top chord, the vertical at i + 1 and two diagonals; both diagonals are flagged.  A unit downward
    load on the last top node.  Returns (nodes, el, unit loads, fixed, tip dof, cable flags)."""
    n = int(n_panels)
    nodes = np.zeros((2 * (n + 1), 2))
    nodes[0::2, 0] = nodes[1::2, 0] = np.arange(n + 1)
    nodes[1::2, 1] = 1.0
    el, cable = [], []
    for i in range(n):
        b0, t0, b1, t1 = 2 * i, 2 * i + 1, 2 * i + 2, 2 * i + 3
        el += [(b0, b1), (t0, t1), (b1, t1), (b0, t1), (t0, b1)]
        cable += [False, False, False, True, True]
    loads = np.zeros(nodes.size)
    tip = 2 * (2 * n + 1) + 1
    loads[tip] = -1.0
    return nodes, np.array(el), loads, np.array([0, 1, 2, 3]), tip, np.array(cable)


# the tip loads at which the girders come down by 5 % of their span (found with newton_cable; the host test checks them)
GIRDER_LOADS = {8: 1.0677, 64: 0.018283}


def bilinear_1d():
    """Nodes 0, 1, 2 at x = 0, 1, 2, both ends fixed; element 0-1 a bar, element 1-2 a cable.  Returns (x, el, fixed, cable)."""
    return np.array([0.0, 1.0, 2.0]), np.array([[0, 1], [1, 2]]), np.array([0, 2]), np.array([False, True])
