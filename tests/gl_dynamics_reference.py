"""Explicit dynamics of the Green-Lagrange truss element in numpy float64: lumped masses, the central-difference step with
its half-kick start, the energies, the bound on the highest frequency and the closed forms the tests pin the scheme to.
Written from the scheme's statement; it shares no code with the kernels.  The internal force is summed per
node over the node's incidences one after the other, in ascending order of the incidence codes (element id << 1 | end), as
the device does, or on request in descending order: the difference of the two is the restatement's own summation spread.
tests/test_gl_dynamics_host.py pins it to the closed forms.

  m_i = sum_{e at i} rho A l0_e / 2 (+ an added nodal mass), the same for every dof of the node
  v_{n+1/2} = c1 v_{n-1/2} + g (lam(t_n) f_ext - f_int(u_n)) / m,   u_{n+1} = u_n + dt v_{n+1/2}
  c1 = (1 - alpha dt/2) / (1 + alpha dt/2),  g = dt / (1 + alpha dt/2);   the start: c1 = 1 - alpha dt/2, g = dt/2
"""
import numpy as np

import gl_reference as gl


def lumped_mass(nodes, el, rho_a, dim, nodal_mass=None):
    """Mass of every dof [n_dofs]: half of rho A l0 of every element at the dof's node, plus nodal_mass (a scalar or one
    value per node)."""
    X, el = gl._as2d(nodes, dim), np.asarray(el, dtype=np.int64)
    l0 = np.linalg.norm(X[el[:, 1]] - X[el[:, 0]], axis=1)
    half = 0.5 * np.broadcast_to(np.asarray(rho_a, dtype=np.float64), l0.shape) * l0
    m = np.zeros(len(X))
    np.add.at(m, el[:, 0], half)
    np.add.at(m, el[:, 1], half)
    if nodal_mass is not None:
        m = m + np.broadcast_to(np.asarray(nodal_mass, dtype=np.float64), m.shape)
    return np.repeat(m, dim)


def load_factor(t, lam0, lam1, t_ramp):
    return lam0 + (lam1 - lam0) * min(1.0, t / t_ramp) if t_ramp > 0.0 else lam1


class Truss:
    """One truss and its scheme.  ea, e0: scalars or [n_elems]; mass: per dof [n_dofs] (lumped_mass); loads: [n_dofs] at
    load factor 1."""

    def __init__(self, nodes, el, fixed, dim, ea, e0, mass, loads=None):
        self.dim = dim
        self.X, self.el = gl._as2d(nodes, dim), np.asarray(el, dtype=np.int64)
        self.n_nodes, self.ne = len(self.X), len(self.el)
        self.n = self.n_nodes * dim
        self.free = gl.free_mask(self.n, fixed)
        self.d0 = self.X[self.el[:, 1]] - self.X[self.el[:, 0]]
        self.l02 = np.sum(self.d0 * self.d0, axis=1)
        self.l0 = np.sqrt(self.l02)
        self.ea = np.broadcast_to(np.asarray(ea, dtype=np.float64), (self.ne,))
        self.e0 = np.broadcast_to(np.asarray(0.0 if e0 is None else e0, dtype=np.float64), (self.ne,))
        self.mass = np.asarray(mass, dtype=np.float64).reshape(-1)
        self.loads = np.zeros(self.n) if loads is None else np.asarray(loads, dtype=np.float64).reshape(-1)
        # incidences by node, ascending code: round r holds the r-th incidence of every node that has one
        codes = np.arange(2 * self.ne)
        node = self.el.reshape(-1)                        # el.reshape(-1)[2 e + end] = el[e, end]
        order = np.lexsort((codes, node))
        codes, node = codes[order], node[order]
        first = np.searchsorted(node, node, side="left")
        rank = np.arange(len(codes)) - first
        count = np.bincount(node, minlength=self.n_nodes)
        back = count[node] - 1 - rank                     # the rank counted from the node's last incidence
        self.degree = np.repeat(count, dim)
        self.rounds = {False: self._rounds(codes, node, rank), True: self._rounds(codes, node, back)}

    @staticmethod
    def _rounds(codes, node, rank):
        out = []
        for r in range(int(rank.max()) + 1 if len(rank) else 0):
            pick = rank == r
            out.append((node[pick], codes[pick] >> 1, np.where(codes[pick] & 1, 1.0, -1.0)))
        return out

    def strain(self, u):
        U = np.asarray(u, dtype=np.float64).reshape(-1, self.dim)
        du = U[self.el[:, 1]] - U[self.el[:, 0]]
        # the difference of squares written out
        return (2.0 * np.sum(self.d0 * du, axis=1) + np.sum(du * du, axis=1)) / (2.0 * self.l02), self.d0 + du, du

    def element_force(self, u):
        e, d, _ = self.strain(u)
        return ((self.ea * (e - self.e0)) / self.l0)[:, None] * d

    def f_int(self, u, descending=False):
        """The sum per node, one incidence after the other."""
        fe = self.element_force(u)
        acc = np.zeros((self.n_nodes, self.dim))
        for nodes_r, elems_r, sign_r in self.rounds[bool(descending)]:
            acc[nodes_r] = acc[nodes_r] + sign_r[:, None] * fe[elems_r]
        return acc.reshape(-1)

    def f_int_scale(self, u):
        """Per dof, the sum of the magnitudes the terms of f_int are formed from, in front of the cancellation of e - e0
        and of the sum over the node's elements (gl_e0_reference.f_int_scale's unit)."""
        U = np.asarray(u, dtype=np.float64).reshape(-1, self.dim)
        du = U[self.el[:, 1]] - U[self.el[:, 0]]
        e_abs = (2.0 * np.sum(np.abs(self.d0) * np.abs(du), axis=1) + np.sum(du * du, axis=1)) / (2.0 * self.l02)
        mag = (np.abs(self.ea) * (e_abs + np.abs(self.e0)) / self.l0)[:, None] * (np.abs(self.d0) + np.abs(du))
        out = np.zeros((self.n_nodes, self.dim))
        np.add.at(out, self.el[:, 1], mag)
        np.add.at(out, self.el[:, 0], mag)
        return out.reshape(-1)

    def step(self, u, v, n, dt, alpha=0.0, lam0=1.0, lam1=1.0, t_ramp=0.0, c1=None, g=None, descending=False):
        """(u_{n+1}, v_{n+1/2}) from (u_n, v_{n-1/2}); c1, g: the start's coefficients in place of the step's."""
        h = 0.5 * alpha * dt
        c1 = (1.0 - h) / (1.0 + h) if c1 is None else c1
        g = dt / (1.0 + h) if g is None else g
        lam = load_factor(n * dt, lam0, lam1, t_ramp)
        r = lam * self.loads - self.f_int(u, descending)
        v_new = np.where(self.free, c1 * v + g * (r / self.mass), 0.0)
        return np.where(self.free, u + dt * v_new, 0.0), v_new

    def start(self, u0, v0, dt, alpha=0.0, **kw):
        """(u_1, v_{1/2}) from (u_0, v_0): the step with c1 = 1 - alpha dt/2 and g = dt/2."""
        return self.step(u0, v0, 0, dt, alpha, c1=1.0 - 0.5 * alpha * dt, g=0.5 * dt, **kw)

    def run(self, u, v, n0, n_steps, dt, **kw):
        for k in range(n_steps):
            u, v = self.step(u, v, n0 + k, dt, **kw)
        return u, v

    def energies(self, u, v):
        """(kinetic sum m v^2 / 2, strain sum E A l0 (e - e0)^2 / 2, f_ext.u, max |v|)."""
        e = self.strain(u)[0]
        moving = v != 0.0
        return (float(np.sum(0.5 * self.mass[moving] * v[moving] ** 2)),
                float(np.sum(0.5 * self.ea * self.l0 * (e - self.e0) ** 2)),
                float(np.dot(self.loads, u)), float(np.max(np.abs(v))) if len(v) else 0.0)

    def beta(self, u):
        """Per element the larger absolute eigenvalue of its block B = (E A / l0^3) d d^T + (N / l0) I."""
        e, d, _ = self.strain(u)
        n_l0 = self.ea * (e - self.e0) / self.l0
        return np.maximum(np.abs(n_l0), np.abs(n_l0 + self.ea * np.sum(d * d, axis=1) / (self.l02 * self.l0)))

    def omega_bound(self, u):
        """sqrt(max_i 2 sum_{e at i} beta_e / m_i) over the nodes with a free dof: v^T K_t v <= sum_e 2 beta_e (|v_i|^2 +
        |v_j|^2) bounds the Rayleigh quotient."""
        b = self.beta(u)
        s = np.zeros(self.n_nodes)
        np.add.at(s, self.el[:, 0], b)
        np.add.at(s, self.el[:, 1], b)
        m = self.mass.reshape(self.n_nodes, self.dim)[:, 0]
        has_free = self.free.reshape(self.n_nodes, self.dim).any(axis=1)
        return float(np.sqrt(np.max(2.0 * s[has_free] / m[has_free])))

    def stable_time_step(self, u, safety=0.9):
        return safety * 2.0 / self.omega_bound(u)

    def omega_true(self, u):
        """The highest frequency of K_t v = omega^2 M v on the free dofs (dense)."""
        import scipy.linalg
        K = gl.restrict(gl.k_t(self.X, self.el, u, self.ea, self.dim, e0=self.e0), self.free).toarray()
        return float(np.sqrt(scipy.linalg.eigvalsh(K, np.diag(self.mass[self.free]))[-1]))


# ---- closed forms ---------------------------------------------------------------------------------------------------
def string(n_elems=8, ea=1000.0, e0=-1e-3, rho_a=0.5, half_span=1.0):
    """n collinear elements on [-half_span, half_span] with both ends held; the inner nodes are free along and across.
    Returns (Truss, h, tension)."""
    x = np.linspace(-half_span, half_span, n_elems + 1)
    nodes = np.stack([x, np.zeros_like(x)], axis=1)
    el = np.stack([np.arange(n_elems), np.arange(1, n_elems + 1)], axis=1)
    fixed = np.array([0, 1, 2 * n_elems, 2 * n_elems + 1])
    T = Truss(nodes, el, fixed, 2, ea, e0, lumped_mass(nodes, el, rho_a, 2))
    return T, 2.0 * half_span / n_elems, -ea * e0


def string_frequency(k, n_elems, tension, node_mass, h):
    """omega_k = 2 sqrt(T / (m h)) sin(k pi / (2 n)) of n - 1 equal masses on a taut string."""
    return 2.0 * np.sqrt(tension / (node_mass * h)) * np.sin(k * np.pi / (2.0 * n_elems))


def string_mode(k, n_elems, amplitude):
    """u [n_dofs] of mode k: uy_i = a sin(k pi i / n)."""
    u = np.zeros(2 * (n_elems + 1))
    u[1::2] = amplitude * np.sin(k * np.pi * np.arange(n_elems + 1) / n_elems)
    return u


def two_bar_far_root(tb, load):
    """The root of P(w) = load beyond w = 2 h (gl.TwoBar: P(w) = ea (2 h w - w^2)(h - w) / l0^3), by bisection and a Newton
    polish."""
    lo, hi = 2.0 * tb.h, 4.0 * tb.h
    while tb.load(hi) < load:
        hi *= 2.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if tb.load(mid) < load else (lo, mid)
    w = 0.5 * (lo + hi)
    for _ in range(3):
        w -= (tb.load(w) - load) / tb.tangent(w)
    return w
