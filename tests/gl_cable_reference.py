"""Tension-only (cable) elements in the explicit dynamics of the Green-Lagrange truss, in numpy float64: the restatement of
gl_dynamics_reference.Truss with a per-element flag.  A flagged element with e - e0 < 0 is slack: N = 0, no force, no
strain energy.  Written from the rule's statement; it shares no code with the kernels or with
pinn_fem_amd/fem/dynamics.py.  step, start, run, f_int (both summation orders) and f_int_scale are the base class's: a slack
element's force is 0.0 and is summed in its place.  tests/test_gl_cable_host.py pins it to closed forms.
"""
import numpy as np

import gl_dynamics_reference as gd
import gl_reference as gl


class CableTruss(gd.Truss):
    """gd.Truss with cable: bool [n_elems] (or a scalar for all), True = tension-only."""

    def __init__(self, nodes, el, fixed, dim, ea, e0, mass, loads=None, cable=False):
        super().__init__(nodes, el, fixed, dim, ea, e0, mass, loads)
        self.cable = np.broadcast_to(np.asarray(cable, dtype=bool), (self.ne,)).copy()

    def slack(self, u):
        """bool [n_elems]: flagged and e - e0 < 0."""
        return self.cable & (self.strain(u)[0] - self.e0 < 0.0)

    def element_force(self, u):
        e, d, _ = self.strain(u)
        se = e - self.e0
        n_l0 = np.where(self.cable & (se < 0.0), 0.0, (self.ea * se) / self.l0)
        return n_l0[:, None] * d

    def energies(self, u, v):
        """(kinetic, strain energy without the slack elements, f_ext.u, max |v|, the number of slack elements)."""
        kin, _, work, vmax = super().energies(u, v)
        se = self.strain(u)[0] - self.e0
        taut = ~self.slack(u)
        return (kin, float(np.sum(0.5 * self.ea[taut] * self.l0[taut] * se[taut] ** 2)), work, vmax, int(np.sum(~taut)))

    def beta(self, u):
        """gd.Truss.beta with e clipped at e0 on the flagged elements: a slack cable counts with its taut, stress-free block
        E A (1 + 2 e0) / l0, which bounds its block in every state between slack and e0."""
        e, _, _ = self.strain(u)
        e = np.where(self.cable, np.maximum(e, self.e0), e)
        n_l0 = self.ea * (e - self.e0) / self.l0
        return np.maximum(np.abs(n_l0), np.abs(n_l0 + self.ea * (1.0 + 2.0 * e) / self.l0))

    def omega_active(self, u):
        """The highest frequency of K_t v = omega^2 M v on the free dofs with the slack elements' blocks zeroed (dense)."""
        import scipy.linalg
        ea = np.where(self.slack(u), 0.0, self.ea)
        K = gl.restrict(gl.k_t(self.X, self.el, u, ea, self.dim, e0=self.e0), self.free).toarray()
        return float(np.sqrt(max(scipy.linalg.eigvalsh(K, np.diag(self.mass[self.free]))[-1], 0.0)))

    def state_changes(self, u, v, n0, n_steps, dt, **kw):
        """run() that also returns the steps n at which slack(u_n) differs from slack(u_{n-1}) and the elements that ever
        changed: (u, v, [n], bool [n_elems])."""
        was, at, ever = self.slack(u), [], np.zeros(self.ne, dtype=bool)
        for k in range(n_steps):
            u, v = self.step(u, v, n0 + k, dt, **kw)
            now = self.slack(u)
            if (now != was).any():
                at.append(n0 + k + 1)
                ever |= now != was
            was = now
        return u, v, at, ever


def with_cables(T, cable):
    """The data of a gd.Truss as a CableTruss."""
    return CableTruss(T.X, T.el, np.flatnonzero(~T.free), T.dim, T.ea, T.e0, T.mass, T.loads, cable)


def seeded_half(n_elems, seed=7):
    """bool [n_elems]: about half the elements flagged, the draw the host and the device tests share."""
    return np.random.default_rng(seed).random(n_elems) < 0.5


def guyed_mast(load=2.0, cable=(False, True, True), elements=(0, 1, 2)):
    """tests/nl_inputs/guyed_mast_slack.json: a mast (bar 0-1) and two pretensioned guys 2-1, 3-1 under a side load at the
    top; `elements` picks a sub-structure.  Returns (CableTruss, nodes, el, fixed, e0 of the picked elements)."""
    nodes = np.array([[0.0, 0.0], [0.0, 4.0], [-3.0, 0.0], [3.0, 0.0]])
    pick = list(elements)
    el = np.array([[0, 1], [2, 1], [3, 1]])[pick]
    e0 = np.array([0.0, -1e-3, -1e-3])[pick]
    fixed = np.array([0, 1, 4, 5, 6, 7])
    loads = np.zeros(8)
    loads[2] = load
    mass = gd.lumped_mass(nodes, np.array([[0, 1], [2, 1], [3, 1]]), 0.5, 2)
    return CableTruss(nodes, el, fixed, 2, 1000.0, e0, mass, loads, np.asarray(cable)[pick]), nodes, el, fixed, e0


def one_cable(load):
    """tests/nl_inputs/cable_free_flight.json: 1-D, nodes 0 and 1, node 0 fixed, one flagged element, E A = 1000, node mass
    0.25."""
    nodes, el = np.array([0.0, 1.0]), np.array([[0, 1]])
    return CableTruss(nodes, el, np.array([0]), 1, 1000.0, None, gd.lumped_mass(nodes, el, 0.5, 1), np.array([0.0, load]), True)
