"""Elastoplastic Green-Lagrange truss elements in numpy / scipy float64: gl_reference's element with one-dimensional
rate-independent plasticity and linear isotropic hardening, written in the Green-Lagrange strain and its conjugate force
(DESIGN.md §7), a Newton loop from a committed state with the closing evaluation, and a walk along a list of load factors
that commits after every increment.  Written from the model's statement on gl_reference's element; it shares no code with
the kernels or with pinn_fem_amd/fem.  tests/test_gl_plastic_host.py pins it to finite differences and closed forms.

Per element, with ey the yield strain, kappa = H / E and the committed (ep_n, al_n):
  se = e - e0,  tr = se - ep_n,  r = ey + kappa al_n,  f = |tr| - r,  plastic <=> f > threshold r  (threshold 2^-40)
  dg = f / (1 + kappa),  sg = sign(tr),  ep = ep_n + dg sg,  al = al_n + dg,  s = tr - dg sg        (where plastic)
  N = E A s,  fe = (N / l0) d,  B = (E A_t / l0^3) d d^T + (N / l0) I,  E A_t = E A kappa / (1 + kappa)  (where plastic)
"""
import numpy as np
import scipy.sparse.linalg as spla

import gl_reference as gl

THRESHOLD = 2.0 ** -40
EY = 1e-3                                   # the yield strain of every case here
MARGIN = 1e-6                               # the margin condition: |f - threshold r| >= MARGIN ey on every element


def _per_element(v, ne):
    return np.array(np.broadcast_to(np.asarray(v, dtype=np.float64), (ne,)))


def element_state_plastic(nodes, el, u, ea, dim, ey, kappa, ep_n=0.0, al_n=0.0, e0=None, threshold=THRESHOLD,
                          tangent="consistent"):
    """(strain [ne] (the total strain e), fe [ne, dim], B [ne, dim, dim], ep [ne], al [ne], plastic bool [ne], terms).
    terms: gl_reference.element_state's, and tr, r, f, s, ea_t of the return map.  tangent = "elastic" keeps E A in the
    material term of B where the element is plastic: the mutant the consistent-tangent test must reject."""
    strain, _, _, t = gl.element_state(nodes, el, u, ea, dim, e0)
    ne = len(strain)
    ey, kappa, ep_n, al_n = (_per_element(v, ne) for v in (ey, kappa, ep_n, al_n))
    se = strain - t["e0"] if e0 is not None else strain
    tr = se - ep_n
    r = ey + kappa * al_n
    f = np.abs(tr) - r
    plastic = f > threshold * r
    with np.errstate(invalid="ignore"):
        dg = np.where(plastic, f / (1.0 + kappa), 0.0)
    sg = np.where(tr < 0.0, -1.0, 1.0)
    ep = np.where(plastic, ep_n + dg * sg, ep_n)
    al = np.where(plastic, al_n + dg, al_n)
    s = np.where(plastic, tr - dg * sg, tr)
    ea_t = np.where(plastic, t["ea"] * kappa / (1.0 + kappa), t["ea"])
    n_l0 = (t["ea"] * s) / t["l0"]
    d = t["d"]
    fe = n_l0[:, None] * d
    k = (t["ea"] if tangent == "elastic" else ea_t) / (t["l02"] * t["l0"])
    B = k[:, None, None] * (d[:, :, None] * d[:, None, :]) + n_l0[:, None, None] * np.eye(dim)
    return strain, fe, B, ep, al, plastic, dict(t, tr=tr, r=r, f=f, s=s, ea_t=ea_t, n=t["ea"] * s, kappa=kappa, ey=ey)


def yield_margin(nodes, el, u, dim, ey, kappa, ep_n=0.0, al_n=0.0, e0=None, threshold=THRESHOLD):
    """min over the elements of |f - threshold r| / ey: how far the nearest element is from changing its branch.  The
    margin condition of the device tests is yield_margin >= MARGIN (elements that never yield, ey = inf, do not count)."""
    t = element_state_plastic(nodes, el, u, 1.0, dim, ey, kappa, ep_n, al_n, e0, threshold)[6]
    finite = np.isfinite(t["ey"])
    if not finite.any():
        return np.inf
    return float(np.min(np.abs(t["f"] - threshold * t["r"])[finite] / t["ey"][finite]))


def _scatter_state(nodes, el, dim, fe, B):
    X, el = gl._as2d(nodes, dim), np.asarray(el, dtype=np.int64)
    return gl._scatter(len(X), dim, el, fe, -1.0), gl.blocks_csr(B, el, len(X), dim)


def f_int_plastic(nodes, el, u, ea, dim, ey, kappa, ep_n=0.0, al_n=0.0, e0=None, **kw):
    st = element_state_plastic(nodes, el, u, ea, dim, ey, kappa, ep_n, al_n, e0, **kw)
    return _scatter_state(nodes, el, dim, st[1], st[2])[0]


def k_t_plastic(nodes, el, u, ea, dim, ey, kappa, ep_n=0.0, al_n=0.0, e0=None, **kw):
    st = element_state_plastic(nodes, el, u, ea, dim, ey, kappa, ep_n, al_n, e0, **kw)
    return _scatter_state(nodes, el, dim, st[1], st[2])[1]


class Mechanism(Exception):
    """A free dof with a non-positive tangent diagonal: only yielding elements hold it.  iteration counts from 1."""

    def __init__(self, iteration, dof, value):
        super().__init__(f"iteration {iteration}: diagonal {value:g} at free dof {dof}")
        self.iteration, self.dof, self.value = iteration, dof, value


def newton_plastic(nodes, el, loads, fixed, ea, dim, ey, kappa, ep_n=0.0, al_n=0.0, lam=1.0, u0=None, tol=1e-10, max_iter=50,
                   min_den=1e-10, linear_solve=spla.spsolve, e0=None, threshold=THRESHOLD):
    """gl_reference.newton's loop with the plastic element: every iteration evaluates the state at u from the committed
    (ep_n, al_n), never from the iterate before, and stops on |du| / max(|u|, min_den) <= tol alone.  The closing
    evaluation at the final u gives the state to commit.  A free dof with a tangent diagonal <= 0 raises Mechanism.
    Returns (u, iterations, converged, ep, al, plastic at the final u)."""
    n = len(gl._as2d(nodes, dim)) * dim
    free = gl.free_mask(n, fixed)
    f = lam * np.asarray(loads, dtype=np.float64).reshape(-1)
    u = np.zeros(n) if u0 is None else np.where(free, np.asarray(u0, dtype=np.float64).reshape(-1), 0.0)
    args = (ea, dim, ey, kappa, ep_n, al_n, e0, threshold)
    done, it = False, 0
    for it in range(1, max_iter + 1):
        st = element_state_plastic(nodes, el, u, *args)
        f_int, K = _scatter_state(nodes, el, dim, st[1], st[2])
        diag = K.diagonal()
        bad = np.flatnonzero(free & ~(diag > 0.0))
        if bad.size:
            raise Mechanism(it, int(bad[0]), float(diag[bad[0]]))
        du = np.zeros(n)
        du[free] = linear_solve(gl.restrict(K, free), (f - f_int)[free])
        u = u + du
        if np.linalg.norm(du) / max(np.linalg.norm(u), min_den) <= tol:
            done = True
            break
    st = element_state_plastic(nodes, el, u, *args)
    return u, it, done, st[3], st[4], st[5]


def load_program(nodes, el, loads, fixed, ea, dim, ey, kappa, load_factors, e0=None, **kw):
    """solve()'s driver with load_factors: one newton_plastic per load factor, started from the last increment's u and
    committed state.  Returns one dict per increment: load_factor, u, ep, al, yielding (bool), iterations, converged; an
    increment that does not converge is the last one and commits nothing."""
    ne = len(el)
    u, ep, al, out = None, np.zeros(ne), np.zeros(ne), []
    for lam in load_factors:
        u, it, ok, ep_new, al_new, plastic = newton_plastic(nodes, el, loads, fixed, ea, dim, ey, kappa, ep, al, lam=lam, u0=u,
                                                            e0=e0, **kw)
        if ok:
            ep, al = ep_new, al_new
        out.append(dict(load_factor=float(lam), u=u, ep=ep, al=al, yielding=plastic, iterations=it, converged=ok))
        if not ok:
            break
    return out


# ---- cases ----------------------------------------------------------------------------------------------------------
class ThreeBar:
    """The textbook three-bar truss: a centre bar of length L and two bars at 45 degrees to it, all hung from a rigid
    support and meeting in one free node, E A = ea for all, the load P pulling along the centre bar.  Small-strain closed
    forms, with N_y = ea ey: elastic N_centre = P / (1 + 1 / sqrt 2); first yield (the centre bar) at P = N_y (1 + 1 / sqrt 2);
    collapse at P_c = N_y (1 + sqrt 2), which is load factor 1 here, so first yield is at 1 / sqrt 2; after unloading from
    P_max the centre bar keeps N_y - P_max / (1 + 1 / sqrt 2) (compression)."""

    def __init__(self, L=1.0, ea=1000.0, ey=EY):
        self.L, self.ea, self.ey, self.n_y = float(L), float(ea), float(ey), float(ea) * float(ey)
        self.nodes = np.array([[-L, L], [0.0, L], [L, L], [0.0, 0.0]])
        self.el = np.array([[0, 3], [1, 3], [2, 3]])
        self.fixed = np.arange(6)
        self.p_collapse = self.n_y * (1.0 + np.sqrt(2.0))
        self.loads = np.zeros(8)
        self.loads[7] = -self.p_collapse
        self.first_yield = 1.0 / np.sqrt(2.0)

    def centre_force_elastic(self, lam):
        return lam * self.p_collapse / (1.0 + 1.0 / np.sqrt(2.0))

    def centre_residual(self, lam_max):
        return self.n_y - lam_max * self.p_collapse / (1.0 + 1.0 / np.sqrt(2.0))


THREE_BAR_PROGRAM = [0.2, 0.4, 0.6, 0.7, 0.8, 0.9, 0.97, 0.5, 0.0, -0.5, 0.0, 0.97]
WARREN_PROGRAM = [0.5, 1.0, 1.2, 1.4, 1.6, 0.8, 0.0]
WARREN_KAPPA = 0.1


def warren_first_yield(n_panels=8, ea=1000.0, ey=EY):
    """(nodes, el, loads at the first-yield tip load, fixed, tip dof) of gl_reference.cantilever_warren.  The first-yield
    tip load is the small-displacement one: the load at which the most strained element of the linear solution (the
    tangent at u = 0) reaches |eps| = ey.  The girder softens as it comes down, so at load factor 1 the Green-Lagrange
    solution has that element past yield by 8e-4 ey: far from the branch point on either side of round-off."""
    nodes, el, unit, fixed, tip = gl.cantilever_warren(n_panels)
    free = gl.free_mask(nodes.size, fixed)
    u = np.zeros(nodes.size)
    u[free] = spla.spsolve(gl.restrict(gl.k_t(nodes, el, u, ea, 2), free), unit[free])
    d0 = nodes[el[:, 1]] - nodes[el[:, 0]]
    du = u.reshape(-1, 2)[el[:, 1]] - u.reshape(-1, 2)[el[:, 0]]
    eps = np.sum(d0 * du, axis=1) / np.sum(d0 * d0, axis=1)
    return nodes, el, (ey / float(np.max(np.abs(eps)))) * unit, fixed, tip


def bar_1d(l0=2.0):
    """One bar of length l0 along x, fixed at node 0: (x, el, fixed)."""
    return np.array([0.0, l0]), np.array([[0, 1]]), np.array([0])


def bar_1d_force(ea, ey, kappa, e):
    """N of a virgin bar in monotonic tension at the strain e >= ey: E A (ey + kappa e) / (1 + kappa)."""
    return ea * (ey + kappa * e) / (1.0 + kappa)


def seeded_field(S_nodes, S_el, dim, rng, amplitude=5e-3):
    """Displacements with |du| / l0 up to about `amplitude`: each node moves by at most amplitude / 2 of the shortest
    element's length in every component."""
    X = gl._as2d(S_nodes, dim)
    el = np.asarray(S_el, dtype=np.int64)
    l_min = float(np.min(np.linalg.norm(X[el[:, 1]] - X[el[:, 0]], axis=1)))
    return rng.uniform(-1.0, 1.0, X.size) * (amplitude * l_min / (2.0 * np.sqrt(dim)))


def seeded_state(ne, rng, ey=EY):
    """A non-zero committed state: ep in +-0.8 ey, al >= |ep| (al is the path length of ep), a fifth of the elements virgin."""
    ep = rng.uniform(-0.8, 0.8, ne) * ey
    al = np.abs(ep) + rng.uniform(0.0, 0.5, ne) * ey
    virgin = rng.random(ne) < 0.2
    return np.where(virgin, 0.0, ep), np.where(virgin, 0.0, al)


def kappa_case(name, ne, rng):
    return {"0": np.zeros(ne), "0.05": np.full(ne, 0.05), "per-element": rng.uniform(0.0, 0.5, ne)}[name]
