"""Initial (eigen-) strains in the Green-Lagrange truss element: the closed forms, meshes and the prestressed girder the
tests pin the element (tests/gl_reference.py, every function's e0 keyword) and the identification on a prestressed
structure (tests/identify_reference.py) to.  It shares no code with the kernels or with pinn_fem_amd/fem.
tests/test_gl_e0_host.py checks the element with e0 against finite differences and these closed forms.

  W(u) = sum_e  E A l0 (e - e0)^2 / 2,   e = (|d|^2 - |d0|^2) / (2 l0^2),  d = d0 + du
  N = E A (e - e0),   fe = (N / l0) d,   B = (E A / l0^3) d d^T + (N / l0) I
e0 < 0 is a pretension (T = -E A e0), thermal loading is e0 = alpha dT, lack of fit e0 = (L_natural - l0) / l0.  e0 acts
in full at every load factor.
"""
import functools

import numpy as np

import gl_reference as gl
import identify_reference as ir


# ---- closed forms and meshes -----------------------------------------------------------------------------------------
class TautString:
    """Two collinear bars between supports at (-a, 0) and (a, 0), both with E*A = ea and the initial strain e0, load P
    across at the middle node.  With the middle's deflection w:  e = w^2 / (2 a^2),  N = ea (e - e0),
    P(w) = 2 N w / a."""

    def __init__(self, a=1.0, ea=1000.0, e0=-1e-3):
        self.a, self.ea, self.e0 = float(a), float(ea), float(e0)
        self.nodes = np.array([[-a, 0.0], [0.0, 0.0], [a, 0.0]])
        self.el = np.array([[0, 1], [1, 2]])
        self.fixed = np.array([0, 1, 4, 5])

    def strain(self, w):
        return w * w / (2.0 * self.a ** 2)

    def force(self, w):
        return self.ea * (self.strain(w) - self.e0)

    def load(self, w):
        return 2.0 * self.force(w) * w / self.a

    def loads(self, p):
        out = np.zeros(6)
        out[3] = p
        return out


class PrestressedTwoBar(gl.TwoBar):
    """gl.TwoBar with the initial strain e0 in both bars.  With the apex drop w:  e = (w^2 - 2 h w) / (2 l0^2),
    P(w) = E A ((w^2 - 2 h w) / (2 l0^2) - e0) (w - h) 2 / l0,  dP/dw = (2 E A / l0) ((3 (w - h)^2 - h^2) / (2 l0^2) - e0):
    the limit point is at w = h - sqrt((h^2 + 2 l0^2 e0) / 3) (a pretension beyond e0 = -h^2 / (2 l0^2) removes it), and
    the unloaded apex already sits at P(w) = 0 below w = 0 for e0 < 0."""

    def __init__(self, a=10.0, h=1.0, ea=1000.0, e0=-1e-3):
        self.e0 = float(e0)
        super().__init__(a, h, ea)
        self.w_lim = self.h - np.sqrt((self.h ** 2 + 2.0 * self.l0 ** 2 * self.e0) / 3.0)
        self.p_lim = self.load(self.w_lim)

    def tangent(self, w):
        return 2.0 * self.ea / self.l0 * ((3.0 * (w - self.h) ** 2 - self.h ** 2) / (2.0 * self.l0 ** 2) - self.e0)

    def load(self, w):
        return self.ea * (self.strain(w) - self.e0) * (w - self.h) * 2.0 / self.l0 ** 3 * self.l0 ** 2


def cable_chain(n, ea=1000.0, e0=-1e-2, sag=0.02):
    """n collinear unit elements between two supports with the pretension -ea e0 and equal loads across at every inner node:
    the load of a parabolic cable with a sag of `sag` of the span under that pretension, p = 8 T sag / n.
    Returns (nodes, el, loads, fixed)."""
    nodes = np.zeros((n + 1, 2))
    nodes[:, 0] = np.arange(n + 1)
    e = np.arange(n)
    el = np.stack([e, e + 1], axis=1)
    loads = np.zeros(2 * (n + 1))
    loads[3:2 * n:2] = -8.0 * (-ea * e0) * sag / n
    return nodes, el, loads, np.array([0, 1, 2 * n, 2 * n + 1])


def heated_bar(n, h=0.75):
    """1-D chain of n equal elements between two supports.  Returns (x, el, fixed)."""
    x = h * np.arange(n + 1)
    e = np.arange(n)
    return x, np.stack([e, e + 1], axis=1), np.array([0, n])


# ---- the prestressed girder ----------------------------------------------------------------------------------------------
E0_AMPLITUDE = 1e-3


@functools.lru_cache(maxsize=None)
def warren_case(n_panels=8, amplitude=E0_AMPLITUDE, seed=0):
    """ir.warren_case(n_panels) (geometry, loads, groups and true factors) with a random initial strain in +-amplitude in
    every element and the measurements generated WITH it: every free dof at every load level.  The case carries e0."""
    base = ir.warren_case(n_panels)
    e0 = np.random.default_rng(seed).uniform(-amplitude, amplitude, len(base.el))
    idx = np.flatnonzero(gl.free_mask(len(base.loads), base.fixed))
    levels = ir.measure(base.nodes, base.el, base.loads, base.fixed, base.ea0 * base.factors[base.groups],
                        [lv[0] for lv in base.levels], idx, e0=e0)
    return ir.Case(base.nodes, base.el, base.loads, base.fixed, base.tip, base.ea0, base.groups, base.factors, levels, e0=e0)


@functools.lru_cache(maxsize=None)
def reference_run(with_prestress=True):
    """(case, ir.identify_factors(case, misfit_tolerance=1e-15)) on warren_case() from all factors 1, with the case's
    initial strain in the model or (with_prestress False) left out of it: computed once, shared by the tests."""
    case = warren_case()
    return case, ir.identify_factors(case, e0=case.e0 if with_prestress else 0.0, misfit_tolerance=1e-15)
