"""Identification of E*A factors from strain-gauge data: the cases whose levels carry gauges and the two-bar closed form
the tests pin tests/identify_reference.py's misfit, residuals and loop (every level's gauges) and tests/gl_reference.py's
B = d e / d u (strains, bt_c, b_v and their magnitude sums) to.  It shares no code with the kernels or with
pinn_fem_amd/fem/identify.py.

  J   = sum_k [ mean_m (u_k[m] - ubar_k[m])^2 + L_k^2 mean_i (e_k[elem_i] - ebar_ki)^2 ]
  rho = per level (u_k[m_k] - ubar_k) / sqrt|m_k|, then L_k (e - ebar) / sqrt p_k;   J = rho.rho
"""
import functools
from dataclasses import dataclass

import numpy as np

import gl_reference as gl
import identify_reference as ir

STRAIN_SCALE = 8.0                   # the span of warren_case(8)


# ---- cases ---------------------------------------------------------------------------------------------------------------
@dataclass
class StrainCase(ir.Case):
    """identify_reference.Case whose levels (ascending load factor) carry gauges: gauges[k] = (elements, strains, scale) or
    None beside levels[k] = (load factor, dofs, values), dofs possibly empty."""

    def dict_levels(self):
        """The levels as identify_nr takes them."""
        out = []
        for (lam, dofs, ubar), gauge in zip(self.levels, self.gauges):
            lv = {"load_factor": lam, "dofs": np.asarray(dofs, dtype=np.int64), "u": np.asarray(ubar, dtype=np.float64)}
            if gauge is not None:
                lv.update(strain_elements=np.asarray(gauge[0], dtype=np.int64), strains=np.asarray(gauge[1]),
                          strain_scale=gauge[2])
            out.append(lv)
        return out

    @property
    def n_rows(self):
        return sum(len(lv[1]) for lv in self.levels) + sum(len(g[0]) for g in self.gauges if g is not None)


def gauge_elements(groups, n_groups, per_group=1):
    """The per_group lowest-numbered elements of every group, in group order."""
    groups = np.asarray(groups, dtype=int)
    return np.concatenate([np.flatnonzero(groups == g)[:per_group] for g in range(n_groups)])


@functools.lru_cache(maxsize=None)
def strain_case(n_groups, gauges_per_group=1, tip=False):
    """case_with_groups(n_groups) measured by strain gauges: at every load level the Green-Lagrange strains of the
    gauges_per_group lowest-numbered elements of every span group, on the structure with the true factors (its states are the
    base case's measurements of every free dof), with strain scale 8.0 (the span); tip: the tip dof as the one displacement
    row of every level, otherwise no displacement data."""
    base = ir.case_with_groups(n_groups)
    elements = gauge_elements(base.groups, base.n_groups, gauges_per_group)
    levels, gauges = [], []
    for lam, dofs, ubar in sorted(base.levels, key=lambda lv: lv[0]):
        u = np.zeros(len(base.loads))
        u[dofs] = ubar
        e = gl.strains(base.nodes, base.el, u, 2)
        m = np.array([base.tip]) if tip else np.zeros(0, dtype=int)
        levels.append((lam, m, u[m].copy()))
        gauges.append((elements.copy(), e[elements].copy(), STRAIN_SCALE))
    return StrainCase(base.nodes, base.el, base.loads, base.fixed, base.tip, base.ea0, base.groups, base.factors, levels,
                      gauges)


@functools.lru_cache(maxsize=None)
def reference_run(n_groups, tip=False):
    """(case, ir.identify_factors(case, misfit_tolerance=1e-15)) from all factors 1: computed once and shared."""
    case = strain_case(n_groups, tip=tip)
    return case, ir.identify_factors(case, misfit_tolerance=1e-15)


@functools.lru_cache(maxsize=None)
def reference_recovery(tip=False):
    """(case, factors, evaluations) of identify_reference.recover on strain_case(4, tip=tip) from all factors 1."""
    case = strain_case(4, tip=tip)
    factors, evaluations, _ = ir.recover(case)
    return case, factors, evaluations


# ---- the two-bar closed form ---------------------------------------------------------------------------------------------
def two_bar_closed_form(tb, p, w, e_bar, scale):
    """dJ/d(ea) of J = L^2 (e(w) - e_bar)^2 (both bars carry e(w) = (w^2 - 2 h w) / (2 l0^2)) at fixed load P with both
    bars at ea: de/dw = (w - h) / l0^2 and dw/d(ea) = -P / (ea * tangent(w))."""
    return 2.0 * scale * scale * (tb.strain(w) - e_bar) * ((w - tb.h) / tb.l0 ** 2) * (-p / (tb.ea * tb.tangent(w)))


def two_bar_bound(tb, w, e_bar, tol):
    """identify_reference.two_bar_bound's reasoning for the strain misfit: the Newton loop stops at |du| <= tol |u|, so w is
    off by at most tol * w, which enters (e(w) - e_bar) through de/dw, de/dw = (w - h) / l0^2 itself, and tangent(w):
    tol w (|de/dw| / |e - e_bar| + 1 / |w - h| + |tangent'| / |tangent|), as much again for the adjoint gradient, which is
    formed at the same iterate; plus 1e-12 for the round-off of both."""
    d_tangent = tb.ea * (6.0 * w - 6.0 * tb.h) / tb.l0 ** 3
    de_dw = (w - tb.h) / tb.l0 ** 2
    return 2.0 * tol * w * (abs(de_dw) / abs(tb.strain(w) - e_bar) + 1.0 / abs(w - tb.h)
                            + abs(d_tangent / tb.tangent(w))) + 1e-12
