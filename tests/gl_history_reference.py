"""Load and support-motion time histories in the explicit dynamics of the Green-Lagrange truss, in numpy float64: the
restatement of the rules of DESIGN.md §7 on top of gl_dynamics_reference.Truss (or gl_cable_reference.CableTruss: whatever has
f_int, free, mass and loads).  It shares no code with the kernels or with pinn_fem_amd/fem/dynamics.py.
tests/test_gl_history_host.py pins it to a closed form (a uniformly accelerated frame).

  a history is sampled at the step times t_n = n dt, once; step n reads sample i(n) = min(n, n_samples - 1)
  lam = lam_samples[i(n)], or the ramp where no load history is given
  a fixed dof with an amplitude a != 0.0 gets u_{n+1} = a sup_samples[i(n + 1)]; every other fixed dof gets 0.0; v = 0.0 on both
"""
import numpy as np

import gl_dynamics_reference as gd


def history_value(t, times, values):
    """The piecewise-linear history through the knots (times strictly increasing) at one time t: the first value up to the
    first knot, the last value beyond the last, and on t_j < t <= t_{j+1}
    v_j + (v_{j+1} - v_j) ((t - t_j) / (t_{j+1} - t_j))."""
    if t <= times[0]:
        return float(values[0])
    if t > times[-1]:
        return float(values[-1])
    j = 0
    while times[j + 1] < t:
        j += 1
    return float(values[j] + (values[j + 1] - values[j]) * ((t - times[j]) / (times[j + 1] - times[j])))


def step_times(n_samples, dt):
    return np.array([n * dt for n in range(n_samples)])


def sample(history, n_samples, dt):
    """A history at the step times: a pair (times, values) through history_value, or a callable of the array of times."""
    t = step_times(n_samples, dt)
    if callable(history):
        return np.asarray(history(t), dtype=np.float64)
    times, values = (np.asarray(a, dtype=np.float64) for a in history)
    return np.array([history_value(x, times, values) for x in t])


def held(samples, n):
    """Sample i(n): a step beyond the table reads the last one."""
    return float(samples[min(n, len(samples) - 1)])


def supports(T, sup, n):
    """u_n on the fixed dofs, 0.0 elsewhere: amp * s[i(n)] where amp != 0.0, the bytes of 0.0 where it is."""
    out = np.zeros(T.n)
    if sup is not None:
        amp, samples = sup
        s = held(samples, n)
        moved = ~T.free & (np.asarray(amp) != 0.0)
        out[moved] = np.asarray(amp, dtype=np.float64)[moved] * s
    return out


def step(T, u, v, n, dt, alpha=0.0, lam=None, sup=None, ramp=(1.0, 1.0, 0.0), c1=None, g=None, descending=False):
    """(u_{n+1}, v_{n+1/2}) from (u_n, v_{n-1/2}).  lam: the load samples or None (the ramp (lam0, lam1, t_ramp)); sup: (amp
    [n_dofs], samples) or None; c1, g: the start's coefficients in place of the step's."""
    h = 0.5 * alpha * dt
    c1 = (1.0 - h) / (1.0 + h) if c1 is None else c1
    g = dt / (1.0 + h) if g is None else g
    lam_n = held(lam, n) if lam is not None else gd.load_factor(n * dt, *ramp)
    r = lam_n * T.loads - T.f_int(u, descending)
    v_new = np.where(T.free, c1 * v + g * (r / T.mass), 0.0)
    return np.where(T.free, u + dt * v_new, supports(T, sup, n + 1)), v_new


def start(T, u0, v0, dt, alpha=0.0, **kw):
    """(u_1, v_{1/2}) from (u_0, v_0): the step with c1 = 1 - alpha dt/2 and g = dt/2, lam[0] and the supports of step 1."""
    return step(T, u0, v0, 0, dt, alpha, c1=1.0 - 0.5 * alpha * dt, g=0.5 * dt, **kw)


def run(T, u, v, n0, n_steps, dt, **kw):
    for k in range(n_steps):
        u, v = step(T, u, v, n0 + k, dt, **kw)
    return u, v


def solve(T, dt, n_steps, alpha=0.0, lam=None, sup=None, u0=None, descending=False):
    """The run of solve_dynamic from rest: u_0 with the supports at amp s(0), the start, then n_steps - 1 steps.  Returns
    (u, v) at step n_steps."""
    u = np.zeros(T.n) if u0 is None else np.array(u0, dtype=np.float64)
    u = np.where(T.free, u, supports(T, sup, 0))
    u, v = start(T, u, np.zeros(T.n), dt, alpha, lam=lam, sup=sup, descending=descending)
    return run(T, u, v, 1, n_steps - 1, dt, alpha=alpha, lam=lam, sup=sup, descending=descending)
