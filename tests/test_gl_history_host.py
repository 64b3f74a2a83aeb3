"""Load and support-motion time histories in the explicit dynamics, CPU side: the float64 restatement of
tests/gl_history_reference.py pinned to a closed form (a uniformly accelerated frame is a uniform load), its piecewise-linear
table against the ramp it replaces, the host sampling of pinn_fem_amd/fem/dynamics.py against the restatement's, every refusal
of check_dynamics, and the JSON / ABI surface.  tests/test_gl_history_f64.py holds the device to the same restatement.
"""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import gl_dynamics_reference as gd
import gl_history_reference as gh
from helpers import ROOT
from pinn_fem_amd.fem import dynamics as dyn
from pinn_fem_amd.fem.model import FEMModel, Material
from pinn_fem_amd.fem.solver import SolverConfig

HERE = os.path.dirname(os.path.abspath(__file__))
U53 = 2.0 ** -53
YOUNG, AREA = 2000.0, 0.5


def _model(T, loads=None):
    return FEMModel(nodes=T.X, elements=T.el, material=Material(YOUNG, AREA, 1.0),
                    loads=np.zeros(T.n) if loads is None else loads, fixed_dofs=np.flatnonzero(~T.free), dimension=2)


def _config(**kw):
    return SolverConfig(method="nr", kinematics="green-lagrange", **kw)


# ---------------------------------------------------------------------------------------------------------------------
# 1. a uniformly accelerated frame
# ---------------------------------------------------------------------------------------------------------------------
def test_moving_frame_is_a_uniform_load():
    """Every support of the 8-element taut string follows u_g(t) = a t^2 / 2 across the string, sampled at the step times,
    from rest, alpha = 0.  f_int reads differences of u alone, and (u_g[n+1] - u_g[n]) / dt = a (n + 1/2) dt exactly, so
    w = u - u_g and v - a (n - 1/2) dt on the free dofs are the run with the supports at rest under the load -m a on the
    free transverse dofs.  a = 0.3, 256 steps at 0.9 of the bound: u_g = 0.25, max |w| 0.014, v_g = 0.39.  The two runs
    differ by a constant number of roundings per step on those magnitudes, growing linearly:
    <= 8 n_steps 2^-53 (|u_g| + max |w|), and the same with the velocities (measured on the CPU: 7.1e-17 against 6.0e-14 in
    u, 2.0e-15 against 1.1e-13 in v).  The string's ascending-against-descending spread is zero (two incidences per node), so
    it is no unit for this test."""
    T, _, _ = gd.string()
    a, n_steps = 0.3, 256
    dt = 0.9 * 2.0 / T.omega_bound(np.zeros(T.n))
    t = gh.step_times(n_steps + 2, dt)
    frame = gh.sample(lambda x: 0.5 * a * x * x, n_steps + 2, dt)
    assert np.array_equal(frame, 0.5 * a * t * t)
    amp = np.zeros(T.n)
    amp[[1, 2 * 8 + 1]] = 1.0                           # uy of both ends
    moving = gh.solve(T, dt, n_steps, sup=(amp, frame))
    across = np.zeros(T.n, dtype=bool)
    across[1::2] = True
    across &= T.free
    still = gd.Truss(T.X, T.el, np.flatnonzero(~T.free), 2, T.ea, T.e0, T.mass, np.where(across, -T.mass * a, 0.0))
    rest = gh.solve(still, dt, n_steps, lam=np.ones(n_steps + 2))
    u_g, v_g = frame[n_steps], a * (n_steps - 0.5) * dt
    w = moving[0] - np.where(across, u_g, 0.0)
    vr = moving[1] - np.where(across, v_g, 0.0)
    assert moving[0][1] == moving[0][17] == u_g and not moving[0][[0, 16]].any() and not moving[1][~T.free].any()
    err_u, err_v = np.max(np.abs(w - rest[0])[T.free]), np.max(np.abs(vr - rest[1])[T.free])
    bound_u = 8 * n_steps * U53 * (abs(u_g) + np.max(np.abs(rest[0])))
    bound_v = 8 * n_steps * U53 * (abs(v_g) + np.max(np.abs(rest[1])))
    print(f"moving frame: u_g {u_g:.3f}, max |w| {np.max(np.abs(rest[0])):.3e}, v_g {v_g:.3f}; u differs by {err_u:.2e} (bound "
          f"{bound_u:.2e}), v by {err_v:.2e} (bound {bound_v:.2e})")
    assert 0.2 < u_g < 0.3 and np.max(np.abs(rest[0])) > 1e-3
    assert err_u <= bound_u and err_v <= bound_v


# ---------------------------------------------------------------------------------------------------------------------
# 2. the ramp as a table
# ---------------------------------------------------------------------------------------------------------------------
def test_the_ramp_as_a_table_is_the_ramp():
    """The table [(0, lam0), (t_ramp, lam1)] through the restatement's history_value is gd.load_factor to the bit: at the
    knots, between them and beyond the last."""
    lam0, lam1, t_ramp = 0.25, 1.5, 0.7
    times, values = np.array([0.0, t_ramp]), np.array([lam0, lam1])
    rng = np.random.default_rng(3)
    ts = np.concatenate([[0.0, t_ramp, 0.5 * t_ramp, np.nextafter(t_ramp, 0.0), np.nextafter(t_ramp, 1.0), 2.0, 1e9],
                         rng.uniform(0.0, t_ramp, 200), rng.uniform(t_ramp, 3.0, 20)])
    for t in ts:
        assert gh.history_value(t, times, values) == gd.load_factor(t, lam0, lam1, t_ramp), t
    dt = t_ramp / 7.0
    got = gh.sample((times, values), 12, dt)
    assert got.tobytes() == np.array([gd.load_factor(n * dt, lam0, lam1, t_ramp) for n in range(12)]).tobytes()
    assert gh.held(got, 11) == gh.held(got, 400) == got[11]


# ---------------------------------------------------------------------------------------------------------------------
# 3. production's sampling
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knots", ["uniform", "non-uniform"])
def test_production_sampling_against_the_restatement(knots):
    """history_samples of fem/dynamics.py against the restatement's sample, within 4 x 2^-53 max |values| per sample, at
    step times that fall on knots, between them, before the first and beyond the last.  A callable and the table it
    tabulates give the same bytes at the knots."""
    rng = np.random.default_rng(11 if knots == "uniform" else 12)
    dt, n = 0.01, 300
    times = 0.04 * np.arange(1, 60) if knots == "uniform" else np.sort(rng.uniform(0.2, 2.6, 41))
    values = rng.standard_normal(times.size)
    got = dyn.history_samples((times, values), np.arange(n, dtype=np.float64) * dt, "test")
    want = gh.sample((times, values), n, dt)
    err = np.max(np.abs(got - want))
    print(f"{knots}: production - restatement {err:.2e}, bound {4 * U53 * np.max(np.abs(values)):.2e}")
    assert got.dtype == np.float64 and got.shape == (n,) and err <= 4 * U53 * np.max(np.abs(values))
    assert got[0] == values[0] and got[-1] == values[-1] and len(set(got.tolist())) > 100
    # lists are taken as arrays are
    assert dyn.history_samples((times.tolist(), values.tolist()), np.arange(n) * dt).tobytes() == got.tobytes()
    # a callable, and the table of its values at the step times
    f = lambda t: np.sin(7.0 * t) - 0.3 * t
    t = np.arange(n, dtype=np.float64) * dt
    by_call = dyn.history_samples(f, t)
    by_table = dyn.history_samples((t, f(t)), t)
    assert by_call.tobytes() == f(t).tobytes() == by_table.tobytes()
    every_third = dyn.history_samples((t[::3], f(t[::3])), t)
    assert every_third[::3].tobytes() == f(t)[::3].tobytes() and not np.array_equal(every_third, by_call)
    assert dyn.history_samples(([0.5], [2.0]), t).tolist() == [2.0] * n


# ---------------------------------------------------------------------------------------------------------------------
# 4. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_check_dynamics_refusals():
    """Everything malformed is a ValueError of check_dynamics, and solve_dynamic raises it before it builds an engine."""
    T = gd.string()[0]
    model = _model(T)
    table = ([0.0, 1.0], [0.0, 1.0])
    motion = lambda **kw: dyn.SupportMotion(**{**dict(dofs=[1, 17], amplitudes=0.1, history=table), **kw})
    good = dyn.DynamicsConfig(n_steps=10, load_history=table, support_motion=motion())
    dyn.check_dynamics(model, _config(), good)
    dyn.check_dynamics(model, _config(), dyn.DynamicsConfig(n_steps=10, load_history=lambda t: np.sin(t),
                                                            support_motion=motion(amplitudes=[0.1, -0.2], history=np.cos)))
    assert dyn.DynamicsConfig().load_history is None and dyn.DynamicsConfig().support_motion is None
    nan, inf = float("nan"), float("inf")
    cases = [
        ("ramp", dict(load_history=table, ramp_time=0.5)),
        ("ramp", dict(load_history=table, load_factor_initial=0.5)),
        ("ramp", dict(load_history=table, load_factor_final=2.0)),
        ("load_history", dict(load_history=3.0)),
        ("load_history", dict(load_history=([0.0, 1.0],))),
        ("load_history", dict(load_history=([0.0, 1.0], [0.0, 1.0, 2.0]))),
        ("load_history", dict(load_history=([], []))),
        ("load_history", dict(load_history=([[0.0, 1.0]], [[0.0, 1.0]]))),
        ("load_history.*finite", dict(load_history=([0.0, 1.0], [0.0, nan]))),
        ("load_history.*finite", dict(load_history=([0.0, inf], [0.0, 1.0]))),
        ("load_history.*strictly increasing", dict(load_history=([0.0, 1.0, 0.5], [0.0, 1.0, 2.0]))),
        ("load_history.*strictly increasing", dict(load_history=([0.0, 1.0, 1.0], [0.0, 1.0, 2.0]))),
        ("load_history", dict(load_history=(["a", "b"], [0.0, 1.0]))),
        ("load_history.*shape", dict(load_history=lambda t: t[:-1])),
        ("load_history.*shape", dict(load_history=lambda t: 1.0)),
        ("load_history.*finite", dict(load_history=lambda t: t / 0.0 if False else np.full(t.shape, nan))),
        ("load_history", dict(load_history=lambda t: np.array(["x"] * t.size))),
        ("support_motion", dict(support_motion=([1, 17], 0.1, table))),
        ("support_motion.*twice", dict(support_motion=motion(dofs=[1, 1]))),
        ("support_motion.*not in fixed_dofs", dict(support_motion=motion(dofs=[1, 3]))),
        ("support_motion.*not in fixed_dofs", dict(support_motion=motion(dofs=[1, 18]))),
        ("support_motion.*not in fixed_dofs", dict(support_motion=motion(dofs=[-1, 17]))),
        ("support_motion", dict(support_motion=motion(dofs=[]))),
        ("support_motion", dict(support_motion=motion(dofs=[1.5, 17]))),
        ("support_motion.*amplitudes", dict(support_motion=motion(amplitudes=[0.1, 0.2, 0.3]))),
        ("support_motion.*amplitudes", dict(support_motion=motion(amplitudes=[[0.1, 0.2]]))),
        ("support_motion.*amplitudes", dict(support_motion=motion(amplitudes=nan))),
        ("support_motion.*amplitudes", dict(support_motion=motion(amplitudes="big"))),
        ("support_motion.history.*strictly increasing", dict(support_motion=motion(history=([1.0, 0.0], [0.0, 1.0])))),
        ("support_motion.history.*finite", dict(support_motion=motion(history=([0.0, 1.0], [inf, 1.0])))),
        ("support_motion.history.*shape", dict(support_motion=motion(history=lambda t: np.zeros((2, t.size))))),
        ("support_motion.history", dict(support_motion=motion(history=None))),
    ]
    for match, kw in cases:
        with pytest.raises(ValueError, match=match):
            dyn.check_dynamics(model, _config(), dyn.DynamicsConfig(n_steps=10, **kw))
        # before an engine is built: without a GPU the engine's own error would be another
        with pytest.raises(ValueError, match=match):
            dyn.solve_dynamic(model, _config(), dyn.DynamicsConfig(n_steps=10, **kw))


# ---------------------------------------------------------------------------------------------------------------------
# JSON and ABI surface
# ---------------------------------------------------------------------------------------------------------------------
def test_json_inputs_parse_to_histories(tmp_path):
    from pinn_fem_amd import fem
    from pinn_fem_amd.cli import generic as g
    assert fem.SupportMotion is dyn.SupportMotion
    p = g.parse_problem(os.path.join(HERE, "nl_inputs", "taut_string_pulse.json"))
    d = p["dynamics"]["config"]
    assert d.load_history == ([0.0, 0.2, 0.4], [0.0, 1.0, 0.0]) and d.support_motion is None and d.n_steps == 300
    assert d.load_history[0][-1] < d.n_steps * d.dt                 # the pulse ends before t_end
    dyn.check_dynamics(p["model"], p["solver_config"], d)
    p = g.parse_problem(os.path.join(HERE, "nl_inputs", "guyed_mast_shaken.json"))
    d = p["dynamics"]["config"]
    m = d.support_motion
    assert isinstance(m, dyn.SupportMotion) and m.dofs == [0, 4, 6] and m.amplitudes == 0.02 and d.cable_elements == [1, 2]
    assert len(m.history[0]) == len(m.history[1]) == 41 and d.load_history is None
    dyn.check_dynamics(p["model"], p["solver_config"], d)
    doc = json.load(open(os.path.join(HERE, "nl_inputs", "guyed_mast_shaken.json")))
    good = doc["accel"]["dynamics"]["support_motion"]
    for key, block in (("load_history", {"times": [0.0, 1.0]}), ("load_history", [[0.0, 1.0], [0.0, 1.0]]),
                       ("load_history", {"times": [0.0], "values": [0.0], "more": 1}),
                       ("support_motion", {k: v for k, v in good.items() if k != "dofs"}),
                       ("support_motion", dict(good, history=[])), ("support_motion", 3)):
        bad = dict(doc, accel=dict(doc["accel"], dynamics=dict(doc["accel"]["dynamics"], **{key: block})))
        (tmp_path / "bad.json").write_text(json.dumps(bad))
        with pytest.raises(ValueError, match="accel.dynamics"):
            g.parse_problem(str(tmp_path / "bad.json"))


def test_abi_surface():
    from pinn_fem_amd import _capi
    lib = _capi.load()
    header = open(os.path.join(ROOT, "include", "pinnfem_hip.h")).read()
    for name in ("pf_gl_dyn_start_hist", "pf_gl_dyn_steps_hist", "pf_gl_dyn_graph_create_hist"):
        assert re.search(r"^int " + name + r"\(", header, re.M) and name in _capi.SYMBOLS and hasattr(lib, name)
        plain = _capi.SYMBOLS[name[: -len("_hist")]][1]
        assert _capi.SYMBOLS[name] == (C.c_int, plain[:3] + [_capi._PH, C.c_void_p] + plain[3:])
    assert lib.pf_abi_version() == 9 and lib.pf_sizeof(7) == C.sizeof(_capi.PfDyn) == 104
    assert C.sizeof(_capi.PfDynHist) == 32
    assert [(f[0], f[1]) for f in _capi.PfDynHist._fields_] == [("lam", C.c_void_p), ("sup", C.c_void_p), ("sup_amp", C.c_void_p),
                                                                 ("n_samples", C.c_longlong)]
    assert re.search(r"const double\* lam;.*\n\s*const double\* sup;.*\n\s*const double\* sup_amp;.*\n\s*long long n_samples;", header)


def test_argument_errors_are_rejected_on_the_host():
    """A bad history record is PF_ERR_ARG with the function's name in front, before the namesake's own checks and before any
    HIP call: this runs without a GPU.  A good one falls through to the namesake's refusal of the (empty) mesh."""
    from pinn_fem_amd import _capi
    lib = _capi.load()
    p, g, d = _capi.PfProblem(), _capi.PfGl(), _capi.PfDyn()
    graph = C.c_void_p()
    some = (C.c_double * 4)(0.0, 1.0, 2.0, 3.0)
    at = C.cast(some, C.c_void_p).value

    def hist(**kw):
        h = _capi.PfDynHist()
        for key, value in dict(dict(lam=at, sup=at, sup_amp=at, n_samples=4), **kw).items():
            setattr(h, key, value)
        return C.byref(h)

    calls = {"pf_gl_dyn_start_hist": lambda h: lib.pf_gl_dyn_start_hist(C.byref(p), C.byref(g), C.byref(d), h, None, None),
             "pf_gl_dyn_steps_hist": lambda h: lib.pf_gl_dyn_steps_hist(C.byref(p), C.byref(g), C.byref(d), h, None, 1, None),
             "pf_gl_dyn_graph_create_hist": lambda h: lib.pf_gl_dyn_graph_create_hist(C.byref(p), C.byref(g), C.byref(d), h, None,
                                                                                      1, None, C.byref(graph))}
    for name, call in calls.items():
        for h, text in ((None, "null hist"), (hist(lam=None, sup=None), "hist holds neither lam nor sup"),
                        (hist(sup_amp=None), "sup without sup_amp"), (hist(lam=None, sup_amp=None), "sup without sup_amp"),
                        (hist(n_samples=0), "n_samples"), (hist(n_samples=-5), "n_samples"), (hist(), "bad mesh"),
                        (hist(sup=None, sup_amp=None), "bad mesh"), (hist(lam=None), "bad mesh")):
            assert call(h) == _capi.PF_ERR_ARG
            assert lib.pf_last_error().decode().startswith(name + ": " + text), lib.pf_last_error()
    assert not graph
