"""The one host setup of the Newton solve and of identification (solver._newton_setup, solver._pre_check) on the device:
what it does with u_initial under either control, that the public evaluation functions of fem/identify.py and the ones
identify_nr drives compute the same bits, and the refusal of a free dof no element stiffens."""
import numpy as np
import pytest
import torch

import gl_e0_reference as g0
import gl_reference as gl
import identify_reference as ir

pytestmark = pytest.mark.gpu

YOUNG, AREA = 2000.0, 0.5                       # E*A = 1000, exact in float32
EA = YOUNG * AREA
CONTROLS = {"load": {}, "displacement": dict(nr_control="displacement", nr_control_dof=5, nr_control_displacement=-0.3)}


def _model(nodes, el, loads, fixed, dimension=2):
    from pinn_fem_amd.fem.model import FEMModel, Material
    return FEMModel(nodes=nodes, elements=el, material=Material(YOUNG, AREA, 1.0), loads=loads, fixed_dofs=fixed,
                    dimension=dimension)


def _config(**kw):
    from pinn_fem_amd.fem.solver import SolverConfig
    base = dict(max_iterations=50, tolerance=1e-10, kinematics="green-lagrange")
    base.update(kw)
    return SolverConfig(**base)


@pytest.fixture(scope="module")
def two_bar():
    tb = gl.TwoBar(ea=EA)
    return _model(tb.nodes, tb.el, tb.loads(0.5 * tb.p_lim), tb.fixed)


def _bits(res, converged=True):
    """Everything a SolverResult computes, as bytes."""
    assert res.converged == converged
    return (res.displacements.tobytes(), res.reactions.tobytes(),
            [(key, np.float64(value).tobytes()) for entry in res.history for key, value in entry.items()])


# ---- 1. the start vector ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("control", list(CONTROLS))
def test_u_initial_of_the_wrong_length_is_refused(two_bar, control):
    from pinn_fem_amd.fem.solver import solve_nr
    for n in (5, 7):
        with pytest.raises(ValueError, match=r"u_initial has \d+ entries, the model has \d+ dofs"):
            solve_nr(two_bar, _config(**CONTROLS[control]), 1.0, u_initial=torch.zeros(n, dtype=torch.float64))
        with pytest.raises(ValueError, match=r"u_initial has \d+ entries, the model has \d+ dofs"):
            solve_nr(two_bar, _config(**CONTROLS[control]), 1.0, u_initial=np.zeros(n))


@pytest.mark.parametrize("control", list(CONTROLS))
def test_fixed_dofs_of_u_initial_are_ignored(two_bar, control):
    from pinn_fem_amd.fem.solver import solve_nr
    clean = np.array([0.0, 0.0, 0.0, 0.0, 0.01, -0.05])
    dirty = clean.copy()
    dirty[[0, 3]] = 0.3, -7.0                                           # dofs 0..3 are the supports
    runs = [solve_nr(two_bar, _config(**CONTROLS[control]), 1.0, u_initial=torch.from_numpy(u0)) for u0 in (clean, dirty)]
    runs.append(solve_nr(two_bar, _config(**CONTROLS[control]), 1.0, u_initial=dirty))         # an array, not a tensor
    print(f"{control} control: {runs[0].history[-1]}")
    assert runs[0].displacements.reshape(-1)[5] < 0.0 and not runs[0].displacements.reshape(-1)[:4].any()
    assert _bits(runs[0]) == _bits(runs[1]) == _bits(runs[2])
    # and the free dofs are used: one Newton step from them is not the one from zero
    one = _config(max_iterations=1, **CONTROLS[control])
    steps = [solve_nr(two_bar, one, 1.0, u_initial=u0) for u0 in (None, clean, dirty)]
    assert _bits(steps[1], False) == _bits(steps[2], False) != _bits(steps[0], False)


def test_the_linear_solve_does_not_use_u_initial(two_bar):
    from pinn_fem_amd.fem.solver import solve_nr
    config = _config(kinematics="linear")
    cold = solve_nr(two_bar, config, 1.0)
    warm = solve_nr(two_bar, config, 1.0, u_initial=torch.tensor([0.3, 0.0, 0.0, -7.0, 0.01, -0.05], dtype=torch.float64))
    short = solve_nr(two_bar, config, 1.0, u_initial=torch.ones(4))     # not even its length is looked at
    assert cold.displacements.reshape(-1)[5] < 0.0
    assert _bits(cold) == _bits(warm) == _bits(short)


# ---- 2. the public evaluations and the ones identify_nr drives ---------------------------------------------------------
@pytest.fixture(scope="module", params=["plain", "initial-strain"])
def warren(request):
    case = ir.warren_case(8) if request.param == "plain" else g0.warren_case(8)
    model = _model(case.nodes, case.el, case.loads, case.fixed)
    config = _config(initial_strain=None if request.param == "plain" else case.e0)
    assert case.n_groups == 4 and case.ea0 == EA
    return case, model, config, np.array([0.1, -0.05, 0.02, 0.0])


def test_direct_and_driven_misfit_agree(warren):
    from pinn_fem_amd.fem import identify, solver
    case, model, config, q0 = warren
    ea = case.ea0 * np.exp(q0)[case.groups]
    J, g_ea, states, counters = identify.misfit_and_gradient(model, config, case.levels, ea)
    eng = solver._engine_for(model, None, None)
    gq = eng.group_sum(g_ea, torch.from_numpy(ea).to(eng.device), case.groups).cpu()
    res = identify.identify_nr(model, config, case.levels, groups=case.groups, q0=q0, method="lbfgs", max_evaluations=1)
    first = res.history[0]
    print(f"J = {J!r} (driven {first['misfit']!r}), |dJ/dq| = {float(torch.linalg.norm(gq))!r} (driven "
          f"{first['gradient_norm']!r}), counters {counters}")
    assert res.evaluations == 1 and len(res.history) == 1 and J > 0.0
    assert first["misfit"] == J and res.misfit == J
    assert first["gradient_norm"] == float(torch.linalg.norm(gq))
    assert res.gradient.tobytes() == gq.numpy().tobytes()
    assert res.counters == counters
    assert all(a.tobytes() == b.cpu().numpy().tobytes() for a, b in zip(res.displacements, states))


def test_direct_and_driven_jacobian_agree(warren):
    from pinn_fem_amd.fem import identify
    case, model, config, q0 = warren
    ea = case.ea0 * np.exp(q0)[case.groups]
    rho, A, states, counters = identify.residuals_and_jacobian(model, config, case.levels, ea, case.groups)
    res = identify.identify_nr(model, config, case.levels, groups=case.groups, q0=q0, method="gauss-newton",
                               max_evaluations=1)
    print(f"J = {float(rho @ rho)!r} (driven {res.misfit!r}), A {A.shape}, stop {res.stop}, counters {counters}")
    assert res.stop == "cap" and res.evaluations == 1 and A.shape == (sum(len(d) for _, d, _ in case.levels), 4)
    assert res.jacobian.tobytes() == A.tobytes()
    assert res.misfit == float(rho @ rho) and res.history[0]["misfit"] == res.misfit
    assert res.counters == counters
    assert all(a.tobytes() == b.cpu().numpy().tobytes() for a, b in zip(res.displacements, states))


# ---- 3. the pre-check without an initial strain --------------------------------------------------------------------------
def test_a_free_dof_no_element_stiffens_is_refused():
    """One 1-D bar, its first node fixed, and a third node no element touches: the diagonal of K is zero there."""
    from pinn_fem_amd.fem import identify
    from pinn_fem_amd.fem.solver import solve_nr
    loads = np.array([0.0, 1.0, 0.0])
    model = _model(np.array([0.0, 1.0, 2.5]), np.array([[0, 1]]), loads, np.array([0]), dimension=1)
    for config in (_config(), _config(kinematics="linear")):
        with pytest.raises(RuntimeError, match="Tangent stiffness became singular"):
            solve_nr(model, config, 1.0)
    with pytest.raises(RuntimeError, match="Tangent stiffness became singular"):
        identify.misfit_and_gradient(model, _config(), [(1.0, [1], [1e-3])], np.array([EA]))
    with pytest.raises(RuntimeError, match="Tangent stiffness became singular"):
        identify.residuals_and_jacobian(model, _config(), [(1.0, [1], [1e-3])], np.array([EA]), [0])
    # the same bar without the loose node solves
    model = _model(np.array([0.0, 1.0]), np.array([[0, 1]]), loads[:2], np.array([0]), dimension=1)
    assert solve_nr(model, _config(), 1.0).converged
