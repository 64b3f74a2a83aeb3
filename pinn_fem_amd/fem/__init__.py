"""Mirror of the reference's `fem` package for the accelerated PINN+GD path."""
from .model import FEMModel, Material
from .properties import Property, ScalarProperty, NNProperty, to_property
from .boundary import free_and_fixed_dofs

__all__ = ["FEMModel", "Material", "Property", "ScalarProperty", "NNProperty", "to_property",
           "free_and_fixed_dofs", "IdentifyResult", "check_identify", "identify_nr", "misfit_and_gradient", "residuals_and_jacobian",
           "check_strains", "PrestressResult", "check_prestress", "identify_prestress", "residuals_and_jacobian_prestress",
           "DynamicsConfig", "DynamicsResult", "check_dynamics", "solve_dynamic", "stable_time_step", "lumped_mass",
           "SupportMotion"]

_IDENTIFY = ("IdentifyResult", "check_identify", "identify_nr", "misfit_and_gradient", "residuals_and_jacobian",
             "check_strains")
_PRESTRESS = ("PrestressResult", "check_prestress", "identify_prestress", "residuals_and_jacobian_prestress")
_DYNAMICS = ("DynamicsConfig", "DynamicsResult", "check_dynamics", "solve_dynamic", "stable_time_step", "lumped_mass",
             "SupportMotion")


def __getattr__(name):
    # fem.identify, fem.prestress and fem.dynamics import the solver (and with it the engine): only when they are asked for
    if name in _IDENTIFY:
        from . import identify
        return getattr(identify, name)
    if name in _PRESTRESS:
        from . import prestress
        return getattr(prestress, name)
    if name in _DYNAMICS:
        from . import dynamics
        return getattr(dynamics, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
