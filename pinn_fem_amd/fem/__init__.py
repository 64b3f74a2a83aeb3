"""Mirror of the reference's `fem` package for the accelerated PINN+GD path."""
from .model import FEMModel, Material
from .properties import Property, ScalarProperty, NNProperty, to_property
from .boundary import free_and_fixed_dofs

__all__ = ["FEMModel", "Material", "Property", "ScalarProperty", "NNProperty", "to_property",
           "free_and_fixed_dofs", "IdentifyResult", "check_identify", "identify_nr", "misfit_and_gradient", "residuals_and_jacobian",
           "check_strains"]

_IDENTIFY = ("IdentifyResult", "check_identify", "identify_nr", "misfit_and_gradient", "residuals_and_jacobian",
             "check_strains")


def __getattr__(name):
    # fem.identify imports the solver (and with it the engine): only when it is asked for
    if name in _IDENTIFY:
        from . import identify
        return getattr(identify, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
