"""Base mean functions (gpbasics/MeanFunctionBasics/BaseMeanFunctions.py:12-193): constant, zero, linear,
exponential and logit.

Detrending with the zero mean is the identity (gpbasics/DataHandling/DataInput.py:253-254), so y reaches the
factorisation untouched.  Every other mean -- and every tree of the operators in ``Operators.py`` -- is one
mean-function program on the device (include/gpk.h, ``gpk_mean_eval`` / ``gpk_mean_vjp``): ``_emit`` flattens a
tree to it, ``get_tf_tensor`` of the linear, exponential and logit means evaluates it and is differentiable in the
hyperparameters through the device reverse mode.  The constant and zero means keep their own ``get_tf_tensor``.
"""
from __future__ import annotations

import math
from typing import List

import torch

from .. import _native as nat
from .. import global_parameters as global_param
from . import MeanFunction as mf

global_param.ensure_init()


class BaseMeanFunction(mf.MeanFunction):
    _OP = None  # the leaf's op code in the device program (GPK_MOP_*)

    def __init__(self, manifestation, input_dimensionality: int):
        super().__init__(mf.MeanFunctionType.BASE_MEAN_FUNCTION, manifestation, input_dimensionality)

    def get_number_base_mean_function(self) -> int:
        return 1

    def set_last_hyper_parameter(self, last_hyper_parameter: List):
        assert len(last_hyper_parameter) == self.get_number_of_hyper_parameter(), \
            "Wrong size/shape of given 'last_hyper_param'"
        self.last_hyper_parameter = last_hyper_parameter

    def get_number_of_hyper_parameter(self) -> int:
        return len(self.get_default_hyper_parameter())

    def get_string_representation(self) -> str:
        return self.manifestation.name

    def get_string_representation_weight(self) -> int:
        return self.manifestation.value - 100

    def deepcopy(self):
        c = type(self)(self.input_dimensionality)
        c.set_last_hyper_parameter(self.last_hyper_parameter)
        return c

    # -- device program -------------------------------------------------------------------------
    def _n_values(self, dim: int) -> int:
        """Flat hyperparameter values of the leaf at input dimensionality ``dim``."""
        return sum(dim if s else 1 for s in self.get_hyper_parameter_dimensionalities())

    def _emit(self, nodes: list, offset: int, dim: int) -> int:
        nodes.append((self._OP, offset, -1, 0))
        return offset + self._n_values(dim)

    def _record_hyper_parameter(self, hyper_parameter: List):
        self.last_hyper_parameter = hyper_parameter

    def _device_tensor(self, hyper_parameter: List, x_vector) -> torch.Tensor:
        assert x_vector is not None, "Input vector x uninitialized: " + str(self)
        assert len(hyper_parameter) == self.get_number_of_hyper_parameter(), "Invalid hyper_param size: " + str(self)
        from ..engine import mean_tensor
        result = mean_tensor(self, hyper_parameter, x_vector)
        self.last_hyper_parameter = hyper_parameter
        return result

    def _filled(self, value: float) -> torch.Tensor:
        return torch.full([self.input_dimensionality], value, dtype=torch.float64)


class ConstantMeanFunction(BaseMeanFunction):
    """m(x) = c for every row of x (BaseMeanFunctions.py:37-63)."""
    _OP = nat.MOP_C

    def __init__(self, input_dimensionality: int):
        super().__init__(mf.MeanFunctionManifestation.C, input_dimensionality)

    def get_tf_tensor(self, hyper_parameter: List, x_vector) -> torch.Tensor:
        assert x_vector is not None, "Input vector x uninitialized: " + str(self)
        assert len(hyper_parameter) == self.get_number_of_hyper_parameter(), "Invalid hyper_param size: " + str(self)
        from ..engine import device
        c = torch.as_tensor(hyper_parameter[0], dtype=torch.float64).to(device())
        self.last_hyper_parameter = hyper_parameter
        return torch.zeros(x_vector.shape[0], dtype=torch.float64, device=device()) + c

    def get_default_hyper_parameter(self) -> List:
        return [torch.tensor(0.01, dtype=torch.float64)]

    def get_hyper_parameter_dimensionalities(self) -> List[list]:
        return [[]]


class ZeroMeanFunction(ConstantMeanFunction):
    """m(x) = 0 (BaseMeanFunctions.py:66-79)."""

    def get_string_representation(self) -> str:
        return "ZERO_MEAN"

    def get_default_hyper_parameter(self) -> List:
        return [torch.tensor(0.0, dtype=torch.float64)]

    def deepcopy(self):
        return ZeroMeanFunction(self.input_dimensionality)


class LinearMeanFunction(BaseMeanFunction):
    """m(x) = sum_k a_k x_k (BaseMeanFunctions.py:82-112); default slopes 1 / D."""
    _OP = nat.MOP_LIN

    def __init__(self, input_dimensionality: int):
        super().__init__(mf.MeanFunctionManifestation.LIN, input_dimensionality)

    def get_tf_tensor(self, hyper_parameter: List, x_vector) -> torch.Tensor:
        return self._device_tensor(hyper_parameter, x_vector)

    def get_default_hyper_parameter(self) -> List:
        return [self._filled(1 / self.input_dimensionality)]

    def get_hyper_parameter_dimensionalities(self) -> List[list]:
        return [[self.input_dimensionality, ]]


class ExponentialMeanFunction(BaseMeanFunction):
    """m(x) = base ^ sum_k (a_k x_k - b_k) (BaseMeanFunctions.py:115-151); defaults a = 1, b = 0, base = e."""
    _OP = nat.MOP_EXP

    def __init__(self, input_dimensionality: int):
        super().__init__(mf.MeanFunctionManifestation.EXP, input_dimensionality)

    def get_tf_tensor(self, hyper_parameter: List, x_vector) -> torch.Tensor:
        return self._device_tensor(hyper_parameter, x_vector)

    def get_default_hyper_parameter(self) -> List:
        return [self._filled(1.0), self._filled(0.0), torch.tensor(math.e, dtype=torch.float64)]

    def get_hyper_parameter_dimensionalities(self) -> List[list]:
        return [[self.input_dimensionality, ], [self.input_dimensionality, ], []]


class LogitMeanFunction(BaseMeanFunction):
    """m(x) = c / (1 + exp(sum_k (a_k x_k - b_k))) (BaseMeanFunctions.py:154-193); defaults a = -1, b = 0, c = 1."""
    _OP = nat.MOP_LOGIT

    def __init__(self, input_dimensionality: int):
        super().__init__(mf.MeanFunctionManifestation.LOGIT, input_dimensionality)

    def get_tf_tensor(self, hyper_parameter: List, x_vector) -> torch.Tensor:
        return self._device_tensor(hyper_parameter, x_vector)

    def get_default_hyper_parameter(self) -> List:
        return [self._filled(-1.0), self._filled(0.0), torch.tensor(1.0, dtype=torch.float64)]

    def get_hyper_parameter_dimensionalities(self) -> List[list]:
        return [[self.input_dimensionality, ], [self.input_dimensionality, ], []]
