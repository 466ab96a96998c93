"""Kernel plugin interface (gpbasics/KernelBasics/Kernel.py).

``Kernel.get_tf_tensor(hyper_parameter, x_vector, x_vector_)`` keeps the reference's name and
argument meaning (K/Kernel.py:51-52) and returns an [n, m] fp64 device tensor computed by the
HIP kernel-matrix build (libgpk ``gpk_kernel_matrix``); ``get_tensor`` is an alias.
Subclasses add ``_emit``: the flattening of the tree into the device's postfix program.
"""
from __future__ import annotations

from enum import Enum
from typing import List

import torch

from ..Auxiliary import BasicGPComponent as bgpc


# enum values follow the reference (K/Kernel.py:10-37); built functionally
ConstantHyperParamType = Enum("ConstantHyperParamType", {"NONE_CONSTANT": 0, "JUST_CONSTANT_BASE_KERNELS": 1,
                                                         "JUST_CONSTANT_CP": 2, "ALL_CONSTANT": 3})
KernelType = Enum("KernelType", {"BASE_KERNEL": 1, "OPERATOR": 2})
KernelManifestation = Enum("KernelManifestation", dict(
    C=101, LIN=102, RQ=103, PER=104, SE=105, WN=106, MAT32=107, MAT52=108, ADD=201, MUL=202, CP=203, PART=204))


def _abstract(obj, name):
    return NotImplementedError("%s.%s is provided by the concrete kernel" % (type(obj).__name__, name))


def split_derivative_planes(planes: torch.Tensor, hyper_parameter: List) -> List[torch.Tensor]:
    """Flat planes [n_hyp, n, m] (DFS order) -> the list aligned with ``hyper_parameter``: entry k is a view of shape
    ``hyper_parameter[k].shape + (n, m)``."""
    shapes = [tuple(torch.as_tensor(h).shape) for h in hyper_parameter]
    counts = [max(1, int(torch.Size(s).numel())) for s in shapes]
    if planes.dim() != 3 or planes.shape[0] != sum(counts):
        raise ValueError("expected %d derivative planes [n_hyp, n, m], got %s" % (sum(counts), tuple(planes.shape)))
    out, i = [], 0
    for s, k in zip(shapes, counts):
        out.append(planes[i:i + k].reshape(s + tuple(planes.shape[1:])))
        i += k
    return out


def stack_derivative_planes(matrices: List[torch.Tensor]) -> torch.Tensor:
    """The inverse of split_derivative_planes: the list's entries [..., n, m] as flat planes [n_hyp, n, m]."""
    return torch.cat([m.reshape((-1,) + tuple(m.shape[-2:])) for m in matrices], dim=0)


class Kernel(bgpc.Component):
    """Abstract kernel: a node of a kernel expression tree."""

    def __init__(self, kernel_type: KernelType, manifestation: KernelManifestation, input_dimensionality: int):
        assert input_dimensionality >= 1, "input_dimensionality for a kernel ought to be one or larger"
        self.kernel_type = kernel_type
        self.manifestation = manifestation
        self.last_hyper_parameter = None
        self.input_dimensionality = input_dimensionality
        self.noise = None

    # -- evaluation -------------------------------------------------------------------------
    def get_tf_tensor(self, hyper_parameter: List, x_vector, x_vector_) -> torch.Tensor:
        assert x_vector is not None and x_vector_ is not None, "Input vectors x and x_ uninitialized: " + str(self)
        assert len(hyper_parameter) == self.get_number_of_hyper_parameter(), "Invalid hyper_param size: " + str(self)
        from .. import engine
        K = engine.kernel_matrix(self, hyper_parameter, x_vector, x_vector_)
        self._record_hyper_parameter(list(hyper_parameter))
        return K

    get_tensor = get_tf_tensor

    def _record_hyper_parameter(self, hyper_parameter: List):
        """The reference's get_tf_tensor stores its argument in last_hyper_parameter."""
        self.last_hyper_parameter = hyper_parameter

    def _emit(self, nodes: list, offset: int, ard_slots: list, dim: int) -> int:
        raise NotImplementedError("%s has no device form" % type(self).__name__)

    # -- tree / hyperparameter plumbing -----------------------------------------------------
    def get_kernel_type(self) -> KernelType:
        return self.kernel_type

    def get_kernel_manifestation(self) -> KernelManifestation:
        return self.manifestation

    def get_number_of_hyper_parameter(self) -> int:
        raise _abstract(self, 'get_number_of_hyper_parameter')

    def get_string_representation(self) -> str:
        raise _abstract(self, 'get_string_representation')

    def get_number_base_kernels(self) -> int:
        raise _abstract(self, 'get_number_base_kernels')

    def get_default_hyper_parameter(self, xrange: List[List[float]], n: int, from_distribution: bool = False) -> List:
        raise _abstract(self, 'get_default_hyper_parameter')

    def set_last_hyper_parameter(self, last_hyper_parameter: List):
        raise _abstract(self, 'set_last_hyper_parameter')

    def get_last_hyper_parameter(self, scaling_x_param=None):
        raise _abstract(self, 'get_last_hyper_parameter')

    def set_noise(self, noise):
        """noise must be a rank-0 value (K/Kernel.py:79-83)."""
        if torch.as_tensor(noise).shape == torch.Size([]):
            self.noise = noise
        else:
            raise Exception("Invalid Noise set for Kernel")

    def get_noise(self):
        return self.noise

    def deepcopy(self):
        raise _abstract(self, 'deepcopy')

    def get_string_representation_weight(self) -> float:
        return 0

    def sort_child_nodes(self):
        pass

    def get_json(self) -> dict:
        raise _abstract(self, 'get_json')

    def get_number_of_child_nodes(self) -> int:
        raise _abstract(self, 'get_number_of_child_nodes')

    def get_derivative_matrices(self, hyper_parameter: List, x_vector, x_vector_) -> List:
        """The derivative matrices d K(x_vector, x_vector_) / d hyper_parameter, a list aligned with
        ``hyper_parameter``: entry k has the shape ``hyper_parameter[k].shape + (n, m)`` -- [n, m] for a scalar,
        [d, n, m] for an ARD vector -- as fp64 device tensors (views of one gpk_kernel_jacobian result).  Base kernels
        and operators alike; ChangePointOperator in its 1-D device form.

        These are the true derivatives of the kernel as this library evaluates it, with respect to the values as
        passed: sign(l) for the Matern kernels' |l|, the analytic 0 of the distance terms at coincident points, 0 for
        the hard change-point mask.  They are deliberately NOT the reference's dead ``get_*_derivative_matrix``
        forms (K/BaseKernels.py:383-399, :232-241), of which SE's and LIN's are not derivatives of their kernels
        (DESIGN.md §7).  Records ``last_hyper_parameter`` as get_tf_tensor does."""
        assert x_vector is not None and x_vector_ is not None, "Input vectors x and x_ uninitialized: " + str(self)
        assert len(hyper_parameter) == self.get_number_of_hyper_parameter(), "Invalid hyper_param size: " + str(self)
        planes = self._derivative_planes(hyper_parameter, x_vector, x_vector_)
        self._record_hyper_parameter(list(hyper_parameter))
        return split_derivative_planes(planes, hyper_parameter)

    def _derivative_planes(self, hyper_parameter: List, x_vector, x_vector_) -> torch.Tensor:
        """[n_hyp, n, m]: one plane per flat hyperparameter in DFS order (engine.kernel_jacobian)."""
        from .. import engine
        return engine.kernel_jacobian(self, hyper_parameter, x_vector, x_vector_)

    def get_hyper_parameter_names(self, kernel_id: int = -1) -> List[str]:
        raise _abstract(self, 'get_hyper_parameter_names')

    def get_dimensionality(self):
        return self.input_dimensionality

    def set_dimensionality(self, input_dimensionality: int):
        self.input_dimensionality = input_dimensionality

    def get_simplified_version(self):
        return self

    def type_compare_to(self, other):
        return self == other

    def get_hash_tuple(self):
        flat = []
        if isinstance(self.last_hyper_parameter, list):
            for h in self.last_hyper_parameter:
                v = torch.as_tensor(h).detach().reshape(-1).tolist()
                flat.extend(float(x) for x in v)
        noise = None if self.noise is None else float(torch.as_tensor(self.noise, dtype=torch.float64))
        return self.manifestation.value, noise, tuple(flat)

    def __hash__(self):
        return hash(self.get_hash_tuple())
