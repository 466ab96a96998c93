"""Mean-function operators (gpbasics/MeanFunctionBasics/Operators.py): n-ary sum and product of mean functions.

The reference evaluates an operator by recursing into its children and folding their vectors left to right
(Operators.py:123-140, :157-176).  Here the whole tree is one device program (include/gpk.h, ``gpk_mean_eval``):
``_emit`` writes the children left to right and the binary op after each child beyond the first -- the same left
fold -- and ``get_tf_tensor`` evaluates it, differentiable in the hyperparameters (``gpk_mean_vjp``).
"""
from __future__ import annotations

from typing import List

import torch

from .. import _native as nat
from . import MeanFunction as mf


class Operator(mf.MeanFunction):
    _BINARY_OP = None

    def __init__(self, manifestation, child_nodes: List[mf.MeanFunction], input_dimensionality: int, sign: str):
        super().__init__(mf.MeanFunctionType.OPERATOR, manifestation, input_dimensionality)
        self.child_nodes: List[mf.MeanFunction] = child_nodes
        if self.manifestation.value < 200:
            print("Invalid manifestation for Operator: ", manifestation)
        self.sortable = False
        self.sign: str = sign

    # -- device program -------------------------------------------------------------------------
    def _emit(self, nodes: list, offset: int, dim: int) -> int:
        if not self.child_nodes:
            raise ValueError("operator without child nodes")
        for i, cn in enumerate(self.child_nodes):
            offset = cn._emit(nodes, offset, dim)
            if i > 0:
                nodes.append((self._BINARY_OP, 0, -1, 0))
        return offset

    def _slices(self, hyper_parameter: List):
        idx = 0
        for cn in self.child_nodes:
            cnt = cn.get_number_of_hyper_parameter()
            yield cn, list(hyper_parameter[idx:idx + cnt])
            idx += cnt

    def _record_hyper_parameter(self, hyper_parameter: List):
        # children record their slices, as the reference's recursive evaluation does
        for cn, sl in self._slices(hyper_parameter):
            cn._record_hyper_parameter(sl)

    def get_tf_tensor(self, hyper_parameter: List, x_vector) -> torch.Tensor:
        assert x_vector is not None, "Input vector x uninitialized: " + str(self)
        assert len(hyper_parameter) == self.get_number_of_hyper_parameter(), \
            "Invalid hyper_param size: " + str(self.get_string_representation()) + str(len(hyper_parameter)) + \
            "!=" + str(self.get_number_of_hyper_parameter())
        from ..engine import mean_tensor
        result = mean_tensor(self, hyper_parameter, x_vector)
        self._record_hyper_parameter(list(hyper_parameter))
        return result

    # -- plumbing -------------------------------------------------------------------------------
    def get_number_of_hyper_parameter(self):
        return sum(cn.get_number_of_hyper_parameter() for cn in self.child_nodes)

    def add_child_mean_function(self, mean_function):
        self.child_nodes = self.child_nodes + [mean_function]

    def replace_child_node(self, index, new_child_node: mf.MeanFunction):
        assert index < len(self.child_nodes), \
            "cannot replace child node at index" + str(index) + ". Invalid as there are only " + \
            str(len(self.child_nodes)) + " child nodes."
        self.child_nodes[index] = new_child_node

    def get_number_base_mean_function(self):
        return sum(cn.get_number_base_mean_function() for cn in self.child_nodes)

    def get_default_hyper_parameter(self) -> List:
        result = []
        for cn in self.child_nodes:
            result = result + cn.get_default_hyper_parameter()
        return result

    def set_last_hyper_parameter(self, last_hyper_parameter: List):
        assert len(last_hyper_parameter) == self.get_number_of_hyper_parameter(), \
            "Invalid hyper_param size: " + str(self)
        for cn, sl in self._slices(last_hyper_parameter):
            cn.set_last_hyper_parameter(sl)

    def get_last_hyper_parameter(self) -> List:
        result = []
        for cn in self.child_nodes:
            result = result + cn.get_last_hyper_parameter()
        return result

    def get_number_of_child_nodes(self):
        return len(self.child_nodes)

    def sort_child_nodes(self):
        if self.sortable:
            self.child_nodes = sorted(self.child_nodes, key=lambda node: node.get_string_representation_weight(),
                                      reverse=False)
        for cn in self.child_nodes:
            if isinstance(cn, Operator):
                cn.sort_child_nodes()

    def get_string_representation_weight(self):
        return sum(cn.get_string_representation_weight() for cn in self.child_nodes)

    def get_string_representation(self):
        if len(self.child_nodes) == 1:
            return self.child_nodes[0].get_string_representation()
        return "(" + self.sign.join(cn.get_string_representation() for cn in self.child_nodes) + ")"

    def get_hyper_parameter_dimensionalities(self) -> List[list]:
        result = []
        for cn in self.child_nodes:
            result.extend(cn.get_hyper_parameter_dimensionalities())
        return result

    def deepcopy(self):
        return type(self)([cn.deepcopy() for cn in self.child_nodes], self.input_dimensionality)


class MultiplicationOperator(Operator):
    _BINARY_OP = nat.MOP_MUL

    def __init__(self, child_nodes: List[mf.MeanFunction], input_dimensionality: int):
        super().__init__(mf.MeanFunctionManifestation.MUL, child_nodes, input_dimensionality, " x ")
        self.sortable = True


class AdditionOperator(Operator):
    _BINARY_OP = nat.MOP_ADD

    def __init__(self, child_nodes: List[mf.MeanFunction], input_dimensionality: int):
        super().__init__(mf.MeanFunctionManifestation.ADD, child_nodes, input_dimensionality, " + ")
        self.sortable = True
