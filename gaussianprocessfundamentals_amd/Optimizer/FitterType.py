"""Fitter kinds (gpbasics/Optimizer/FitterType.py:4-6, same names and values)."""
import enum


class FitterType(enum.Enum):
    # the reference's definition ends in a comma, so this member's value is the tuple (0,), not 0: kept, since
    # FitterType((0,)) and .value are what a drop-in user may have pickled or compared
    GRADIENT = (0,)
    NON_GRADIENT = 1
