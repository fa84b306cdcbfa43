"""Conditioners: x[B,d] -> h[B,d,hs] (package name spelled as in the reference)."""
from .Conditioner import Conditioner
from .CouplingConditioner import CouplingConditioner
from .AutoregressiveConditioner import AutoregressiveConditioner
from .DAGConditioner import DAGConditioner
from .StrADEConditioner import StrADEConditioner

__all__ = ["Conditioner", "AutoregressiveConditioner", "CouplingConditioner", "DAGConditioner", "StrADEConditioner"]
