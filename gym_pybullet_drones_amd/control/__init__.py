from .BaseControl import BaseControl
from .DSLPIDControl import DSLPIDControl, DSLPIDControlBatch
from .MRAC import MRAC, VectorMRAC

__all__ = ["BaseControl", "DSLPIDControl", "DSLPIDControlBatch", "MRAC", "VectorMRAC"]
