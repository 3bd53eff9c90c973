from .BaseControl import BaseControl
from .CTBRControl import CTBRControl, VectorCTBR
from .DSLPIDControl import DSLPIDControl, DSLPIDControlBatch
from .MRAC import MRAC, VectorMRAC

__all__ = ["BaseControl", "CTBRControl", "VectorCTBR", "DSLPIDControl", "DSLPIDControlBatch", "MRAC", "VectorMRAC"]
