from .dense import DenseStack, TFBatchNorm, TFDense, DenseParams
from .embedding import FieldTables
from .ftrl import RowFtrl
from .row_adam import NamedTables, RowAdam

__all__ = ["DenseStack", "TFBatchNorm", "TFDense", "DenseParams", "FieldTables", "NamedTables", "RowAdam", "RowFtrl"]
