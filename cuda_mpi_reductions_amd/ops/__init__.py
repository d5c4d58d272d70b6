"""Tensor operations backed by the native gfx950 kernels (csrc/kernels)."""
from .reduce import (  # noqa: F401
    DTYPE_CODES, OP_CODES, FaninError, KernelConfig, Reducer, cpu_reduce, default_acc_dtype, dtype_code,
    ladder_reduce, op_code, reduce, reduce_partials, sum_tolerance,
)
from .fill import PATTERNS, fill_, mt19937_fill_, synthetic  # noqa: F401
from .moments import combine_moments, moments  # noqa: F401
from .reduce_dim import reduce_dim  # noqa: F401
from .norm import norm  # noqa: F401
from .reduce_many import ReduceMany, norm_many, reduce_many  # noqa: F401
from .arg_reduce import arg_reduce, argmax, argmin  # noqa: F401
from .scan import ScanConfig, cummax, cummin, cumsum, scan, scan_plan, scan_workspace  # noqa: F401
from .segment import SegmentConfig, segment_plan, segment_reduce, segment_workspace  # noqa: F401
from .segment_scan import SegScanConfig, scan_dim, segment_scan, segscan_plan, segscan_workspace  # noqa: F401
from .histogram import HistogramConfig, bincount, histc, histogram_plan  # noqa: F401
from .sort import SortConfig, argsort, group_by_key, sort, sort_plan  # noqa: F401
from .topk import TopkConfig, topk, topk_plan  # noqa: F401
from .select import SelectConfig, masked_select, nonzero, select_plan, unique, unique_consecutive  # noqa: F401
from .softmax import SoftmaxConfig, cross_entropy, log_softmax, logsumexp, softmax, softmax_plan  # noqa: F401
