"""MI355X-native parallelized SGD: a drop-in for the hot path of
Patrickgsheng/spark-parallelized-sgd (ParallelizedSGD.runParallelizedSGD / optimize).

The per-partition SGD chains, the Gradient/SGDUpdater per-sample math and the model averaging
run as HIP kernels for gfx950 (csrc/, built into libpsgd.so, C ABI in include/psgd.h). This
package is the host side: the reference's Optimizer API and driver loop.

The directory name contains dashes; import it through __graft_entry__.load_package() (which
registers it as `spark_parallelized_sgd_amd`).
"""
from ._native import (DeviceError, IllegalArgumentException, UnsupportedOperationException,
                      build)
from .data import (CsrPartition, DensePartition, DeviceCsrPartition, DevicePartition, PartitionedData,
                   shard_range)
from .gradient import Gradient, HingeGradient, LeastSquaresGradient, LogisticGradient
from .feature import PCA, PCAModel, StandardScaler, StandardScalerModel, column_stats
from .optimization import (ColumnStats, DriverCheckpoint, Evaluation, HipEngine, ParallelizedSGD, ShardedEngine,
                           evaluate, evaluate_multinomial, make_params, runParallelizedSGD)
from .gradient_descent import (GradientDescent, GradientSum, gradient_sum, gradient_sum_multinomial, runMiniBatchSGD,
                               runMiniBatchSGDMultinomial)
from .newton import HessianSum, Newton, hessian_sum, runNewton
from .updater import (AdaGradSGDUpdater, AdamSGDUpdater, L1SGDUpdater, SGDUpdater,
                      SimpleSGDUpdater, SquaredL2SGDUpdater)
from .evaluation import BinaryClassificationMetrics, MulticlassMetrics
from .split import kFold, randomSplit
from .stat import (Gramian, computePrincipalComponents, computeSVD, corr, covariance, gramian, multiply,
                   normal_equations)
from .util import loadLibSVMFile

__all__ = [
    "ParallelizedSGD", "runParallelizedSGD", "evaluate", "evaluate_multinomial", "Evaluation", "HipEngine",
    "BinaryClassificationMetrics", "MulticlassMetrics", "randomSplit", "kFold",
    "GradientDescent", "runMiniBatchSGD", "gradient_sum", "GradientSum",
    "gradient_sum_multinomial", "runMiniBatchSGDMultinomial",
    "Newton", "runNewton", "hessian_sum", "HessianSum",
    "Gramian", "gramian", "covariance", "corr", "normal_equations",
    "multiply", "computePrincipalComponents", "computeSVD", "PCA", "PCAModel",
    "column_stats", "ColumnStats", "StandardScaler", "StandardScalerModel", "ShardedEngine", "make_params",
    "Gradient", "LogisticGradient", "LeastSquaresGradient", "HingeGradient",
    "SGDUpdater", "SimpleSGDUpdater", "SquaredL2SGDUpdater", "L1SGDUpdater",
    "AdaGradSGDUpdater", "AdamSGDUpdater",
    "PartitionedData", "DensePartition", "CsrPartition", "DevicePartition", "DeviceCsrPartition",
    "shard_range", "loadLibSVMFile",
    "IllegalArgumentException", "UnsupportedOperationException", "DeviceError", "build",
]
