"""laser_amd -- MI355X (gfx950) implementation of mratsim/laser's packed-panel GEMM hot path.

The product is liblaser_hip.so (hand-written HIP behind the C-ABI of include/laser_hip.h); this
package is the thin host-side mirror of the reference's Nim procs over that ABI.  No CPU fallback.
"""
from ._lib import LaserHipError, LIB_PATH, lib  # noqa: F401
from .primitives import *  # noqa: F401,F403
from . import primitives  # noqa: F401
from . import tensor  # noqa: F401
from . import sharded  # noqa: F401
from .foreach import forEach  # noqa: F401
from .reduce import reduce_sum, reduce_min, reduce_max, forEachReduce  # noqa: F401
from .simd_math import exp, softmax, softmax_backward, log, logsumexp, log_softmax, softmax_cross_entropy  # noqa: F401
from .simd_math import tanh, sigmoid, activation, activation_grad  # noqa: F401
from .simd_math import sin, cos, sincos  # noqa: F401
from .nn import bias_grad, linear_backward, layer_norm, layer_norm_backward  # noqa: F401
from .optim import sgd_step, adam_step, grad_norm, adam_bias_correction, SGD, Adam  # noqa: F401
from .nn import embedding, embedding_group, embedding_backward  # noqa: F401
from .nn import attention, attention_backward  # noqa: F401
from .sampling import Sampler, newSampler, multinomial, sample_top_k  # noqa: F401
from .select import topk, argmax, argmin, take_rows, topk_plan, topk_last_kernel  # noqa: F401
from .random import Rng, randomTensor, randomNormalTensor  # noqa: F401
from .scan import cumsum, searchsorted, cdfSample, cdfSampleAndRemove  # noqa: F401
from .sharded import (shard_plan, set_shard_devices, get_shard_devices, gemm_strided_sharded, matmul_sharded,  # noqa: F401
                      gemm_strided_sharded_dev, shard_rows, GATHER_NONE, GATHER_PEER, GATHER_RCCL, SHARD_PIN_TILE)
from .tensor import (Tensor, HipStorage, newTensor, toTensor, fromTorch, deepCopy, copyFrom, copyFromRaw,  # noqa: F401
                     setZero, forEachMap, MAP_OPS)

__version__ = "0.1.0"
