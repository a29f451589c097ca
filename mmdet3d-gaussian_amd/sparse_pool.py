"""Sparse max pooling: spconv 1.x's `SparseMaxPool3d` (include/gd3d.h, gd3d_sparse_max_pool_*; csrc/sparse_pool.hip).

`sparse_max_pool(features, index)` takes the maximum of every output row's window over the tables of a strided `sparse_conv_index` — one
launch forward, one backward, both gathers: no atomics, the same bits from run to run, capturable.  The output element is a copy of an
input element (no rounding in any type); a row without a valid neighbour or past the count is zero; a NaN in a window gives NaN.  The
backward hands grad_out to EVERY input that equals its window's maximum (spconv 1.x's rule).  fp32, fp16 and bf16 are native, another
dtype goes through fp32.  `SparseMaxPool3d` is the module.
"""
import math

import torch

from . import _host
from .sparse_conv import SparseConvIndex, sparse_conv_index
from .sparse_tensor import DTYPE_CODES, MAX_CHANNELS, MAX_OFFSETS, SparseConvTensor, SparseModule, as_dtype, kernel_dtype, triple


class _SparseMaxPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, nbr, nbr_t, num):
        dtype = kernel_dtype(features)
        x = as_dtype(features, dtype)
        (N, C), (R, K), dev = x.shape, nbr.shape, x.device
        out = torch.empty((R, C), dtype=dtype, device=dev)
        ptr = _host.ptr_or_null
        _host.call('gd3d_sparse_max_pool_forward', dev, (ptr(x), ptr(nbr), ptr(num), N, R, K, C, DTYPE_CODES.get(dtype, 0), ptr(out)))
        ctx.save_for_backward(x, out, nbr_t)
        ctx.state = (features.dtype, dtype)
        return out if dtype == features.dtype else out.to(features.dtype)

    @staticmethod
    @_host.guard_double_backward
    def backward(ctx, grad_out):
        x, out, nbr_t = ctx.saved_tensors
        x_dtype, dtype = ctx.state
        (N, C), R, K, dev = x.shape, out.size(0), nbr_t.size(1), x.device
        gy = as_dtype(grad_out, dtype)
        gx = torch.empty((N, C), dtype=dtype, device=dev)
        ptr = _host.ptr_or_null
        _host.call('gd3d_sparse_max_pool_backward', dev, (ptr(gy), ptr(x), ptr(out), ptr(nbr_t), N, R, K, C, DTYPE_CODES.get(dtype, 0), ptr(gx)))
        return gx.to(x_dtype), None, None, None


def sparse_max_pool(features, index):
    """Max pooling over the tables of `sparse_conv_index(subm=False)` -> (R, C), differentiable w.r.t. features.

    out[o, c] = max over the offsets j with index.nbr[o, j] >= 0 of features[nbr[o, j], c]; features (N, C), 1 <= C <= 256.  Every row is
    written: a row at or past num[0] (the static `max_out` form) and a row without a valid neighbour are ZERO, not -inf.  A NaN in the
    window gives NaN (torch's rule); a window of -inf gives -inf.  The output element is a copy of an input element: bit-equal to a dense
    `max_pool3d` of the -inf-filled input read at `out_coors`, in every type.
    Backward: grad_features[i, c] = the sum in ascending j over the offsets with o = index.nbr_t[i, j] >= 0 and features[i, c] == out[o, c]
    of grad_out[o, c], accumulated in fp32 and rounded once — every tied input of a window receives the gradient (spconv 1.x's equality
    rule; torch hands it to one), a NaN window passes none, inactive rows and inputs that feed only dropped outputs get zero.
    One launch each way, no atomics: the same bits from run to run and under graph replay.  fp32, fp16 and bf16 run natively, another
    floating dtype is evaluated in fp32 and cast back."""
    if not isinstance(index, SparseConvIndex) or index.subm or index.nbr_t is None:
        raise RuntimeError('sparse_max_pool: index must be the record sparse_conv_index(subm=False) returns')
    K = index.nbr.size(1)
    if not isinstance(features, torch.Tensor) or features.dim() != 2 or not features.dtype.is_floating_point:
        raise RuntimeError(f'shape mismatch: sparse_max_pool: features must be a floating-point (N, C) tensor, got {tuple(getattr(features, "shape", ()))}')
    if features.size(0) != index.num_in:
        raise RuntimeError(f'shape mismatch: sparse_max_pool: the index was built over {index.num_in} rows, got {features.size(0)}')
    if not 1 <= features.size(1) <= MAX_CHANNELS or not 1 <= K <= MAX_OFFSETS:
        raise RuntimeError(f'sparse_max_pool: 1 .. {MAX_CHANNELS} channels and 1 .. {MAX_OFFSETS} offsets are supported, got {features.size(1)} and {K}')
    if index.nbr.device != features.device:
        raise RuntimeError(f'sparse_max_pool: index is on {index.nbr.device}, features on {features.device}')
    return _SparseMaxPool.apply(features, index.nbr, index.nbr_t, index.num)


class SparseMaxPool3d(SparseModule):
    """spconv 1.x's `SparseMaxPool3d(kernel_size, stride=1, padding=0, dilation=1)`: the maximum over each output cell's window of active
    inputs, on the output cells `SparseConv3d` of the same geometry has (`sparse_conv_index(subm=False)`, built per call: a pooling layer
    has no `indice_key`).  max_out (an addition, as on `SparseConv3d`): an int gives the static, capturable form.  Dilation must be 1."""

    def __init__(self, kernel_size, stride=1, padding=0, dilation=1, *, max_out=None):
        super().__init__()
        if triple(dilation, 'dilation') != (1, 1, 1):
            raise RuntimeError(f'SparseMaxPool3d: dilation must be 1, got {dilation}')
        self.kernel_size, self.stride, self.padding = triple(kernel_size, 'kernel_size'), triple(stride, 'stride'), triple(padding, 'padding')
        self.dilation = (1, 1, 1)
        self.max_out = max_out
        if math.prod(self.kernel_size) > MAX_OFFSETS or min(self.kernel_size) < 1:
            raise RuntimeError(f'SparseMaxPool3d: kernel_size {self.kernel_size} must hold 1 .. {MAX_OFFSETS} offsets')

    def forward(self, x):
        SparseConvTensor.expect(x, 'SparseMaxPool3d')
        index = sparse_conv_index(x.indices, x.spatial_shape, x.batch_size, self.kernel_size, self.stride, self.padding, False, self.max_out)
        return x.derive(sparse_max_pool(x.features, index), index.out_coors, index.out_shape)

    def extra_repr(self):
        return f'kernel_size={self.kernel_size}, stride={self.stride}, padding={self.padding}' + ('' if self.max_out is None else f', max_out={self.max_out}')
