"""Batch normalisation over the LIVE rows of a sparse tensor (include/gd3d.h, gd3d_sparse_bn_*; csrc/sparse_bn.hip).

`nn.BatchNorm1d` on `.features` knows nothing about which rows are live: in the static forms (`sparse_conv_index(..., max_out=R)`,
`hard_voxelize(static=True)`) and with inactive rows inside a tensor it counts dead rows in its mean and variance, writes the polluted
values into its running buffers and turns the zero rows into `shift`.  `sparse_batch_norm` takes the statistics over the live rows alone —
liveness is read from `coors` on the device, by `sparse_conv_index`'s rule, and no count is read back — adds a basic block's residual,
applies the ReLU, and writes exact zeros to the dead rows: training and eval, forward and backward, fp32 / fp16 / bf16, deterministic,
without atomics, capturable.  `SparseBatchNorm1d` is the module (the parameters, buffers and `state_dict` keys of `nn.BatchNorm1d`);
`convert_sparse_batchnorm` / `SparseEncoder.convert_norm()` (sparse_encoder.py) put it into an encoder, opt-in; `fuse_sparse_conv_bn`
folds it as it folds a `BatchNorm1d`.
"""
import torch
from torch import nn

from . import _host, _lib
from .sparse_tensor import ACT_CODES, DTYPE_CODES, MAX_CHANNELS, SparseConvTensor, SparseModule, as_dtype, check_activation, coors_i32, kernel_dtype, triple

_workspace_bytes = _host.memo(lambda r, c: _lib.load().gd3d_sparse_bn_workspace_bytes(r, c))


def _workspace(R, C, dev):
    return torch.empty((_workspace_bytes(R, C),), dtype=torch.uint8, device=dev) if dev.type == 'cuda' else None


class _SparseBatchNorm(torch.autograd.Function):
    """one C entry forward (statistics, finish, normalise: at most 3 launches; 1 in eval), one backward (at most 3)"""

    @staticmethod
    def forward(ctx, features, weight, bias, residual, coors, running_mean, running_var, num_batches_tracked, shape, B, training, momentum, eps,
                activation):
        dtype = kernel_dtype(features)
        x = as_dtype(features, dtype)
        res = None if residual is None else as_dtype(residual, dtype)
        w = None if weight is None else _host.f32c(weight)
        b = None if bias is None else _host.f32c(bias)
        (R, C), dev = x.shape, x.device
        batch_stats = training or running_mean is None                     # track_running_stats=False: batch statistics in eval too
        out = torch.empty((R, C), dtype=dtype, device=dev)
        # save_mean and save_invstd: the two rows of one tensor (eval: the running buffers themselves); one workspace for both directions
        stats = torch.empty((2, C), dtype=torch.float32, device=dev) if batch_stats else None
        work = _workspace(R, C, dev) if batch_stats else None
        update = training and running_mean is not None
        ptr = _host.ptr
        _host.call('gd3d_sparse_bn_forward', dev,
                   (_host.ptr_or_null(x), _host.ptr_or_null(coors), _host.ptr_or_null(res), ptr(w), ptr(b),
                    ptr(running_mean) if update or not batch_stats else None, ptr(running_var) if update or not batch_stats else None,
                    ptr(num_batches_tracked) if update else None, R, C, B, *shape, int(batch_stats), float(momentum), float(eps),
                    ACT_CODES[activation], DTYPE_CODES.get(dtype, 0), ptr(work), _host.ptr_or_null(out),
                    stats.data_ptr() if batch_stats else None, stats.data_ptr() + 4 * C if batch_stats else None))
        ctx.save_for_backward(x, w, stats if batch_stats else running_mean, None if batch_stats else running_var, out if activation == 'relu' else None, coors)
        ctx.work = work
        ctx.state = (shape, B, batch_stats, eps, activation, dtype, features.dtype, None if weight is None else weight.dtype,
                     None if bias is None else bias.dtype, None if residual is None else residual.dtype)
        return out if dtype == features.dtype else out.to(features.dtype)

    @staticmethod
    @_host.guard_double_backward
    def backward(ctx, grad_out):
        x, w, mean, var, out, coors = ctx.saved_tensors
        shape, B, batch_stats, eps, activation, dtype, x_dtype, w_dtype, b_dtype, r_dtype = ctx.state
        (R, C), dev = x.shape, x.device
        gy = as_dtype(grad_out, dtype)
        gx = torch.empty((R, C), dtype=dtype, device=dev)
        gres = torch.empty((R, C), dtype=dtype, device=dev) if r_dtype is not None and ctx.needs_input_grad[3] else None
        need_w, need_b = w_dtype is not None and ctx.needs_input_grad[1], b_dtype is not None and ctx.needs_input_grad[2]
        gwb = torch.empty((2, C), dtype=torch.float32, device=dev) if need_w or need_b else None      # grad_weight, grad_bias: two rows of one tensor
        gw, gb = (gwb[0] if need_w else None), (gwb[1] if need_b else None)
        work = ctx.work if ctx.work is not None else _workspace(R, C, dev)
        ptr, ptr0 = _host.ptr, _host.ptr_or_null
        _host.call('gd3d_sparse_bn_backward', dev,
                   (ptr0(gy), ptr0(x), ptr0(out), ptr0(coors), ptr(w), mean.data_ptr(), mean.data_ptr() + 4 * C if batch_stats else var.data_ptr(), R, C, B,
                    *shape, int(batch_stats), float(eps), ACT_CODES[activation], DTYPE_CODES.get(dtype, 0), ptr(work), ptr0(gx), ptr0(gres), ptr(gw), ptr(gb)))
        return (gx.to(x_dtype) if ctx.needs_input_grad[0] else None, None if gw is None else gw.to(w_dtype), None if gb is None else gb.to(b_dtype),
                None if gres is None else gres.to(r_dtype), None, None, None, None, None, None, None, None, None, None)


def _check_channel_vector(t, C, name, features, dtype=None):
    if t is None:
        return
    if not isinstance(t, torch.Tensor) or t.shape != (C,) or not (t.dtype.is_floating_point if dtype is None else t.dtype == dtype):
        raise RuntimeError(f'shape mismatch: sparse_batch_norm: {name} must be a {"floating-point" if dtype is None else dtype} ({C},) tensor, got '
                           f'{tuple(getattr(t, "shape", ()))} {getattr(t, "dtype", type(t).__name__)}')
    if t.device != features.device:
        raise RuntimeError(f'sparse_batch_norm: {name} is on {t.device}, features on {features.device}')
    if dtype is not None and not t.is_contiguous():
        raise RuntimeError(f'sparse_batch_norm: {name} is updated in place and must be contiguous')


def sparse_batch_norm(features, coors, spatial_shape, batch_size, weight, bias, running_mean, running_var, num_batches_tracked=None, *, training,
                      momentum=0.1, eps=1e-5, residual=None, activation=None):
    """act(batch_norm(features) + residual) over the LIVE rows of a sparse tensor -> (R, C), differentiable w.r.t. features, weight, bias
    and residual.

    features (R, C) fp32, fp16 or bf16 (another floating dtype is evaluated in fp32 and cast back), 1 <= C <= 256; coors (R, 4) integer rows
    [b, z, y, x], taken as `sparse_conv_index` takes them: a row with a negative entry, b >= batch_size or a coordinate outside
    `spatial_shape` is dead.  With n the number of live rows (counted on the device, never read back):

    training=True (or running_mean is None: `track_running_stats=False`): mean and biased var over the live rows, invstd = 1 / sqrt(var +
    eps), y = act((x - mean) * invstd * weight + bias + residual) on live rows; running_mean <- (1 - momentum) running_mean + momentum
    mean, running_var likewise with var * n / (n - 1), num_batches_tracked += 1, all three written on the device by the same call.
    n < 2 leaves the three untouched: n = 0 gives zeros, n = 1 gives act(bias + residual) on the one live row (`F.batch_norm` raises for one
    value per channel; a capturable call cannot know n).  training=False: y = act(x * scale + shift + residual), scale = weight /
    sqrt(running_var + eps), shift = bias - running_mean * scale; one launch.

    Dead rows of y, grad_features and grad_residual are EXACTLY zero whatever the dead rows of features and residual hold, NaN included;
    nothing a dead row holds can change a bit of any output.  weight, bias: (C,) or None (`affine=False`); statistics, weight, bias and
    their gradients are fp32; residual (R, C) of the features' dtype; activation None or 'relu'.  momentum=None (torch's cumulative
    average) raises.  The same bits from run to run and under graph replay; no atomics, no host read."""
    if not isinstance(features, torch.Tensor) or features.dim() != 2 or not features.dtype.is_floating_point:
        raise RuntimeError(f'shape mismatch: sparse_batch_norm: features must be a floating-point (R, C) tensor, got '
                           f'{tuple(getattr(features, "shape", ()))} {getattr(features, "dtype", type(features).__name__)}')
    R, C = features.shape
    if not 1 <= C <= MAX_CHANNELS:
        raise RuntimeError(f'sparse_batch_norm: 1 .. {MAX_CHANNELS} channels are supported, got {C}')
    if not isinstance(coors, torch.Tensor) or coors.dim() != 2 or coors.size(0) != R:
        raise RuntimeError(f'shape mismatch: sparse_batch_norm: coors must be an ({R}, 4) tensor [b, z, y, x], got {tuple(getattr(coors, "shape", ()))}')
    c = coors_i32(coors, 'sparse_batch_norm')
    if c.device != features.device:
        raise RuntimeError(f'sparse_batch_norm: coors is on {c.device}, features on {features.device}')
    shape, B = triple(spatial_shape, 'spatial_shape'), int(batch_size)
    if B < 0 or min(shape) < 1:
        raise RuntimeError(f'sparse_batch_norm: needs batch_size >= 0 and a positive spatial_shape, got {B}, {shape}')
    if momentum is None:
        raise RuntimeError('sparse_batch_norm: momentum=None (a cumulative moving average) is not supported: the update is written on the device '
                           'with a fixed momentum')
    check_activation(activation, 'sparse_batch_norm')
    _check_channel_vector(weight, C, 'weight', features)
    _check_channel_vector(bias, C, 'bias', features)
    if (running_mean is None) != (running_var is None):
        raise RuntimeError('sparse_batch_norm: running_mean and running_var come together or not at all')
    _check_channel_vector(running_mean, C, 'running_mean', features, torch.float32)
    _check_channel_vector(running_var, C, 'running_var', features, torch.float32)
    if num_batches_tracked is not None and (not isinstance(num_batches_tracked, torch.Tensor) or num_batches_tracked.numel() != 1
                                            or num_batches_tracked.dtype != torch.int64 or num_batches_tracked.device != features.device):
        raise RuntimeError(f'sparse_batch_norm: num_batches_tracked must hold one int64 on {features.device}')
    if residual is not None:
        if not isinstance(residual, torch.Tensor) or residual.shape != (R, C) or residual.dtype != features.dtype:
            raise RuntimeError(f'shape mismatch: sparse_batch_norm: residual must be a {features.dtype} ({R}, {C}) tensor, got '
                               f'{tuple(getattr(residual, "shape", ()))} {getattr(residual, "dtype", type(residual).__name__)}')
        if residual.device != features.device:
            raise RuntimeError(f'sparse_batch_norm: residual is on {residual.device}, features on {features.device}')
    return _SparseBatchNorm.apply(features, weight, bias, residual, c, running_mean, running_var, num_batches_tracked, shape, B, bool(training),
                                  momentum, eps, activation)


class SparseBatchNorm1d(nn.BatchNorm1d, SparseModule):
    """`nn.BatchNorm1d` for a `SparseConvTensor`: the constructor, parameters, buffers and `state_dict` keys of `nn.BatchNorm1d`, the
    statistics over the live rows alone, dead rows zero (`sparse_batch_norm`).  activation (keyword-only): None or 'relu', applied in the
    same pass.  forward(x, residual=None) returns a `SparseConvTensor` of x's lineage; residual: (R, C) features (or a tensor holding
    them) added before the activation — the identity of a basic block."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True, device=None, dtype=None, *, activation=None):
        check_activation(activation, 'SparseBatchNorm1d')
        super().__init__(num_features, eps, momentum, affine, track_running_stats, device=device, dtype=dtype)
        self.activation = activation

    @classmethod
    def from_batchnorm(cls, bn, activation=None):
        """a SparseBatchNorm1d that SHARES bn's parameters and buffers (nothing is copied), in bn's mode"""
        if not isinstance(bn, nn.BatchNorm1d):
            raise RuntimeError(f'SparseBatchNorm1d.from_batchnorm: only BatchNorm1d is converted, got {type(bn).__name__}')
        new = cls(bn.num_features, bn.eps, bn.momentum, False, False, activation=activation)
        new.affine, new.track_running_stats = bn.affine, bn.track_running_stats
        for name, p in bn._parameters.items():
            new._parameters[name] = p
        for name, b in bn._buffers.items():
            new._buffers[name] = b
        new.train(bn.training)
        return new

    def forward(self, x, residual=None):
        SparseConvTensor.expect(x, type(self).__name__)
        features = sparse_batch_norm(x.features, x.indices, x.spatial_shape, x.batch_size, self.weight, self.bias, self.running_mean, self.running_var,
                                     self.num_batches_tracked, training=self.training, momentum=self.momentum, eps=self.eps,
                                     residual=getattr(residual, 'features', residual), activation=self.activation)
        return x.derive(features)

    def extra_repr(self):
        return super().extra_repr() + f', activation={self.activation!r}'
