"""The bottom layer of the sparse stack: spconv 1.x's `SparseConvTensor`, `SparseModule`, `SparseSequential` and `ToDense`,
`sparse_to_dense` (`SparseConvTensor.dense()`; csrc/sparse_dense.hip), and what every op above shares — the limits and code tables of
include/gd3d.h and the argument helpers.  sparse_conv.py, sparse_bn.py and sparse_pool.py are built on this module and sparse_encoder.py on
those three; nothing here knows of them.
"""
import math
from collections import OrderedDict

import torch
from torch import nn

from . import _host

MAX_CHANNELS = 256
MAX_OFFSETS = 27
DTYPE_CODES = {torch.float16: 1, torch.bfloat16: 2}           # GD3D_DTYPE_F16, GD3D_DTYPE_BF16 (include/gd3d.h); fp32 is 0
ACT_CODES = {None: 0, 'relu': 1}                              # GD3D_ACT_NONE, GD3D_ACT_RELU (include/gd3d.h)


def triple(v, name):
    if isinstance(v, (list, tuple)):
        v = tuple(int(x) for x in v)
        if len(v) != 3:
            raise RuntimeError(f'{name} must be a number or hold 3 values (z, y, x), got {len(v)}')
        return v
    return (int(v),) * 3


def coors_i32(coors, who):
    if not isinstance(coors, torch.Tensor) or coors.dim() != 2 or coors.size(1) != 4:
        raise RuntimeError(f'shape mismatch: {who}: coors must be an (N, 4) tensor [b, z, y, x], got {tuple(getattr(coors, "shape", ()))}')
    if coors.dtype.is_floating_point or coors.dtype == torch.bool:
        raise RuntimeError(f'{who}: coors must be an integer tensor, got {coors.dtype}')
    c = coors if coors.dtype == torch.int32 else coors.to(torch.int32)
    return c if c.is_contiguous() else c.contiguous()


def kernel_dtype(t):
    """the dtype the kernels run `t` in: its own where that is fp32, fp16 or bf16, else fp32 (evaluated there and cast back)"""
    return t.dtype if t.dtype in DTYPE_CODES else torch.float32


def as_dtype(t, dtype):
    """t as a contiguous tensor of `dtype`; t itself when it already is"""
    if t.dtype != dtype:
        t = t.to(dtype)
    return t if t.is_contiguous() else t.contiguous()


def check_activation(activation, who):
    if activation not in ACT_CODES:
        raise RuntimeError(f"{who}: activation must be None or 'relu', got {activation!r}")


class _SparseToDense(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, coors, shape, B):
        half = features.dtype in DTYPE_CODES                                           # 2-byte elements are copied as they are
        x = features.contiguous() if half else _host.f32c(features)
        N, C, dev = x.size(0), x.size(1), x.device
        dense = torch.empty((B, C) + shape, dtype=x.dtype, device=dev)
        ptr = _host.ptr_or_null
        _host.call('gd3d_sparse_to_dense_16' if half else 'gd3d_sparse_to_dense', dev, (ptr(x), ptr(coors), N, C, B, *shape, ptr(dense)))
        ctx.save_for_backward(coors)
        ctx.state = (shape, B, N, C, features.dtype)
        return dense if features.dtype == dense.dtype else dense.to(features.dtype)

    @staticmethod
    @_host.guard_double_backward
    def backward(ctx, grad_dense):
        (coors,) = ctx.saved_tensors
        shape, B, N, C, dtype = ctx.state
        half = dtype in DTYPE_CODES and grad_dense.dtype == dtype
        g = grad_dense.contiguous() if half else _host.f32c(grad_dense)
        gx = torch.empty((N, C), dtype=g.dtype, device=g.device)
        ptr = _host.ptr_or_null
        _host.call('gd3d_sparse_to_dense_backward_16' if half else 'gd3d_sparse_to_dense_backward', g.device,
                   (ptr(g), ptr(coors), N, C, B, *shape, ptr(gx)))
        return gx.to(dtype), None, None, None


def sparse_to_dense(features, coors, spatial_shape, batch_size):
    """`SparseConvTensor.dense()` -> (B, C, D, H, W): zeros, then dense[b, :, z, y, x] = features[row] for every active row of coors
    (N, 4) [b, z, y, x]; a fill and one launch.  Differentiable w.r.t. features: the backward is one gather, zeros for an inactive row.
    fp16 / bf16 features are copied as 2-byte elements (no fp32 temporary); every other dtype goes through fp32."""
    shape = triple(spatial_shape, 'spatial_shape')
    c = coors_i32(coors, 'sparse_to_dense')
    if not isinstance(features, torch.Tensor) or features.dim() != 2 or features.size(0) != c.size(0) or not features.dtype.is_floating_point:
        raise RuntimeError(f'shape mismatch: sparse_to_dense: features must be a floating-point ({c.size(0)}, C) tensor, got '
                           f'{tuple(getattr(features, "shape", ()))}')
    B = int(batch_size)
    if min(shape) == 0 and B >= 0:                                                     # the shape of a layer without output cells
        return features.new_zeros((B, features.size(1)) + shape)
    if B < 0 or min(shape) < 1 or not 1 <= features.size(1) <= MAX_CHANNELS:
        raise RuntimeError(f'sparse_to_dense: needs batch_size >= 0, a positive spatial_shape and 1 .. {MAX_CHANNELS} channels, got {B}, {shape}, '
                           f'{features.size(1)}')
    if c.device != features.device:
        raise RuntimeError(f'sparse_to_dense: coors is on {c.device}, features on {features.device}')
    return _SparseToDense.apply(features, c, shape, B)


# ---- spconv 1.x's surface ------------------------------------------------------------------------------------------------------------

class SparseConvTensor:
    """spconv 1.x's tensor: features (N, C), indices (N, 4) int32 [b, z, y, x], spatial_shape (D, H, W), batch_size, and `indice_dict`
    — the indices built so far, by `indice_key`, shared along a tensor's lineage."""

    def __init__(self, features, indices, spatial_shape, batch_size, grid=None):
        self.features = features
        self.indices = indices
        self.spatial_shape = list(spatial_shape)
        self.batch_size = batch_size
        self.indice_dict = {}
        self.grid = grid

    @staticmethod
    def expect(x, who):
        """the guard of a module `who` on its input"""
        if not isinstance(x, SparseConvTensor):
            raise RuntimeError(f'{who} takes a SparseConvTensor, got {type(x).__name__}')

    def derive(self, features, indices=None, spatial_shape=None):
        """a tensor of this one's lineage (batch_size, grid, the SHARED indice_dict) that holds `features` — on these rows, or on `indices`
        and `spatial_shape` where a layer moved to other rows"""
        out = SparseConvTensor(features, self.indices if indices is None else indices, self.spatial_shape if spatial_shape is None else spatial_shape,
                               self.batch_size, self.grid)
        out.indice_dict = self.indice_dict
        return out

    @property
    def spatial_size(self):
        return math.prod(self.spatial_shape)

    def find_indice_pair(self, key):
        return None if key is None else self.indice_dict.get(key)

    def dense(self, channels_first=True):
        out = sparse_to_dense(self.features, self.indices, self.spatial_shape, self.batch_size)
        return out if channels_first else out.permute(0, 2, 3, 4, 1).contiguous()

    @property
    def sparity(self):
        return self.indices.shape[0] / max(1, self.spatial_size * self.batch_size)


class SparseModule(nn.Module):
    """Marks the modules that take and return a `SparseConvTensor` (everything else `SparseSequential` applies to `.features`)."""


class ToDense(SparseModule):
    """spconv 1.x's `ToDense`: `x.dense()` as a module -> (B, C, D, H, W)."""

    def forward(self, x):
        SparseConvTensor.expect(x, 'ToDense')
        return x.dense()


class SparseSequential(SparseModule):
    """spconv 1.x's container: sparse modules take the tensor, every other `nn.Module` (BatchNorm1d, ReLU) is applied to `.features`."""

    def __init__(self, *args, **kwargs):
        super().__init__()
        if len(args) == 1 and isinstance(args[0], OrderedDict):
            for key, module in args[0].items():
                self.add_module(key, module)
        else:
            for idx, module in enumerate(args):
                self.add_module(str(idx), module)
        for name, module in kwargs.items():
            if name in self._modules:
                raise ValueError('name exists.')
            self.add_module(name, module)

    def __getitem__(self, idx):
        if not -len(self) <= idx < len(self):
            raise IndexError(f'index {idx} is out of range')
        return list(self._modules.values())[idx]

    def __len__(self):
        return len(self._modules)

    def add(self, module, name=None):
        name = str(len(self._modules)) if name is None else name
        if name in self._modules:
            raise KeyError('name exists')
        self.add_module(name, module)

    def rewrite(self, step):
        """in place, the walk of every rewrite of a container (fusing, converting the norms): `step(modules, i)` looks at the module at
        position i of the list `modules` and at what follows it, and returns (the module that takes its place under its name, the next
        position to look at); the modules it skipped are gone"""
        names, modules = list(self._modules), list(self._modules.values())
        rewritten, i = OrderedDict(), 0
        while i < len(modules):
            name = names[i]
            rewritten[name], i = step(modules, i)
        self._modules = rewritten

    def forward(self, input):
        for module in self._modules.values():
            if isinstance(module, SparseModule):
                input = module(input)
            elif isinstance(input, SparseConvTensor):
                if input.indices.shape[0] != 0:
                    input.features = module(input.features)
            else:
                input = module(input)
        return input
