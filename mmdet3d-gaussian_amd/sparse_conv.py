"""Sparse 3D convolution: spconv 1.x's `SubMConv3d` / `SparseConv3d` / `SparseConvTensor` / `SparseSequential` as mmdet3d re-exports them
(`mmdet3d.ops.spconv`), mmdet3d's `SparseBasicBlock`, `make_sparse_convmodule` and `SparseEncoder`, and the reference's
`MlvlSparseEncoder` (models/middle_encoders/mlvl_sparse_encoder.py:11-32): PV-RCNN's `voxel_middle_encoder` and CenterPoint's
`pts_middle_encoder`.  mmdet3d and spconv are CUDA-only and absent from the reference tree: the op is RESTATED (include/gd3d.h,
DESIGN.md §3.18) — a sparse convolution equals the dense `conv3d` of the densified input read at the active output sites.

Three calls carry it (csrc/sparse_conv.hip, csrc/sparse_conv_wgrad.hip, csrc/sparse_dense.hip): `sparse_conv_index` builds the neighbour tables of one layer geometry in one stream-ordered
run of launches (64-bit keys, a stable radix sort, look-ups by lower bound; the outputs of a strided layer in ascending (b, z, y, x)
order, as spconv 1.x's GPU path gives them), `sparse_conv` evaluates a layer over a table (one launch forward; one for the input
gradient; three for the weight and bias gradients; no atomics, the bits replay), `sparse_to_dense` is `SparseConvTensor.dense()`.  CUDA
tensors go to the kernels on the current stream, CPU tensors to the library's `_cpu` twins.  By default fp32: another dtype is evaluated
in fp32 and cast back.  `compute_dtype=torch.float16 / torch.bfloat16 / 'auto'` (a keyword of `sparse_conv`, of every layer and of every
builder here) selects the mixed-precision form (csrc/sparse_conv_16.hip): 16-bit operands on the matrix cores, fp32
accumulation, a 16-bit output, fp32 weight and bias gradients.  `scale=, shift=, residual=, activation=` on `sparse_conv`, and
`fuse_sparse_conv_bn` / `SparseEncoder.fuse()` on the modules, put an eval BatchNorm, a block's residual add and the ReLU into the
forward launch.  Dilation must be 1.

The way back up: `sparse_conv_index` keeps the rows it was built over (`in_coors`, `in_shape`), and
`sparse_conv_index_inverse` hands the same tables back with the roles swapped, so `sparse_inverse_conv` / `SparseInverseConv3d` (spconv 1.x's
inverse convolution) are the launches above over `nbr_t` — no new kernel, every form included; `make_sparse_inverse_convmodule` is
mmdet3d's conv module around one.  `ToDense` is `x.dense()` as a module, `SparseUNet` mmdet3d's encoder-decoder middle encoder, which
returns per-voxel `seg_features` next to the BEV map.  Max pooling over the same tables lives in sparse_pool.py.
"""
import ctypes
import math
from collections import OrderedDict
from typing import NamedTuple, Optional

import torch
from torch import nn

from . import _host, _lib

MAX_CHANNELS = 256
MAX_OFFSETS = 27


class SparseConvIndex(NamedTuple):
    """The tables of one layer geometry over one set of input rows (include/gd3d.h, gd3d_sparse_conv_index)."""
    out_coors: torch.Tensor              # (R, 4) int32 [b, z, y, x]; -1 rows past num[0]
    out_shape: tuple                     # (oD, oH, oW)
    nbr: torch.Tensor                    # (R, K) int32: the input row output row o reads through offset j, or -1
    nbr_t: Optional[torch.Tensor]        # (N, K) int32: the output row that reads input row i through offset j, or -1; None for subm
    num: Optional[torch.Tensor]          # (2,) int64 on the device: rows kept, true count; None in an inverse view (every row counts)
    out_batch_cnt: Optional[torch.Tensor]   # (B,) int32: kept rows per sample; None in an inverse view
    subm: bool = False
    num_in: int = 0                      # N, the input rows the tables were built over
    in_coors: Optional[torch.Tensor] = None   # (N, 4) int32 contiguous: those rows (what `sparse_conv_index_inverse` hands back as outputs)
    in_shape: Optional[tuple] = None     # the input spatial_shape (D, H, W)


def _triple(v, name):
    if isinstance(v, (list, tuple)):
        v = tuple(int(x) for x in v)
        if len(v) != 3:
            raise RuntimeError(f'{name} must be a number or hold 3 values (z, y, x), got {len(v)}')
        return v
    return (int(v),) * 3


def _geometry(spatial_shape, kernel_size, stride, padding, subm, who):
    """(shape, kernel, stride, padding, out_shape) as int triples, validated as the C entry point validates them"""
    n, k, s, p = _triple(spatial_shape, 'spatial_shape'), _triple(kernel_size, 'kernel_size'), _triple(stride, 'stride'), _triple(padding, 'padding')
    if min(n) < 1 or min(k) < 1 or min(s) < 1 or min(p) < 0:
        raise RuntimeError(f'{who}: spatial_shape {n}, kernel_size {k} and stride {s} must be positive, padding {p} not negative')
    if k[0] * k[1] * k[2] > MAX_OFFSETS:
        raise RuntimeError(f'{who}: kernel_size {k} has more than {MAX_OFFSETS} offsets')
    if subm and any(ka % 2 == 0 or sa != 1 or pa != ka // 2 for ka, sa, pa in zip(k, s, p)):
        raise RuntimeError(f'{who}: a submanifold convolution needs odd kernel extents, stride 1 and padding k // 2, got kernel_size {k}, '
                           f'stride {s}, padding {p}')
    o = tuple(max(0, (na + 2 * pa - ka) // sa + 1) for na, ka, sa, pa in zip(n, k, s, p))     # 0: the kernel does not fit, no output
    return n, k, s, p, o


_index_workspace_bytes = _host.memo(lambda n, k, subm: _lib.load().gd3d_sparse_conv_index_workspace_bytes(n, k, subm))
_weight_workspace_bytes = _host.memo(lambda r, k, cin, cout: _lib.load().gd3d_sparse_conv_backward_weight_workspace_bytes(r, k, cin, cout))


def _workspace(nbytes, dev):
    return torch.empty((nbytes,), dtype=torch.uint8, device=dev) if dev.type == 'cuda' else None


def _coors_i32(coors, who):
    if not isinstance(coors, torch.Tensor) or coors.dim() != 2 or coors.size(1) != 4:
        raise RuntimeError(f'shape mismatch: {who}: coors must be an (N, 4) tensor [b, z, y, x], got {tuple(getattr(coors, "shape", ()))}')
    if coors.dtype.is_floating_point or coors.dtype == torch.bool:
        raise RuntimeError(f'{who}: coors must be an integer tensor, got {coors.dtype}')
    c = coors if coors.dtype == torch.int32 else coors.to(torch.int32)
    return c if c.is_contiguous() else c.contiguous()


def sparse_conv_index(coors, spatial_shape, batch_size, kernel_size, stride=1, padding=0, subm=False, max_out=None, dilation=1):
    """The neighbour tables of one layer -> `SparseConvIndex(out_coors, out_shape, nbr, nbr_t, num, out_batch_cnt)`.

    coors (N, 4) integer rows [b, z, y, x]; a row with a negative entry, b >= batch_size or a coordinate outside `spatial_shape` is
    inactive (the tail rows of `hard_voxelize(static=True)`): no output, nobody's neighbour.  Active rows must be unique.
    subm=True  : odd kernel, stride 1, padding k // 2 (anything else raises); the outputs are the inputs, R = N, no read-back.
    subm=False : out_shape = (n + 2p - k) // s + 1 (0 on an axis the kernel does not fit: no output); the active outputs in ascending (b, z, y, x) order.  max_out=None reads the count
                 back ONCE and returns exact-size views; an int gives the static, capturable form: R = max_out rows, the lowest keys
                 kept, the rows past num[0] holding -1, and nothing read back.
    Every output is an integer and replays bit for bit on the device, in the `_cpu` twin and in the numpy restatement of the tests."""
    if _triple(dilation, 'dilation') != (1, 1, 1):
        raise RuntimeError(f'sparse_conv_index: dilation must be 1, got {dilation}')
    subm = bool(subm)
    n, k, s, p, o = _geometry(spatial_shape, kernel_size, stride, padding, subm, 'sparse_conv_index')
    c = _coors_i32(coors, 'sparse_conv_index')
    B, N, K, dev = int(batch_size), c.size(0), k[0] * k[1] * k[2], c.device
    if B < 0:
        raise RuntimeError(f'sparse_conv_index: batch_size must not be negative, got {B}')
    if subm:
        R = N
    elif max_out is None:
        # what N rows can reach: every row feeds at most prod(ceil(k / s)) output cells
        R = min(N * math.prod(-(-ka // sa) for ka, sa in zip(k, s)), B * o[0] * o[1] * o[2])
    else:
        R = int(max_out)
        if R < 0:
            raise RuntimeError(f'sparse_conv_index: max_out must not be negative, got {R}')
    out_coors = torch.empty((R, 4), dtype=torch.int32, device=dev)
    nbr = torch.empty((R, K), dtype=torch.int32, device=dev)
    nbr_t = None if subm else torch.empty((N, K), dtype=torch.int32, device=dev)
    num = torch.empty((2,), dtype=torch.int64, device=dev)
    cnt = torch.empty((B,), dtype=torch.int32, device=dev)
    work = _workspace(_index_workspace_bytes(N, K, int(subm)), dev)
    i3 = ctypes.c_int32 * 3
    ptr = _host.ptr_or_null
    _host.call('gd3d_sparse_conv_index', dev,
               (ptr(c), N, B, i3(*n), i3(*k), i3(*s), i3(*p), int(subm), R, ptr(work), ptr(out_coors), ptr(nbr), ptr(nbr_t), num.data_ptr(),
                ptr(cnt)))
    if not subm and max_out is None:
        kept = int(num[0])                                                           # the one read-back
        out_coors, nbr = out_coors[:kept], nbr[:kept]
    return SparseConvIndex(out_coors, o, nbr, nbr_t, num, cnt, subm, N, c, n)


def sparse_conv_index_inverse(index):
    """The record of the INVERSE layer of a strided layer's `index`: the same tensors with the roles swapped, nothing built, nothing copied.

    nbr = index.nbr_t (N, K), nbr_t = index.nbr (R, K), out_coors = index.in_coors, out_shape = index.in_shape, num_in = R, subm = False.
    The offset numbering stays the forward layer's, as in spconv 1.x, whose inverse layer swaps the pair lists and keeps j.  num is None
    (every entry takes a null count: all N rows are considered; the rows that no kept output reaches hold -1 throughout and come out zero)
    and so is out_batch_cnt, which nothing here reads.  A submanifold index and a record without `in_coors` raise."""
    if not isinstance(index, SparseConvIndex):
        raise RuntimeError('sparse_conv_index_inverse: index must be the record sparse_conv_index returns')
    if index.subm or index.nbr_t is None:
        raise RuntimeError('sparse_conv_index_inverse: a submanifold index has no inverse layer (its outputs are its inputs); only the index of '
                           'a SparseConv3d can be inverted')
    if index.in_coors is None or index.in_shape is None:
        raise RuntimeError('sparse_conv_index_inverse: the record does not carry in_coors / in_shape (it was not made by sparse_conv_index)')
    return SparseConvIndex(index.in_coors, tuple(index.in_shape), index.nbr_t, index.nbr, None, None, False, index.nbr.size(0), None, None)


def _weight3(weight, who):
    if not isinstance(weight, torch.Tensor) or weight.dim() not in (3, 5) or not weight.dtype.is_floating_point:
        raise RuntimeError(f'shape mismatch: {who}: weight must be a floating-point (K, Cin, Cout) or (kz, ky, kx, Cin, Cout) tensor, got '
                           f'{tuple(getattr(weight, "shape", ()))}')
    return weight.reshape(-1, weight.size(-2), weight.size(-1))


def _backward_entries(x, w, gy, nbr, nbr_t, num, subm, need_x, need_w, has_bias, dtype):
    """the backward entries on contiguous operands of the kernels' types (dtype None: fp32) -> (gx, gw, gb) as the kernels wrote them,
    None where not asked for"""
    N, (K, Cin, Cout), R, dev = x.size(0), w.shape, nbr.size(0), x.device
    suffix, code = ('', ()) if dtype is None else ('_16', (_DTYPE_CODES[dtype],))
    ptr = _host.ptr_or_null
    gx = gw = gb = None
    if need_x:
        gx = torch.empty((N, Cin), dtype=dtype or torch.float32, device=dev)
        _host.call('gd3d_sparse_conv_backward_input' + suffix, dev,
                   (ptr(gy), ptr(w), ptr(nbr if subm else nbr_t), int(subm), N, R, K, Cin, Cout, *code, ptr(gx)))
    if need_w:
        gw = torch.empty((K, Cin, Cout), dtype=torch.float32, device=dev)              # fp32 also on the 16-bit path: master weights get unrounded gradients
        gb = torch.empty((Cout,), dtype=torch.float32, device=dev) if has_bias else None
        work = _workspace(_weight_workspace_bytes(R, K, Cin, Cout), dev)
        _host.call('gd3d_sparse_conv_backward_weight' + suffix, dev,
                   (ptr(x), ptr(gy), ptr(nbr), ptr(num), N, R, K, Cin, Cout, *code, ptr(work), ptr(gw), ptr(gb)))
    return gx, gw, gb


_DTYPE_CODES = {torch.float16: 1, torch.bfloat16: 2}          # GD3D_DTYPE_F16, GD3D_DTYPE_BF16 (include/gd3d.h)


def _autocast_dtype(device_type):
    """the autocast dtype of `device_type` where autocast is enabled for it, else None"""
    if device_type not in ('cuda', 'cpu'):
        return None
    return torch.get_autocast_dtype(device_type) if torch.is_autocast_enabled(device_type) else None


def _check_compute_dtype(compute_dtype, who):
    if compute_dtype is not None and not (isinstance(compute_dtype, str) and compute_dtype == 'auto') and compute_dtype not in _DTYPE_CODES:
        raise RuntimeError(f"{who}: compute_dtype must be None, torch.float16, torch.bfloat16 or 'auto', got {compute_dtype!r}")
    return compute_dtype


def _resolve_compute_dtype(compute_dtype, features):
    """None (the fp32 path), torch.float16 or torch.bfloat16.  'auto': the features' dtype if it is one of the two, else the autocast
    dtype where autocast is enabled for the features' device, else None"""
    if _check_compute_dtype(compute_dtype, 'sparse_conv') is None or compute_dtype in _DTYPE_CODES:
        return compute_dtype
    if features.dtype in _DTYPE_CODES:
        return features.dtype
    dtype = _autocast_dtype(features.device.type)
    return dtype if dtype in _DTYPE_CODES else None


def _as16(t, dtype):
    """t as a contiguous tensor of `dtype`; t itself when it already is"""
    if t.dtype != dtype:
        t = t.to(dtype)
    return t if t.is_contiguous() else t.contiguous()


_ACT_CODES = {None: 0, 'relu': 1}                             # GD3D_ACT_NONE, GD3D_ACT_RELU (include/gd3d.h)


class _SparseConv(torch.autograd.Function):
    """One layer over its tables, every form.  dtype None: fp32 operands; torch.float16 / torch.bfloat16: 16-bit features, weight, residual,
    grad_out and output, fp32 bias, scale, shift and parameter gradients.  residual, scale, shift, activation all None: the plain entry
    (gd3d_sparse_conv_forward[_16]); any of them given: conv -> * scale + shift -> + residual -> ReLU in ONE forward launch
    (gd3d_sparse_conv_forward_fused[_16]).  Differentiable w.r.t. features, weight, bias and residual; scale and shift are
    constants (a frozen BatchNorm).  The backward is the same entries in every form (`_backward_entries`)."""

    @staticmethod
    def forward(ctx, features, weight, bias, residual, scale, shift, nbr, nbr_t, num, subm, activation, dtype):
        if dtype is None:
            x, w, code = _host.f32c(features), _host.f32c(weight), ()
        else:
            x, w, code = _as16(features, dtype), _as16(weight, dtype), (_DTYPE_CODES[dtype],)
        b = None if bias is None else _host.f32c(bias)
        N, (K, Cin, Cout), R, dev = x.size(0), w.shape, nbr.size(0), x.device
        out = torch.empty((R, Cout), dtype=dtype or torch.float32, device=dev)
        ptr = _host.ptr_or_null
        if residual is None and scale is None and shift is None and activation is None:
            sc = None
            _host.call('gd3d_sparse_conv_forward' if dtype is None else 'gd3d_sparse_conv_forward_16', dev,
                       (ptr(x), ptr(w), ptr(b), ptr(nbr), ptr(num), N, R, K, Cin, Cout, *code, ptr(out)))
        else:
            res = None if residual is None else (_host.f32c(residual) if dtype is None else _as16(residual, dtype))
            sc = None if scale is None else _host.f32c(scale)
            sh = None if shift is None else _host.f32c(shift)
            if b is not None:                                                          # the conv's own bias, folded on the host: shift' = bias * scale + shift
                b = b if sc is None else b * sc
                sh = b if sh is None else b + sh
            _host.call('gd3d_sparse_conv_forward_fused' if dtype is None else 'gd3d_sparse_conv_forward_fused_16', dev,
                       (ptr(x), ptr(w), ptr(sc), ptr(sh), ptr(res), ptr(nbr), ptr(num), N, R, K, Cin, Cout, _ACT_CODES[activation], *code, ptr(out)))
        ctx.save_for_backward(x, w, nbr, nbr_t, num, sc, out if activation == 'relu' else None)
        ctx.state = (subm, bias is not None, features.dtype, weight.dtype, None if bias is None else bias.dtype,
                     None if residual is None else residual.dtype, weight.shape, dtype)
        return out if dtype is not None or features.dtype == torch.float32 else out.to(features.dtype)

    @staticmethod
    @_host.guard_double_backward
    def backward(ctx, grad_out):
        x, w, nbr, nbr_t, num, sc, out = ctx.saved_tensors
        subm, has_bias, x_dtype, w_dtype, b_dtype, r_dtype, w_shape, dtype = ctx.state
        g = grad_out if dtype is not None else _host.f32c(grad_out)
        if out is not None:
            g = g * (out > 0)                                                          # the ReLU's gradient, exact
        gres = g.to(r_dtype) if r_dtype is not None and ctx.needs_input_grad[3] else None
        gy = g if sc is None else g.float() * sc                                       # what reaches the convolution: the existing backward entries run on it
        gy = _host.f32c(gy) if dtype is None else _as16(gy, dtype)
        gx, gw, gb = _backward_entries(x, w, gy, nbr, nbr_t, num, subm, ctx.needs_input_grad[0],
                                       ctx.needs_input_grad[1] or (has_bias and ctx.needs_input_grad[2]), has_bias, dtype)
        gx = None if gx is None else gx.to(x_dtype)
        gw = None if gw is None else gw.to(w_dtype).reshape(w_shape)
        gb = None if gb is None else gb.to(b_dtype)
        return gx, gw, gb, gres, None, None, None, None, None, None, None, None


def _check_fused_operands(scale, shift, residual, activation, features, Cout, R):
    if activation not in _ACT_CODES:
        raise RuntimeError(f"sparse_conv: activation must be None or 'relu', got {activation!r}")
    for name, t in (('scale', scale), ('shift', shift)):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or t.shape != (Cout,) or not t.dtype.is_floating_point:
            raise RuntimeError(f'shape mismatch: sparse_conv: {name} must be a floating-point ({Cout},) tensor, got {tuple(getattr(t, "shape", ()))}')
        if t.requires_grad:
            raise RuntimeError(f'sparse_conv: {name} is a constant of the fused layer (a frozen BatchNorm) and must not require grad')
        if t.device != features.device:
            raise RuntimeError(f'sparse_conv: {name} is on {t.device}, features on {features.device}')
    if residual is not None:
        if not isinstance(residual, torch.Tensor) or residual.shape != (R, Cout) or not residual.dtype.is_floating_point:
            raise RuntimeError(f'shape mismatch: sparse_conv: residual must be a floating-point ({R}, {Cout}) tensor, got '
                               f'{tuple(getattr(residual, "shape", ()))}')
        if residual.device != features.device:
            raise RuntimeError(f'sparse_conv: residual is on {residual.device}, features on {features.device}')


def sparse_conv(features, weight, bias, index, compute_dtype=None, *, scale=None, shift=None, residual=None, activation=None):
    """One sparse convolution layer over the tables of `sparse_conv_index` -> (R, Cout), differentiable w.r.t. features, weight, bias.

    out[o] = sum over the offsets j with index.nbr[o, j] >= 0 of features[nbr[o, j]] @ weight[j] (+ bias); weight is spconv 1.x's
    (kz, ky, kx, Cin, Cout) or the flat (K, Cin, Cout).  A row without a valid neighbour — an inactive row of a submanifold layer, a tail row
    of the static form — is zero, bias or not, and takes no part in any gradient.  Forward: one launch; input gradient: one (the same
    kernel over the transposed table and weight); weight and bias gradients: per-chunk partial sums and one finishing launch.  No atomics
    anywhere: the same bits from run to run.

    compute_dtype=None: fp32 (another dtype is evaluated in fp32 and cast back).  torch.float16 / torch.bfloat16: the mixed-precision form —
    features and weight are cast to it (nothing is done where they already are), the bias stays fp32, the products are accumulated in fp32 on
    the matrix cores and rounded once; the output comes back in compute_dtype, grad_features in the features' dtype, and the weight and
    bias gradients are computed in fp32 and cast to the parameters' dtypes.  'auto': the features' dtype if it is one of the two, else the
    autocast dtype where autocast is enabled for the features' device, else None.

    scale, shift, residual, activation (keyword-only): the fused layer — ONE forward launch evaluates
    act((conv + bias) * scale + shift + residual) on the rows that have a valid neighbour and writes zero to every other row, whatever
    shift and residual hold.  scale, shift: (Cout,) constants (an eval BatchNorm folded: `fuse_sparse_conv_bn`), kept in fp32; a tensor that
    requires grad raises.  residual: (R, Cout), the identity of a basic block.  activation: None or 'relu'.  The conv's own bias is folded on
    the host, shift' = bias * scale + shift, and each output element is one fixed fp32 sequence — fmaf(acc, scale, shift'), + residual, the
    ReLU — rounded once on the 16-bit path.  Differentiable w.r.t. features, weight, bias and residual: g = grad_out * (out > 0) under the
    ReLU, grad_residual = g, and the backward launches above run on g * scale.  With all four None the call is the one it always was."""
    if not isinstance(index, SparseConvIndex):
        raise RuntimeError('sparse_conv: index must be the record sparse_conv_index returns')
    w = _weight3(weight, 'sparse_conv')
    K, Cin, Cout = w.shape
    if not isinstance(features, torch.Tensor) or features.dim() != 2 or features.size(1) != Cin or not features.dtype.is_floating_point:
        raise RuntimeError(f'shape mismatch: sparse_conv: features must be a floating-point (N, {Cin}) tensor, got {tuple(getattr(features, "shape", ()))}')
    if features.size(0) != index.num_in or index.nbr.size(1) != K:
        raise RuntimeError(f'shape mismatch: sparse_conv: the index was built over {index.num_in} rows and {index.nbr.size(1)} offsets, got '
                           f'{features.size(0)} rows and a weight of {K} offsets')
    if max(Cin, Cout) > MAX_CHANNELS or min(Cin, Cout) < 1:
        raise RuntimeError(f'sparse_conv: 1 .. {MAX_CHANNELS} channels are supported, got {Cin} -> {Cout}')
    if bias is not None and (not isinstance(bias, torch.Tensor) or bias.shape != (Cout,)):
        raise RuntimeError(f'shape mismatch: sparse_conv: bias must be ({Cout},), got {tuple(getattr(bias, "shape", ()))}')
    for name, t in (('weight', weight), ('bias', bias), ('index', index.nbr)):
        if t is not None and t.device != features.device:
            raise RuntimeError(f'sparse_conv: {name} is on {t.device}, features on {features.device}')
    dtype = _resolve_compute_dtype(compute_dtype, features)
    if scale is not None or shift is not None or residual is not None or activation is not None:
        _check_fused_operands(scale, shift, residual, activation, features, Cout, index.nbr.size(0))
    return _SparseConv.apply(features, w, bias, residual, scale, shift, index.nbr, index.nbr_t, index.num, index.subm, activation, dtype)


def sparse_inverse_conv(features, weight, bias, index, compute_dtype=None, *, scale=None, shift=None, residual=None, activation=None):
    """spconv 1.x's inverse convolution over the tables of the FORWARD layer's `index` (a strided `sparse_conv_index`) -> (N, Cout):
    `sparse_conv` over `sparse_conv_index_inverse(index)` — the same launches, forward and backward, the 16-bit and the fused forms included.

    out[i] = sum over the offsets j with index.nbr_t[i, j] >= 0 of features[nbr_t[i, j]] @ weight[j] (+ bias), features (R, Cin) on the
    forward layer's output rows, out on its input rows; weight (kz, ky, kx, Cin, Cout) or (K, Cin, Cout), the offset j numbered as in the
    forward layer.  It equals the dense `conv_transpose3d` of the densified features read at the forward layer's input sites.
    The rule for a row without a valid neighbour holds: that row is ZERO, bias or not — an inactive input row, an active input that no
    output cell reaches (a stride above the kernel, a truncated edge), an input whose outputs were all dropped by `max_out`.  spconv writes
    the bias to such a row; mmdet3d builds these layers without bias, where the two agree."""
    return sparse_conv(features, weight, bias, sparse_conv_index_inverse(index), compute_dtype, scale=scale, shift=shift, residual=residual,
                       activation=activation)


class _SparseToDense(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, coors, shape, B):
        half = features.dtype in _DTYPE_CODES                                          # 2-byte elements are copied as they are
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
        half = dtype in _DTYPE_CODES and grad_dense.dtype == dtype
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
    shape = _triple(spatial_shape, 'spatial_shape')
    c = _coors_i32(coors, 'sparse_to_dense')
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


class SparseConvolution(SparseModule):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, bias=True, subm=False, indice_key=None,
                 max_out=None, *, compute_dtype=None):
        super().__init__()
        self.compute_dtype = _check_compute_dtype(compute_dtype, type(self).__name__)     # None, torch.float16, torch.bfloat16 or 'auto': `sparse_conv`
        if _triple(dilation, 'dilation') != (1, 1, 1):
            raise RuntimeError(f'{type(self).__name__}: dilation must be 1, got {dilation}')
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.kernel_size = _triple(kernel_size, 'kernel_size')
        self.subm = bool(subm)
        # a submanifold layer pads by k // 2 whatever it is handed, as spconv does
        self.stride = (1, 1, 1) if self.subm else _triple(stride, 'stride')
        self.padding = tuple(k // 2 for k in self.kernel_size) if self.subm else _triple(padding, 'padding')
        self.dilation = (1, 1, 1)
        self.indice_key = indice_key
        self.max_out = max_out
        if not 1 <= self.in_channels <= MAX_CHANNELS or not 1 <= self.out_channels <= MAX_CHANNELS:
            raise RuntimeError(f'{type(self).__name__}: 1 .. {MAX_CHANNELS} channels are supported, got {in_channels} -> {out_channels}')
        if math.prod(self.kernel_size) > MAX_OFFSETS or min(self.kernel_size) < 1:
            raise RuntimeError(f'{type(self).__name__}: kernel_size {self.kernel_size} must hold 1 .. {MAX_OFFSETS} offsets')
        if self.subm and any(k % 2 == 0 for k in self.kernel_size):
            raise RuntimeError(f'{type(self).__name__}: a submanifold convolution needs odd kernel extents, got {self.kernel_size}')
        self.weight = nn.Parameter(torch.empty(*self.kernel_size, self.in_channels, self.out_channels))
        self.bias = nn.Parameter(torch.empty(self.out_channels)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        bound = 1.0 / math.sqrt(math.prod(self.kernel_size) * self.in_channels)   # kaiming_uniform_(a=sqrt(5)) over fan_in = K * Cin
        nn.init.uniform_(self.weight, -bound, bound)
        if self.bias is not None:
            nn.init.uniform_(self.bias, -bound, bound)

    def build_index(self, x):
        return sparse_conv_index(x.indices, x.spatial_shape, x.batch_size, self.kernel_size, self.stride, self.padding, self.subm, self.max_out)

    def index_of(self, x):
        """the index of this layer over x's rows: the one stored under `indice_key`, or a new one (stored under the key)"""
        if not isinstance(x, SparseConvTensor):
            raise RuntimeError(f'{type(self).__name__} takes a SparseConvTensor, got {type(x).__name__}')
        index = x.find_indice_pair(self.indice_key)
        if index is not None and (index.num_in != x.features.size(0) or index.subm != self.subm or index.nbr.size(1) != math.prod(self.kernel_size)):
            raise RuntimeError(f'{type(self).__name__}: the index stored under indice_key {self.indice_key!r} was built for another layer '
                               'geometry or another set of rows')
        if index is None:
            index = self.build_index(x)
            if self.indice_key is not None:
                x.indice_dict[self.indice_key] = index
        return index

    def output_of(self, x, index, features):
        """the layer's output tensor: `features` on the output rows of `index`, x's lineage"""
        out = SparseConvTensor(features, x.indices if self.subm else index.out_coors, index.out_shape, x.batch_size, x.grid)
        out.indice_dict = x.indice_dict
        return out

    def forward(self, x):
        index = self.index_of(x)
        return self.output_of(x, index, sparse_conv(x.features, self.weight, self.bias, index, self.compute_dtype))

    def extra_repr(self):
        return (f'{self.in_channels}, {self.out_channels}, kernel_size={self.kernel_size}, stride={self.stride}, padding={self.padding}, '
                f'bias={self.bias is not None}, indice_key={self.indice_key!r}'
                + ('' if self.compute_dtype is None else f', compute_dtype={self.compute_dtype!r}'))


class SubMConv3d(SparseConvolution):
    """spconv 1.x's submanifold convolution: the outputs are the inputs.  `stride` and `padding` are accepted and not used (k // 2)."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, bias=True, indice_key=None, *, compute_dtype=None):
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, bias, True, indice_key, compute_dtype=compute_dtype)


class SparseConv3d(SparseConvolution):
    """spconv 1.x's regular sparse convolution.  max_out (an addition): an int gives the static form of `sparse_conv_index`."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, bias=True, indice_key=None, max_out=None, *,
                 compute_dtype=None):
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, bias, False, indice_key, max_out,
                         compute_dtype=compute_dtype)


class SparseInverseConv3d(SparseConvolution):
    """spconv 1.x's inverse convolution (its positional signature): undoes the geometry of the `SparseConv3d` that stored its index under
    `indice_key` — the output lies on that layer's INPUT rows (`indices`, `spatial_shape`), through the same tables with the roles swapped
    (`sparse_inverse_conv`).  Builds nothing and leaves `indice_dict` as it was; a missing key raises.  A row without a valid neighbour is
    zero, bias or not (spconv writes the bias there)."""

    def __init__(self, in_channels, out_channels, kernel_size, indice_key, bias=True, *, compute_dtype=None):
        super().__init__(in_channels, out_channels, kernel_size, 1, 0, 1, bias, False, indice_key, compute_dtype=compute_dtype)

    def build_index(self, x):
        raise RuntimeError(f'{type(self).__name__} builds no index: it needs the one a SparseConv3d stored under indice_key {self.indice_key!r}')

    def index_of(self, x):
        """the inverse view of the index stored under `indice_key` (`sparse_conv_index_inverse`); x must lie on that layer's output rows"""
        if not isinstance(x, SparseConvTensor):
            raise RuntimeError(f'{type(self).__name__} takes a SparseConvTensor, got {type(x).__name__}')
        index = x.find_indice_pair(self.indice_key)
        if index is None:
            raise RuntimeError(f'{type(self).__name__}: no index is stored under indice_key {self.indice_key!r}: the SparseConv3d it inverts must '
                               'run first, with the same key, on this tensor\'s lineage')
        if index.subm:
            raise RuntimeError(f'{type(self).__name__}: the index stored under indice_key {self.indice_key!r} is a submanifold layer\'s: there is '
                               'nothing to invert')
        if index.nbr.size(1) != math.prod(self.kernel_size) or index.nbr.size(0) != x.features.size(0):
            raise RuntimeError(f'{type(self).__name__}: the index stored under indice_key {self.indice_key!r} has {index.nbr.size(1)} offsets and '
                               f'{index.nbr.size(0)} output rows, this layer {math.prod(self.kernel_size)} offsets and the tensor '
                               f'{x.features.size(0)} rows')
        return sparse_conv_index_inverse(index)

    def extra_repr(self):
        return (f'{self.in_channels}, {self.out_channels}, kernel_size={self.kernel_size}, bias={self.bias is not None}, '
                f'indice_key={self.indice_key!r}' + ('' if self.compute_dtype is None else f', compute_dtype={self.compute_dtype!r}'))


class ToDense(SparseModule):
    """spconv 1.x's `ToDense`: `x.dense()` as a module -> (B, C, D, H, W)."""

    def forward(self, x):
        if not isinstance(x, SparseConvTensor):
            raise RuntimeError(f'ToDense takes a SparseConvTensor, got {type(x).__name__}')
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


def _norm1d(norm_cfg, channels):
    cfg = dict(norm_cfg or dict(type='BN1d'))
    kind = cfg.pop('type', 'BN1d')
    if kind not in ('BN1d', 'BN'):
        raise RuntimeError(f'norm_cfg type {kind!r}: only BN1d is built here')
    cfg.pop('requires_grad', None)
    return nn.BatchNorm1d(channels, **cfg)


class SparseBasicBlock(SparseModule):
    """mmdet3d's sparse residual block: conv -> norm -> relu -> conv -> norm -> add identity -> relu, both SubMConv3d k3 without bias.
    indice_key (an addition): one index for both layers; the result does not depend on it."""
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None, conv_cfg=None, norm_cfg=None, indice_key=None, compute_dtype=None):
        super().__init__()
        if conv_cfg is not None and conv_cfg.get('type', 'SubMConv3d') != 'SubMConv3d':
            raise RuntimeError(f'SparseBasicBlock is built from SubMConv3d, got conv_cfg {conv_cfg}')
        self.conv1 = SubMConv3d(inplanes, planes, 3, stride, padding=1, bias=False, indice_key=indice_key, compute_dtype=compute_dtype)
        self.norm1 = _norm1d(norm_cfg, planes)
        self.conv2 = SubMConv3d(planes, planes, 3, padding=1, bias=False, indice_key=indice_key, compute_dtype=compute_dtype)
        self.norm2 = _norm1d(norm_cfg, planes)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample

    def forward(self, x):
        identity = x.features
        out = self.conv1(x)
        out.features = self.relu(self.norm1(out.features))
        out = self.conv2(out)
        out.features = self.norm2(out.features)
        if self.downsample is not None:
            identity = self.downsample(x)
        out.features = self.relu(out.features + identity)
        return out


def _convmodule(who, types, in_channels, out_channels, kernel_size, indice_key, stride, padding, conv_type, norm_cfg, order, compute_dtype):
    """the layers of `order` — conv (no bias) of one of `types`, BatchNorm1d(eps, momentum from norm_cfg), ReLU — in a `SparseSequential`"""
    if not isinstance(order, tuple) or len(order) > 3 or not set(order) <= {'conv', 'norm', 'act'}:
        raise RuntimeError(f"{who}: order must be a tuple over 'conv', 'norm', 'act', got {order!r}")
    if 'conv' in order and conv_type not in types:
        raise RuntimeError(f'{who}: conv_type {conv_type!r} is not built here ({", ".join(types)})')
    layers = []
    for layer in order:
        if layer == 'conv':
            if conv_type == 'SubMConv3d':
                layers.append(SubMConv3d(in_channels, out_channels, kernel_size, stride, padding, bias=False, indice_key=indice_key,
                                         compute_dtype=compute_dtype))
            elif conv_type == 'SparseConv3d':
                layers.append(SparseConv3d(in_channels, out_channels, kernel_size, stride, padding, bias=False, indice_key=indice_key,
                                           compute_dtype=compute_dtype))
            else:                                                                      # stride and padding are not used, as in mmdet3d
                layers.append(SparseInverseConv3d(in_channels, out_channels, kernel_size, indice_key, bias=False, compute_dtype=compute_dtype))
        elif layer == 'norm':
            layers.append(_norm1d(norm_cfg, out_channels))
        else:
            layers.append(nn.ReLU(inplace=True))
    return SparseSequential(*layers)


def make_sparse_convmodule(in_channels, out_channels, kernel_size, indice_key, stride=1, padding=0, conv_type='SubMConv3d', norm_cfg=None,
                           order=('conv', 'norm', 'act'), compute_dtype=None):
    """mmdet3d's sparse conv module: the layers of `order` — conv (no bias), BatchNorm1d(eps, momentum from norm_cfg), ReLU — in a
    `SparseSequential`.  compute_dtype (an addition) is handed to the conv.  conv_type: 'SubMConv3d' or 'SparseConv3d'; the module around a
    'SparseInverseConv3d' is built by `make_sparse_inverse_convmodule`."""
    return _convmodule('make_sparse_convmodule', ('SubMConv3d', 'SparseConv3d'), in_channels, out_channels, kernel_size, indice_key, stride, padding,
                       conv_type, norm_cfg, order, compute_dtype)


def make_sparse_inverse_convmodule(in_channels, out_channels, kernel_size, indice_key, norm_cfg=None, order=('conv', 'norm', 'act'),
                                   compute_dtype=None):
    """mmdet3d's `make_sparse_convmodule(conv_type='SparseInverseConv3d')`: a `SparseInverseConv3d` (no bias) over the index stored under
    `indice_key`, BatchNorm1d and ReLU in the order of `order`, in a `SparseSequential`.  mmdet3d ignores stride and padding for this type;
    here they are not taken."""
    return _convmodule('make_sparse_inverse_convmodule', ('SparseInverseConv3d',), in_channels, out_channels, kernel_size, indice_key, 1, 0,
                       'SparseInverseConv3d', norm_cfg, order, compute_dtype)


# ---- conv + BatchNorm + residual + ReLU in one launch ----------------------------------------------------------------

def _fold_batchnorm(bn):
    """an eval-mode BatchNorm1d as y = x * scale + shift -> (scale, shift), computed in fp64 and kept in fp32"""
    if not isinstance(bn, nn.BatchNorm1d):
        raise RuntimeError(f'fuse_sparse_conv_bn: only BatchNorm1d is folded, got {type(bn).__name__}')
    if bn.training:
        raise RuntimeError('fuse_sparse_conv_bn: a BatchNorm in training mode normalises by batch statistics and cannot be folded; call .eval() first')
    if bn.running_mean is None or bn.running_var is None:
        raise RuntimeError('fuse_sparse_conv_bn: a BatchNorm without running statistics (track_running_stats=False) cannot be folded')
    mean, var = bn.running_mean.detach().double(), bn.running_var.detach().double()
    gamma = torch.ones_like(var) if bn.weight is None else bn.weight.detach().double()
    beta = torch.zeros_like(var) if bn.bias is None else bn.bias.detach().double()
    scale = gamma / torch.sqrt(var + bn.eps)
    return scale.float(), (beta - mean * scale).float()


class FusedSparseConv(SparseModule):
    """A `SubMConv3d` / `SparseConv3d` with the eval BatchNorm1d and / or the ReLU that followed it, evaluated in ONE launch
    (`sparse_conv(..., scale, shift, residual, activation)`).  `conv` is the layer itself: its parameters, `indice_key`, `max_out` and
    `compute_dtype` are shared, not copied.  scale, shift: fp32 buffers (None without a BatchNorm).  forward(x, residual=None)."""

    def __init__(self, conv, norm=None, activation=None):
        super().__init__()
        if not isinstance(conv, SparseConvolution):
            raise RuntimeError(f'FusedSparseConv: conv must be a SubMConv3d or a SparseConv3d, got {type(conv).__name__}')
        if activation not in _ACT_CODES:
            raise RuntimeError(f"FusedSparseConv: activation must be None or 'relu', got {activation!r}")
        scale, shift = (None, None) if norm is None else _fold_batchnorm(norm)
        if scale is not None and scale.numel() != conv.out_channels:
            raise RuntimeError(f'FusedSparseConv: the BatchNorm has {scale.numel()} features, the convolution {conv.out_channels} output channels')
        self.conv = conv
        self.register_buffer('scale', None if scale is None else scale.to(conv.weight.device))
        self.register_buffer('shift', None if shift is None else shift.to(conv.weight.device))
        self.activation = activation

    indice_key = property(lambda self: self.conv.indice_key)
    max_out = property(lambda self: self.conv.max_out)
    compute_dtype = property(lambda self: self.conv.compute_dtype)

    def forward(self, x, residual=None):
        conv = self.conv
        index = conv.index_of(x)
        return conv.output_of(x, index, sparse_conv(x.features, conv.weight, conv.bias, index, conv.compute_dtype, scale=self.scale, shift=self.shift,
                                                    residual=residual, activation=self.activation))

    def extra_repr(self):
        return (f'norm={self.scale is not None}, activation={self.activation!r}, indice_key={self.indice_key!r}, max_out={self.max_out!r}'
                + ('' if self.compute_dtype is None else f', compute_dtype={self.compute_dtype!r}'))


class FusedSparseBasicBlock(SparseModule):
    """A `SparseBasicBlock` in two launches: conv1 + norm1 + relu, then conv2 + norm2 + identity + relu.  A `downsample` is evaluated first."""

    def __init__(self, block):
        super().__init__()
        if not isinstance(block, SparseBasicBlock):
            raise RuntimeError(f'FusedSparseBasicBlock: block must be a SparseBasicBlock, got {type(block).__name__}')
        self.conv1 = FusedSparseConv(block.conv1, block.norm1, 'relu')
        self.conv2 = FusedSparseConv(block.conv2, block.norm2, 'relu')
        self.downsample = None if block.downsample is None else fuse_sparse_conv_bn(block.downsample)

    def forward(self, x):
        identity = x.features
        if self.downsample is not None:
            identity = self.downsample(x)
        return self.conv2(self.conv1(x), residual=getattr(identity, 'features', identity))


def _fuse_sequential(seq):
    """in place: every conv of `seq` that is followed by an eval BatchNorm1d and / or an nn.ReLU becomes one FusedSparseConv under the
    conv's name; a conv that nothing follows (a pre-activation order) stays"""
    items, fused, i = list(seq._modules.items()), OrderedDict(), 0
    while i < len(items):
        name, module = items[i]
        i += 1
        if type(module) in (SubMConv3d, SparseConv3d, SparseInverseConv3d, SparseConvolution):
            norm = act = None
            if i < len(items) and isinstance(items[i][1], nn.modules.batchnorm._BatchNorm):
                norm, i = items[i][1], i + 1
                if getattr(norm, 'activation', None) == 'relu':                        # a SparseBatchNorm1d carries its ReLU (sparse_bn.py)
                    act = 'relu'
            if act is None and i < len(items) and isinstance(items[i][1], nn.ReLU):
                act, i = 'relu', i + 1
            if norm is not None or act is not None:
                module = FusedSparseConv(module, norm, act)
        fused[name] = module
    seq._modules = fused


def fuse_sparse_conv_bn(module):
    """mmcv's `fuse_conv_bn` for the sparse encoder: in place, and returns the module (a `SparseBasicBlock` handed in directly comes back
    as its fused replacement).  Inside every `SparseSequential` a `SubMConv3d` / `SparseConv3d` followed by an eval-mode `BatchNorm1d` and / or
    an `nn.ReLU` becomes a `FusedSparseConv`; every `SparseBasicBlock` becomes a `FusedSparseBasicBlock`.  scale = gamma / sqrt(running_var
    + eps) and shift = beta - running_mean * scale are computed in fp64 and held as fp32 buffers (affine=False: gamma = 1, beta = 0).  A
    BatchNorm in training mode, or one without running statistics, raises.  For inference and frozen-BN fine-tuning: the fused layers stay
    differentiable w.r.t. the conv's parameters and their input.  In the static `max_out` form the rows past the count come out zero, as
    `sparse_conv` promises, where the unfused BatchNorm turned them into `shift`.  An eval `SparseBatchNorm1d` (sparse_bn.py) folds as a
    `BatchNorm1d` does and its `activation` is carried into the `FusedSparseConv`; a converted basic block fuses to the same
    `FusedSparseBasicBlock`."""
    if isinstance(module, SparseBasicBlock):
        return FusedSparseBasicBlock(module)
    for name, child in list(module.named_children()):
        module._modules[name] = fuse_sparse_conv_bn(child)
    if isinstance(module, SparseSequential):
        _fuse_sequential(module)
    return module


class SparseEncoder(nn.Module):
    """mmdet3d 0.x's `SparseEncoder`, restated from its published sparse_encoder.py (absent from the reference tree: not pinned):
    CenterPoint's `pts_middle_encoder` (configs/_base_/models/centerpoint_01voxel_second_secfpn_nus.py:10-19).  forward returns
    `spatial_features`: conv_out's dense() viewed as (B, C * D, H, W)."""

    def __init__(self, in_channels, sparse_shape, order=('conv', 'norm', 'act'), norm_cfg=dict(type='BN1d', eps=1e-3, momentum=0.01),
                 base_channels=16, output_channels=128, encoder_channels=((16,), (32, 32, 32), (64, 64, 64), (64, 64, 64)),
                 encoder_paddings=((1,), (1, 1, 1), (1, 1, 1), ((0, 1, 1), 1, 1)), block_type='conv_module', compute_dtype=None):
        super().__init__()
        if block_type not in ('conv_module', 'basicblock'):
            raise RuntimeError(f"block_type must be 'conv_module' or 'basicblock', got {block_type!r}")
        if not isinstance(order, tuple) or len(order) != 3 or set(order) != {'conv', 'norm', 'act'}:
            raise RuntimeError(f"order must be a permutation of ('conv', 'norm', 'act'), got {order!r}")
        self.sparse_shape = list(sparse_shape)
        self.in_channels, self.order, self.base_channels, self.output_channels = in_channels, order, base_channels, output_channels
        self.encoder_channels, self.encoder_paddings = encoder_channels, encoder_paddings
        self.stage_num = len(encoder_channels)
        self.fp16_enabled = False                 # mmdet3d's attribute, inert here: compute_dtype='auto' is what follows autocast and the fp16 hook
        self.compute_dtype = _check_compute_dtype(compute_dtype, type(self).__name__)    # handed to every conv built below
        self.conv_input = make_sparse_convmodule(in_channels, base_channels, 3, norm_cfg=norm_cfg, padding=1, indice_key='subm1',
                                                 conv_type='SubMConv3d', order=order if order[0] == 'conv' else ('conv',),
                                                 compute_dtype=compute_dtype)
        encoder_out_channels = self.make_encoder_layers(make_sparse_convmodule, norm_cfg, base_channels, block_type=block_type)
        self.conv_out = make_sparse_convmodule(encoder_out_channels, output_channels, kernel_size=(3, 1, 1), stride=(2, 1, 1), norm_cfg=norm_cfg,
                                               padding=0, indice_key='spconv_down2', conv_type='SparseConv3d', compute_dtype=compute_dtype)

    def make_encoder_layers(self, make_block, norm_cfg, in_channels, block_type='conv_module', conv_cfg=dict(type='SubMConv3d')):
        self.encoder_layers = SparseSequential()
        out_channels = in_channels
        for i, blocks in enumerate(self.encoder_channels):
            blocks_list = []
            for j, out_channels in enumerate(tuple(blocks)):
                padding = tuple(self.encoder_paddings[i])[j]
                if i != 0 and j == 0 and block_type == 'conv_module':     # every stage but the first starts with the strided layer
                    blocks_list.append(make_block(in_channels, out_channels, 3, norm_cfg=norm_cfg, stride=2, padding=padding,
                                                  indice_key=f'spconv{i + 1}', conv_type='SparseConv3d', compute_dtype=self.compute_dtype))
                elif block_type == 'basicblock':
                    if j == len(blocks) - 1 and i != len(self.encoder_channels) - 1:
                        blocks_list.append(make_block(in_channels, out_channels, 3, norm_cfg=norm_cfg, stride=2, padding=padding,
                                                      indice_key=f'spconv{i + 1}', conv_type='SparseConv3d', compute_dtype=self.compute_dtype))
                    else:
                        blocks_list.append(SparseBasicBlock(out_channels, out_channels, norm_cfg=norm_cfg, conv_cfg=conv_cfg,
                                                            indice_key=f'subm{i + 1}', compute_dtype=self.compute_dtype))
                else:
                    blocks_list.append(make_block(in_channels, out_channels, 3, norm_cfg=norm_cfg, padding=padding, indice_key=f'subm{i + 1}',
                                                  conv_type='SubMConv3d', compute_dtype=self.compute_dtype))
                in_channels = out_channels
            self.encoder_layers.add_module(f'encoder_layer{i + 1}', SparseSequential(*blocks_list))
        return out_channels

    def encode(self, voxel_features, coors, batch_size):
        """-> (the stages' SparseConvTensors, conv_out's dense() viewed as (B, C * D, H, W))"""
        x = self.conv_input(SparseConvTensor(voxel_features, coors.int(), self.sparse_shape, batch_size))
        encode_features = []
        for encoder_layer in self.encoder_layers:
            x = encoder_layer(x)
            encode_features.append(x)
        spatial_features = self.conv_out(encode_features[-1]).dense()
        N, C, D, H, W = spatial_features.shape
        return encode_features, spatial_features.view(N, C * D, H, W)

    def forward(self, voxel_features, coors, batch_size):
        return self.encode(voxel_features, coors, batch_size)[1]

    def fuse(self):
        """`fuse_sparse_conv_bn` on this encoder (in eval mode): every conv -> BatchNorm1d -> ReLU and every basic block in fused launches"""
        return fuse_sparse_conv_bn(self)

    def convert_norm(self):
        """`convert_sparse_batchnorm` on this encoder (opt-in, in place): every BatchNorm1d (+ ReLU) and every basic block on the live-row
        `SparseBatchNorm1d` — what training in the static form needs; `.eval().fuse()` still works afterwards"""
        from .sparse_bn import convert_sparse_batchnorm
        return convert_sparse_batchnorm(self)


class MlvlSparseEncoder(SparseEncoder):
    """The reference's `MlvlSparseEncoder` (models/middle_encoders/mlvl_sparse_encoder.py:11-32), PV-RCNN's `voxel_middle_encoder`:
    forward returns dict(encode_features = every stage's SparseConvTensor, spatial_features)."""

    def forward(self, voxel_features, coors, batch_size):
        encode_features, spatial_features = self.encode(voxel_features, coors, batch_size)
        return dict(encode_features=encode_features, spatial_features=spatial_features)


class SparseUNet(SparseEncoder):
    """mmdet3d 0.x's `SparseUNet` middle encoder (Part-A2's), restated from its published sparse_unet.py (absent from the reference tree: not
    pinned): `SparseEncoder`'s conv_input, encoder_layers and conv_out, and a decoder that goes back up stage by stage.  Decoder block n
    (4 .. 1): `lateral_layer{n}` a `SparseBasicBlock` on 'subm{n}', `merge_layer{n}` a SubMConv3d module over the concatenated [bottom,
    lateral] features on 'subm{n}', `upsample_layer{n}` a `SparseInverseConv3d` module over the index the encoder stored under 'spconv{n}'
    (block 1: a SubMConv3d module on 'subm1').  The decoder builds no index of its own.
    forward returns dict(spatial_features (B, C * D, H, W), seg_features (num_voxels, decoder_channels[-1][-1])): per-voxel features on the
    input voxels, in the input's row order."""

    def __init__(self, in_channels, sparse_shape, order=('conv', 'norm', 'act'), norm_cfg=dict(type='BN1d', eps=1e-3, momentum=0.01),
                 base_channels=16, output_channels=128, encoder_channels=((16,), (32, 32, 32), (64, 64, 64), (64, 64, 64)),
                 encoder_paddings=((1,), (1, 1, 1), (1, 1, 1), ((0, 1, 1), 1, 1)),
                 decoder_channels=((64, 64, 64), (64, 64, 32), (32, 32, 16), (16, 16, 16)), decoder_paddings=((1, 0), (1, 0), (0, 0), (0, 1)),
                 compute_dtype=None):
        super().__init__(in_channels, sparse_shape, order, norm_cfg, base_channels, output_channels, encoder_channels, encoder_paddings,
                         'conv_module', compute_dtype)
        if len(decoder_channels) != len(encoder_channels) or any(len(tuple(c)) != 3 for c in decoder_channels):
            raise RuntimeError(f'SparseUNet: decoder_channels must hold one (lateral, merge, upsample) triple per encoder stage, got {decoder_channels!r}')
        self.decoder_channels, self.decoder_paddings = decoder_channels, decoder_paddings
        self.make_decoder_layers(norm_cfg, tuple(encoder_channels[-1])[-1])

    def make_decoder_layers(self, norm_cfg, in_channels):
        block_num = len(self.decoder_channels)
        for i, block_channels in enumerate(self.decoder_channels):
            n, paddings = block_num - i, self.decoder_paddings[i]
            setattr(self, f'lateral_layer{n}', SparseBasicBlock(in_channels, block_channels[0], norm_cfg=norm_cfg, indice_key=f'subm{n}',
                                                                compute_dtype=self.compute_dtype))
            setattr(self, f'merge_layer{n}', make_sparse_convmodule(in_channels * 2, block_channels[1], 3, norm_cfg=norm_cfg, padding=paddings[0],
                                                                    indice_key=f'subm{n}', conv_type='SubMConv3d', compute_dtype=self.compute_dtype))
            if n != 1:
                setattr(self, f'upsample_layer{n}', make_sparse_inverse_convmodule(in_channels, block_channels[2], 3, norm_cfg=norm_cfg,
                                                                                   indice_key=f'spconv{n}', compute_dtype=self.compute_dtype))
            else:                                                        # the last block stays on the input rows: a submanifold layer
                setattr(self, f'upsample_layer{n}', make_sparse_convmodule(in_channels, block_channels[2], 3, norm_cfg=norm_cfg, padding=paddings[1],
                                                                           indice_key='subm1', conv_type='SubMConv3d', compute_dtype=self.compute_dtype))
            in_channels = block_channels[2]

    @staticmethod
    def reduce_channel(x, out_channels):
        """x.features (n, C) -> (n, out_channels): the sum over groups of C / out_channels adjacent channels"""
        n, in_channels = x.features.shape
        if in_channels % out_channels != 0 or in_channels < out_channels:
            raise RuntimeError(f'SparseUNet.reduce_channel: {in_channels} channels cannot be reduced to {out_channels}')
        x.features = x.features.view(n, out_channels, -1).sum(dim=2)
        return x

    def decoder_layer_forward(self, x_lateral, x_bottom, lateral_layer, merge_layer, upsample_layer):
        x = lateral_layer(x_lateral)
        x.features = torch.cat((x_bottom.features, x.features), dim=1)
        x_merge = merge_layer(x)
        x = self.reduce_channel(x, x_merge.features.shape[1])
        x.features = x_merge.features + x.features
        return upsample_layer(x)

    def forward(self, voxel_features, coors, batch_size):
        encode_features, spatial_features = self.encode(voxel_features, coors, batch_size)
        x = encode_features[-1]
        for n in range(self.stage_num, 0, -1):
            x = self.decoder_layer_forward(encode_features[n - 1], x, getattr(self, f'lateral_layer{n}'), getattr(self, f'merge_layer{n}'),
                                           getattr(self, f'upsample_layer{n}'))
        return dict(spatial_features=spatial_features, seg_features=x.features)
