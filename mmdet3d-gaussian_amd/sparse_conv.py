"""Sparse 3D convolution: spconv 1.x's `SubMConv3d` / `SparseConv3d` / `SparseInverseConv3d` as mmdet3d re-exports them
(`mmdet3d.ops.spconv`), on the tensor and containers of sparse_tensor.py; the blocks, builders and encoders made of them are in
sparse_encoder.py.  mmdet3d and spconv are CUDA-only and absent from the reference tree: the op is RESTATED
(include/gd3d.h) — a sparse convolution equals the dense `conv3d` of the densified input read at the active output sites.

Two calls carry it (csrc/sparse_conv.hip, csrc/sparse_conv_wgrad.hip): `sparse_conv_index` builds the neighbour tables of one layer geometry in one stream-ordered
run of launches (64-bit keys, a stable radix sort, look-ups by lower bound; the outputs of a strided layer in ascending (b, z, y, x)
order, as spconv 1.x's GPU path gives them), `sparse_conv` evaluates a layer over a table (one launch forward; one for the input
gradient; three for the weight and bias gradients; no atomics, the bits replay).  CUDA
tensors go to the kernels on the current stream, CPU tensors to the library's `_cpu` twins.  By default fp32: another dtype is evaluated
in fp32 and cast back.  `compute_dtype=torch.float16 / torch.bfloat16 / 'auto'` (a keyword of `sparse_conv`, of every layer and of every
builder of sparse_encoder.py) selects the mixed-precision form (csrc/sparse_conv_16.hip): 16-bit operands on the matrix cores, fp32
accumulation, a 16-bit output, fp32 weight and bias gradients.  `scale=, shift=, residual=, activation=` on `sparse_conv`, and
`FusedSparseConv` as the module, put an eval BatchNorm, a block's residual add and the ReLU into the
forward launch.  `weight_grad='mfma'` (same places; opt-in) takes the 16-bit weight gradient's partial sums on the matrix
cores too (csrc/sparse_conv_wgrad_16.hip).  Dilation must be 1.

The way back up: `sparse_conv_index` keeps the rows it was built over (`in_coors`, `in_shape`), and
`sparse_conv_index_inverse` hands the same tables back with the roles swapped, so `sparse_inverse_conv` / `SparseInverseConv3d` (spconv 1.x's
inverse convolution) are the launches above over `nbr_t` — no new kernel, every form included.  Max pooling over the same tables lives
in sparse_pool.py, live-row batch normalisation in sparse_bn.py.
"""
import ctypes
import math
from typing import NamedTuple, Optional

import torch
from torch import nn

from . import _host, _lib
from .sparse_tensor import (ACT_CODES, DTYPE_CODES, MAX_CHANNELS, MAX_OFFSETS, SparseConvTensor, SparseModule, as_dtype, check_activation, coors_i32,
                            triple)
from .sparse_tensor import SparseSequential, ToDense, sparse_to_dense  # noqa: F401  (the tensor layer stays visible from this module)


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


def _geometry(spatial_shape, kernel_size, stride, padding, subm, who):
    """(shape, kernel, stride, padding, out_shape) as int triples, validated as the C entry point validates them"""
    n, k, s, p = triple(spatial_shape, 'spatial_shape'), triple(kernel_size, 'kernel_size'), triple(stride, 'stride'), triple(padding, 'padding')
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


def sparse_conv_index(coors, spatial_shape, batch_size, kernel_size, stride=1, padding=0, subm=False, max_out=None, dilation=1):
    """The neighbour tables of one layer -> `SparseConvIndex(out_coors, out_shape, nbr, nbr_t, num, out_batch_cnt)`.

    coors (N, 4) integer rows [b, z, y, x]; a row with a negative entry, b >= batch_size or a coordinate outside `spatial_shape` is
    inactive (the tail rows of `hard_voxelize(static=True)`): no output, nobody's neighbour.  Active rows must be unique.
    subm=True  : odd kernel, stride 1, padding k // 2 (anything else raises); the outputs are the inputs, R = N, no read-back.
    subm=False : out_shape = (n + 2p - k) // s + 1 (0 on an axis the kernel does not fit: no output); the active outputs in ascending (b, z, y, x) order.  max_out=None reads the count
                 back ONCE and returns exact-size views; an int gives the static, capturable form: R = max_out rows, the lowest keys
                 kept, the rows past num[0] holding -1, and nothing read back.
    Every output is an integer and replays bit for bit on the device, in the `_cpu` twin and in the numpy restatement of the tests."""
    if triple(dilation, 'dilation') != (1, 1, 1):
        raise RuntimeError(f'sparse_conv_index: dilation must be 1, got {dilation}')
    subm = bool(subm)
    n, k, s, p, o = _geometry(spatial_shape, kernel_size, stride, padding, subm, 'sparse_conv_index')
    c = coors_i32(coors, 'sparse_conv_index')
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


def check_weight_grad(weight_grad, who):
    if weight_grad is not None and not (isinstance(weight_grad, str) and weight_grad == 'mfma'):
        raise RuntimeError(f"{who}: weight_grad must be None or 'mfma', got {weight_grad!r}")
    return weight_grad


def _weight_entry(dtype, dev, weight_grad):
    """the weight-gradient entry of a compute dtype (None: fp32) on a device: the matrix-core form only for 'mfma' on 16-bit operands on the
    device"""
    if dtype is None:
        return 'gd3d_sparse_conv_backward_weight'
    return 'gd3d_sparse_conv_backward_weight_16' + ('_mfma' if weight_grad == 'mfma' and dev.type == 'cuda' else '')


def _backward_entries(x, w, gy, nbr, nbr_t, num, subm, need_x, need_w, has_bias, dtype, weight_grad=None):
    """the backward entries on contiguous operands of the kernels' types (dtype None: fp32) -> (gx, gw, gb) as the kernels wrote them,
    None where not asked for.  weight_grad: None or 'mfma' (`sparse_conv`)"""
    N, (K, Cin, Cout), R, dev = x.size(0), w.shape, nbr.size(0), x.device
    suffix, code = ('', ()) if dtype is None else ('_16', (DTYPE_CODES[dtype],))
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
        _host.call(_weight_entry(dtype, dev, weight_grad), dev,
                   (ptr(x), ptr(gy), ptr(nbr), ptr(num), N, R, K, Cin, Cout, *code, ptr(work), ptr(gw), ptr(gb)))
    return gx, gw, gb


def _autocast_dtype(device_type):
    """the autocast dtype of `device_type` where autocast is enabled for it, else None"""
    if device_type not in ('cuda', 'cpu'):
        return None
    return torch.get_autocast_dtype(device_type) if torch.is_autocast_enabled(device_type) else None


def check_compute_dtype(compute_dtype, who):
    if compute_dtype is not None and not (isinstance(compute_dtype, str) and compute_dtype == 'auto') and compute_dtype not in DTYPE_CODES:
        raise RuntimeError(f"{who}: compute_dtype must be None, torch.float16, torch.bfloat16 or 'auto', got {compute_dtype!r}")
    return compute_dtype


def _resolve_compute_dtype(compute_dtype, features):
    """None (the fp32 path), torch.float16 or torch.bfloat16.  'auto': the features' dtype if it is one of the two, else the autocast
    dtype where autocast is enabled for the features' device, else None"""
    if check_compute_dtype(compute_dtype, 'sparse_conv') is None or compute_dtype in DTYPE_CODES:
        return compute_dtype
    if features.dtype in DTYPE_CODES:
        return features.dtype
    dtype = _autocast_dtype(features.device.type)
    return dtype if dtype in DTYPE_CODES else None


class _SparseConv(torch.autograd.Function):
    """One layer over its tables, every form.  dtype None: fp32 operands; torch.float16 / torch.bfloat16: 16-bit features, weight, residual,
    grad_out and output, fp32 bias, scale, shift and parameter gradients.  residual, scale, shift, activation all None: the plain entry
    (gd3d_sparse_conv_forward[_16]); any of them given: conv -> * scale + shift -> + residual -> ReLU in ONE forward launch
    (gd3d_sparse_conv_forward_fused[_16]).  Differentiable w.r.t. features, weight, bias and residual; scale and shift are
    constants (a frozen BatchNorm).  The backward is the same entries in every form (`_backward_entries`)."""

    @staticmethod
    def forward(ctx, features, weight, bias, residual, scale, shift, nbr, nbr_t, num, subm, activation, dtype, weight_grad=None):
        if dtype is None:
            x, w, code = _host.f32c(features), _host.f32c(weight), ()
        else:
            x, w, code = as_dtype(features, dtype), as_dtype(weight, dtype), (DTYPE_CODES[dtype],)
        b = None if bias is None else _host.f32c(bias)
        N, (K, Cin, Cout), R, dev = x.size(0), w.shape, nbr.size(0), x.device
        out = torch.empty((R, Cout), dtype=dtype or torch.float32, device=dev)
        ptr = _host.ptr_or_null
        if residual is None and scale is None and shift is None and activation is None:
            sc = None
            _host.call('gd3d_sparse_conv_forward' if dtype is None else 'gd3d_sparse_conv_forward_16', dev,
                       (ptr(x), ptr(w), ptr(b), ptr(nbr), ptr(num), N, R, K, Cin, Cout, *code, ptr(out)))
        else:
            res = None if residual is None else (_host.f32c(residual) if dtype is None else as_dtype(residual, dtype))
            sc = None if scale is None else _host.f32c(scale)
            sh = None if shift is None else _host.f32c(shift)
            if b is not None:                                                          # the conv's own bias, folded on the host: shift' = bias * scale + shift
                b = b if sc is None else b * sc
                sh = b if sh is None else b + sh
            _host.call('gd3d_sparse_conv_forward_fused' if dtype is None else 'gd3d_sparse_conv_forward_fused_16', dev,
                       (ptr(x), ptr(w), ptr(sc), ptr(sh), ptr(res), ptr(nbr), ptr(num), N, R, K, Cin, Cout, ACT_CODES[activation], *code, ptr(out)))
        ctx.save_for_backward(x, w, nbr, nbr_t, num, sc, out if activation == 'relu' else None)
        ctx.state = (subm, bias is not None, features.dtype, weight.dtype, None if bias is None else bias.dtype,
                     None if residual is None else residual.dtype, weight.shape, dtype, weight_grad)
        return out if dtype is not None or features.dtype == torch.float32 else out.to(features.dtype)

    @staticmethod
    @_host.guard_double_backward
    def backward(ctx, grad_out):
        x, w, nbr, nbr_t, num, sc, out = ctx.saved_tensors
        subm, has_bias, x_dtype, w_dtype, b_dtype, r_dtype, w_shape, dtype, weight_grad = ctx.state
        g = grad_out if dtype is not None else _host.f32c(grad_out)
        if out is not None:
            g = g * (out > 0)                                                          # the ReLU's gradient, exact
        gres = g.to(r_dtype) if r_dtype is not None and ctx.needs_input_grad[3] else None
        gy = g if sc is None else g.float() * sc                                       # what reaches the convolution: the existing backward entries run on it
        gy = _host.f32c(gy) if dtype is None else as_dtype(gy, dtype)
        gx, gw, gb = _backward_entries(x, w, gy, nbr, nbr_t, num, subm, ctx.needs_input_grad[0],
                                       ctx.needs_input_grad[1] or (has_bias and ctx.needs_input_grad[2]), has_bias, dtype, weight_grad)
        gx = None if gx is None else gx.to(x_dtype)
        gw = None if gw is None else gw.to(w_dtype).reshape(w_shape)
        gb = None if gb is None else gb.to(b_dtype)
        return gx, gw, gb, gres, None, None, None, None, None, None, None, None, None


def _check_fused_operands(scale, shift, residual, activation, features, Cout, R):
    check_activation(activation, 'sparse_conv')
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


def sparse_conv(features, weight, bias, index, compute_dtype=None, *, scale=None, shift=None, residual=None, activation=None, weight_grad=None):
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
    ReLU, grad_residual = g, and the backward launches above run on g * scale.  With all four None the call is the one it always was.

    weight_grad (keyword-only): None — the weight and bias gradients as they always were, entry for entry.  'mfma': on the
    device, where the resolved compute dtype is torch.float16 / torch.bfloat16, the backward takes the per-chunk partial sums of the weight
    gradient on the matrix cores (gd3d_sparse_conv_backward_weight_16_mfma): the same chunks, workspace, fp32 outputs and bias gradient,
    another order of addition inside a chunk, the same bits from run to run.  It is inert where the resolved compute dtype is None (fp32),
    and inert on CPU tensors, where the `_cpu` twin of the default entry runs: a network can carry the switch through 'auto' and through
    CPU runs.  Anything else raises."""
    check_weight_grad(weight_grad, 'sparse_conv')
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
    return _SparseConv.apply(features, w, bias, residual, scale, shift, index.nbr, index.nbr_t, index.num, index.subm, activation, dtype,
                             weight_grad)


def sparse_inverse_conv(features, weight, bias, index, compute_dtype=None, *, scale=None, shift=None, residual=None, activation=None,
                        weight_grad=None):
    """spconv 1.x's inverse convolution over the tables of the FORWARD layer's `index` (a strided `sparse_conv_index`) -> (N, Cout):
    `sparse_conv` over `sparse_conv_index_inverse(index)` — the same launches, forward and backward, the 16-bit and the fused forms included.

    out[i] = sum over the offsets j with index.nbr_t[i, j] >= 0 of features[nbr_t[i, j]] @ weight[j] (+ bias), features (R, Cin) on the
    forward layer's output rows, out on its input rows; weight (kz, ky, kx, Cin, Cout) or (K, Cin, Cout), the offset j numbered as in the
    forward layer.  It equals the dense `conv_transpose3d` of the densified features read at the forward layer's input sites.
    The rule for a row without a valid neighbour holds: that row is ZERO, bias or not — an inactive input row, an active input that no
    output cell reaches (a stride above the kernel, a truncated edge), an input whose outputs were all dropped by `max_out`.  spconv writes
    the bias to such a row; mmdet3d builds these layers without bias, where the two agree.  weight_grad: as in `sparse_conv`."""
    return sparse_conv(features, weight, bias, sparse_conv_index_inverse(index), compute_dtype, scale=scale, shift=shift, residual=residual,
                       activation=activation, weight_grad=weight_grad)


class SparseConvolution(SparseModule):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, bias=True, subm=False, indice_key=None,
                 max_out=None, *, compute_dtype=None, weight_grad=None):
        super().__init__()
        self.compute_dtype = check_compute_dtype(compute_dtype, type(self).__name__)     # None, torch.float16, torch.bfloat16 or 'auto': `sparse_conv`
        self.weight_grad = check_weight_grad(weight_grad, type(self).__name__)           # None or 'mfma': `sparse_conv`; an attribute, not a buffer
        if triple(dilation, 'dilation') != (1, 1, 1):
            raise RuntimeError(f'{type(self).__name__}: dilation must be 1, got {dilation}')
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.kernel_size = triple(kernel_size, 'kernel_size')
        self.subm = bool(subm)
        # a submanifold layer pads by k // 2 whatever it is handed, as spconv does
        self.stride = (1, 1, 1) if self.subm else triple(stride, 'stride')
        self.padding = tuple(k // 2 for k in self.kernel_size) if self.subm else triple(padding, 'padding')
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
        SparseConvTensor.expect(x, type(self).__name__)
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
        return x.derive(features, None if self.subm else index.out_coors, index.out_shape)

    def forward(self, x):
        index = self.index_of(x)
        return self.output_of(x, index, sparse_conv(x.features, self.weight, self.bias, index, self.compute_dtype, weight_grad=self.weight_grad))

    def extra_repr(self):
        return (f'{self.in_channels}, {self.out_channels}, kernel_size={self.kernel_size}, stride={self.stride}, padding={self.padding}, '
                f'bias={self.bias is not None}, indice_key={self.indice_key!r}'
                + ('' if self.compute_dtype is None else f', compute_dtype={self.compute_dtype!r}')
                + ('' if self.weight_grad is None else f', weight_grad={self.weight_grad!r}'))


class SubMConv3d(SparseConvolution):
    """spconv 1.x's submanifold convolution: the outputs are the inputs.  `stride` and `padding` are accepted and not used (k // 2)."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, bias=True, indice_key=None, *, compute_dtype=None,
                 weight_grad=None):
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, bias, True, indice_key, compute_dtype=compute_dtype,
                         weight_grad=weight_grad)


class SparseConv3d(SparseConvolution):
    """spconv 1.x's regular sparse convolution.  max_out (an addition): an int gives the static form of `sparse_conv_index`."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, bias=True, indice_key=None, max_out=None, *,
                 compute_dtype=None, weight_grad=None):
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, bias, False, indice_key, max_out,
                         compute_dtype=compute_dtype, weight_grad=weight_grad)


class SparseInverseConv3d(SparseConvolution):
    """spconv 1.x's inverse convolution (its positional signature): undoes the geometry of the `SparseConv3d` that stored its index under
    `indice_key` — the output lies on that layer's INPUT rows (`indices`, `spatial_shape`), through the same tables with the roles swapped
    (`sparse_inverse_conv`).  Builds nothing and leaves `indice_dict` as it was; a missing key raises.  A row without a valid neighbour is
    zero, bias or not (spconv writes the bias there)."""

    def __init__(self, in_channels, out_channels, kernel_size, indice_key, bias=True, *, compute_dtype=None, weight_grad=None):
        super().__init__(in_channels, out_channels, kernel_size, 1, 0, 1, bias, False, indice_key, compute_dtype=compute_dtype,
                         weight_grad=weight_grad)

    def build_index(self, x):
        raise RuntimeError(f'{type(self).__name__} builds no index: it needs the one a SparseConv3d stored under indice_key {self.indice_key!r}')

    def index_of(self, x):
        """the inverse view of the index stored under `indice_key` (`sparse_conv_index_inverse`); x must lie on that layer's output rows"""
        SparseConvTensor.expect(x, type(self).__name__)
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
                f'indice_key={self.indice_key!r}' + ('' if self.compute_dtype is None else f', compute_dtype={self.compute_dtype!r}')
                + ('' if self.weight_grad is None else f', weight_grad={self.weight_grad!r}'))


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
    `compute_dtype` and `weight_grad` are shared, not copied.  scale, shift: fp32 buffers (None without a BatchNorm).  forward(x, residual=None)."""

    def __init__(self, conv, norm=None, activation=None):
        super().__init__()
        if not isinstance(conv, SparseConvolution):
            raise RuntimeError(f'FusedSparseConv: conv must be a SubMConv3d or a SparseConv3d, got {type(conv).__name__}')
        check_activation(activation, 'FusedSparseConv')
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
    weight_grad = property(lambda self: self.conv.weight_grad)

    def forward(self, x, residual=None):
        conv = self.conv
        index = conv.index_of(x)
        return conv.output_of(x, index, sparse_conv(x.features, conv.weight, conv.bias, index, conv.compute_dtype, scale=self.scale, shift=self.shift,
                                                    residual=residual, activation=self.activation, weight_grad=conv.weight_grad))

    def extra_repr(self):
        return (f'norm={self.scale is not None}, activation={self.activation!r}, indice_key={self.indice_key!r}, max_out={self.max_out!r}'
                + ('' if self.compute_dtype is None else f', compute_dtype={self.compute_dtype!r}')
                + ('' if self.weight_grad is None else f', weight_grad={self.weight_grad!r}'))
