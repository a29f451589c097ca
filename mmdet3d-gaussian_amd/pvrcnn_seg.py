"""PV-RCNN's keypoint segmentation slice: `PointwiseMaskHead.loss` (the reference's
mmdet3d_gaussian/models/roi_heads/mask_heads/pointwise_mask_head.py:124-144) and the keypoint reweighting of
`PVRCNNROIHead._bbox_forward` (models/roi_heads/pvrcnn_roi_head.py:211-212).

The reference spends a dozen small torch ops forward and as many backward on 8192 x 1 logits for the loss, and a sigmoid, a max, a
product and their backward nodes for the reweighting.  Here: ONE launch for the loss with its gradient (csrc/seg_head.hip, a single
workgroup) and one streaming launch each for the reweighting's forward and backward; no read-back, so the step
can be captured in a hipGraph.  CUDA tensors go to the kernels on the current stream, CPU tensors to the library's `_cpu` twins
(csrc/seg_head_cpu.cpp).

mmdet's `FocalLoss` is third party, absent here and not pinned by the reference: its math is RESTATED from mmdet 2.x's published
`py_sigmoid_focal_loss` (include/gd3d.h spells it out).  Two properties of the reference are restated, not repaired:
  * with `class_agnostic=True` the positives carry label 1 and K = 1, so the one-hot value of the single column is [label == 0]:
    the column is trained towards 1 on the NON-positive rows;
  * a target above `num_classes` would make `F.one_hot` raise in the reference; here such a row has weight 0 and contributes
    nothing (no check runs on the host: it would need a sync).
"""
import torch

from . import _host
from ._host import cfg_get as _get, f32c, ptr_or_null as _ptr

MAX_K = 255      # seg_head_common.h: the winner column is a byte


def _focal_cfg(loss_seg):
    kind = _get(loss_seg, 'type', type(loss_seg).__name__)
    if kind != 'FocalLoss' or not _get(loss_seg, 'use_sigmoid', True) or _get(loss_seg, 'activated', False):
        raise RuntimeError(f'pvrcnn_seg_loss: loss_seg is {kind!r} (use_sigmoid={_get(loss_seg, "use_sigmoid", True)}, '
                           f'activated={_get(loss_seg, "activated", False)}); the reference head configures FocalLoss(use_sigmoid=True) on logits')
    if _get(loss_seg, 'reduction', 'mean') != 'sum':
        raise RuntimeError("pvrcnn_seg_loss: loss_seg must have reduction 'sum'")
    gamma, alpha = float(_get(loss_seg, 'gamma', 2.0)), float(_get(loss_seg, 'alpha', 0.25))
    if not gamma >= 0 or not 0 <= alpha <= 1:
        raise RuntimeError(f'pvrcnn_seg_loss: loss_seg needs gamma >= 0 and 0 <= alpha <= 1, got gamma={gamma}, alpha={alpha}')
    return gamma, alpha, float(_get(loss_seg, 'loss_weight', 1.0))


def _launch_seg_loss(x, targets, cfg, need_grad):
    """x (N, K) contiguous fp32, targets (N,) contiguous int64 -> (out (2,) = [loss, n_pos], grad (N, K) or None): the one launch"""
    gamma, alpha, weight, num_classes, agnostic = cfg[:5]
    out = torch.empty(2, dtype=torch.float32, device=x.device)
    grad = torch.empty_like(x) if need_grad else None
    _host.call('gd3d_seg_head_loss', x.device,
               (_ptr(x), _ptr(targets), x.size(0), x.size(1), num_classes, int(agnostic), gamma, alpha, weight, out.data_ptr(), _ptr(grad)))
    return out, grad


class _SegLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cfg, targets, seg_preds):
        out, grad = _launch_seg_loss(f32c(seg_preds), targets, cfg, ctx.needs_input_grad[2] and cfg[5])
        ctx.state = (grad, seg_preds.dtype)
        return out[0]

    @staticmethod
    @_host.guard_double_backward
    def backward(ctx, grad_loss):
        grad, dtype = ctx.state
        # `_host.unit_grad`'s constant is known by address: the stored gradient is final, nothing is launched, and the tensor returned
        # IS the node's buffer (as in pvrcnn_train._RoiHeadLoss: do not modify it in place under retain_graph)
        if grad is None:
            return None, None, None
        return None, None, (grad if _host.is_unit_grad(grad_loss) else grad * grad_loss).to(dtype)


def pvrcnn_seg_loss(loss_seg, seg_preds, seg_targets, num_classes, class_agnostic=False):
    """`PointwiseMaskHead.loss` in one launch, gradient included -> {'loss_seg': 0-dim tensor}.

    loss_seg    : the head's module — mmdet FocalLoss(use_sigmoid=True, reduction='sum'), not `activated`, gamma >= 0, 0 <= alpha <= 1 —
                  or its config dict; its loss_weight is honoured.  Anything else raises.
    seg_preds   : (N, K) floating point, K = 1 when class_agnostic else num_classes.
    seg_targets : (N,) integer, `pointwise_mask_targets`' output: -1 ignore, 0..num_classes-1 a class, num_classes background.
    Per row, pos = [0 <= c < num_classes], neg = [c == num_classes], weight (pos + neg) / max(sum pos, 1); the label is pos when
    class_agnostic, else c with the ignored rows at num_classes; loss_seg = loss_weight * sum of weight * sigmoid focal loss.
    Restated from the reference, not repaired: class agnostic, the positives carry label 1 and K = 1, so the single column's one-hot
    value is [label == 0] — it is trained towards 1 on the NON-positive rows; and a target above num_classes (where the reference's
    `F.one_hot` raises) gets weight 0 and contributes nothing — nothing is checked on the host, that would need a sync.
    Differentiable with respect to seg_preds only.  Non-fp32 inputs are evaluated in fp32 and cast back.  The forward launch writes
    the gradient; backward launches nothing when the upstream gradient is `unit_grad`'s constant, else one elementwise scale."""
    gamma, alpha, weight = _focal_cfg(loss_seg)
    num_classes, agnostic = int(num_classes), bool(class_agnostic)
    if num_classes < 1:
        raise RuntimeError(f'pvrcnn_seg_loss: num_classes must be positive, got {num_classes}')
    K = 1 if agnostic else num_classes
    if not isinstance(seg_preds, torch.Tensor) or seg_preds.dim() != 2 or seg_preds.size(1) != K or not seg_preds.dtype.is_floating_point:
        raise RuntimeError(f'shape mismatch: seg_preds must be a floating-point (N, {K}) tensor for class_agnostic={agnostic}, '
                           f'num_classes={num_classes}, got {getattr(seg_preds, "dtype", type(seg_preds))} {tuple(getattr(seg_preds, "shape", ()))}')
    if K > MAX_K:
        raise RuntimeError(f'pvrcnn_seg_loss: at most {MAX_K} columns, got {K}')
    N = seg_preds.size(0)
    if not isinstance(seg_targets, torch.Tensor) or seg_targets.shape != (N,):
        raise RuntimeError(f'shape mismatch: seg_targets must be ({N},), got {tuple(getattr(seg_targets, "shape", ()))}')
    if seg_targets.dtype.is_floating_point or seg_targets.dtype == torch.bool:
        raise RuntimeError(f'seg_targets must be an integer tensor, got {seg_targets.dtype}')
    if seg_targets.device != seg_preds.device:
        raise RuntimeError(f'seg_targets is on {seg_targets.device}, seg_preds on {seg_preds.device}')
    # grad mode is off inside Function.forward: whether a gradient can be asked for at all is read here (forward only: a null gradient pointer)
    loss = _SegLoss.apply((gamma, alpha, weight, num_classes, agnostic, torch.is_grad_enabled()), _host.i64c(seg_targets.detach()), seg_preds)
    return dict(loss_seg=loss if seg_preds.dtype == torch.float32 else loss.to(seg_preds.dtype))


def _launch_reweight(feats, x, need_win):
    """feats (N, C), x (N, K) contiguous fp32, N > 0 -> (out (N, C), win (N,) uint8 or None): the one launch"""
    out = torch.empty_like(feats)
    win = torch.empty((feats.size(0),), dtype=torch.uint8, device=feats.device) if need_win else None
    _host.call('gd3d_keypoint_reweight', feats.device,
               (feats.data_ptr(), x.data_ptr(), feats.size(0), feats.size(1), x.size(1), out.data_ptr(), _host.ptr(win)))
    return out, win


class _Reweight(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feats, seg_preds, track):
        f, x = f32c(feats), f32c(seg_preds)
        need = track and (ctx.needs_input_grad[0] or ctx.needs_input_grad[1])
        out, win = _launch_reweight(f, x, need)    # forward only (inference, no_grad): no winner array
        if need:
            ctx.save_for_backward(f, x, win)
        ctx.dtypes = (feats.dtype, seg_preds.dtype)
        return out if feats.dtype == torch.float32 else out.to(feats.dtype)

    @staticmethod
    @_host.guard_double_backward
    def backward(ctx, grad_out):
        f, x, win = ctx.saved_tensors
        g = f32c(grad_out)
        gf = torch.empty_like(f) if ctx.needs_input_grad[0] else None
        gx = torch.empty_like(x) if ctx.needs_input_grad[1] else None
        _host.call('gd3d_keypoint_reweight_backward', f.device,
                   (g.data_ptr(), f.data_ptr(), x.data_ptr(), win.data_ptr(), f.size(0), f.size(1), x.size(1), _host.ptr(gf), _host.ptr(gx)))
        return (None if gf is None else gf.to(ctx.dtypes[0])), (None if gx is None else gx.to(ctx.dtypes[1])), None


def keypoint_reweight(feats, seg_preds):
    """`keypoints_feats * seg_preds.sigmoid().max(dim=-1, keepdim=True).values` (PVRCNNROIHead._bbox_forward) in one launch, its
    backward in one more: feats (N, C), seg_preds (N, K) floating point, 1 <= K <= 255, C >= 1 -> (N, C), the `features` operand of
    `QueryAndGroup`.  Differentiable with respect to both operands; on equal fp32 sigmoid values the lowest column takes the whole
    gradient (as CPU torch's max(dim) routes it).  Non-fp32 inputs are evaluated in fp32 and cast back.  Without a gradient to
    compute (inference, `torch.no_grad()`) the winner array is not written.  N = 0 returns an empty tensor without a launch."""
    for t, name in ((feats, 'feats'), (seg_preds, 'seg_preds')):
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or not t.dtype.is_floating_point:
            raise RuntimeError(f'shape mismatch: {name} must be a floating-point (N, {"C" if name == "feats" else "K"}) tensor, got '
                               f'{getattr(t, "dtype", type(t))} {tuple(getattr(t, "shape", ()))}')
    if seg_preds.size(0) != feats.size(0):
        raise RuntimeError(f'shape mismatch: {feats.size(0)} rows of feats for {seg_preds.size(0)} rows of seg_preds')
    if seg_preds.device != feats.device:
        raise RuntimeError(f'seg_preds is on {seg_preds.device}, feats on {feats.device}')
    if feats.size(1) < 1 or not 1 <= seg_preds.size(1) <= MAX_K:
        raise RuntimeError(f'keypoint_reweight: needs C >= 1 and 1 <= K <= {MAX_K}, got C={feats.size(1)}, K={seg_preds.size(1)}')
    if feats.size(0) == 0:
        return feats * seg_preds.to(feats.dtype).sum(dim=-1, keepdim=True)     # empty, of feats' shape and dtype, attached to both operands: nothing is launched
    return _Reweight.apply(feats, seg_preds, torch.is_grad_enabled())     # grad mode is off inside Function.forward: read here
