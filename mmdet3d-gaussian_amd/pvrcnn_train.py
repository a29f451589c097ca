"""The training slice of `PVRCNNBboxHead`: the reference's mmdet3d_gaussian/models/roi_heads/bbox_heads/pvrcnn_bbox_head.py:213-316
(`get_targets` with `_get_target_single`, the concat=True form) and :140-211 with :318-351 (`loss` with `get_corner_loss_lidar`).

The reference spends a chain of small torch ops per sample on 512 to 2048 rows (649 kernels per step at 4 x 128 RoIs, backward
included) and three host syncs (`reg_mask.bool().any()`, `pos_inds.any()`, boolean indexing).  Here: ONE launch for the targets and ONE for the three losses with their gradients (csrc/roi_head.hip, a single
workgroup each), no read-back, so the whole step can be captured in a hipGraph.  CUDA tensors go to the kernels on
the current stream, CPU tensors to the library's `_cpu` twins (csrc/roi_head_cpu.cpp).

mmdet's `CrossEntropyLoss(use_sigmoid=True)` and `SmoothL1Loss`, and mmdet3d's `DeltaXYZWLHRBBoxCoder`, `rotation_3d_in_axis` and
`LiDARInstance3DBoxes.corners` are third party, absent here and not pinned by the reference: their math is RESTATED from the
published text (include/gd3d.h spells it out).  The rotation's sense changed between mmdet3d 0.x and 1.0 — `clockwise` selects, as
in `pvrcnn_head_get_bboxes` (default: 1.0's counter-clockwise).

Two points where the corner loss is not differentiable are settled by rule: a zero corner distance has a zero gradient (as
torch.norm's backward does), and on an EXACT tie of the distances to the gt and to the flipped gt the unflipped one takes the whole
gradient (torch.min's backward gives each half).
"""
import torch

from . import _host
from ._host import cfg_get as _get, f32c, ptr_or_null as _ptr


def _rows7(t, name, like):
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.size(1) != 7 or not t.dtype.is_floating_point:
        raise RuntimeError(f'shape mismatch: {name} must be a floating-point (rows, 7) tensor, got {getattr(t, "dtype", type(t))} '
                           f'{tuple(getattr(t, "shape", ()))}')
    if like is not None and t.device != like.device:
        raise RuntimeError(f'{name} is on {t.device}, the other operands on {like.device}')
    return f32c(t.detach())


def _vec(t, name, like, rows=None):
    if not isinstance(t, torch.Tensor) or t.dim() != 1 or (rows is not None and t.size(0) != rows):
        raise RuntimeError(f'shape mismatch: {name} must be a ({"R" if rows is None else rows},) tensor, got {tuple(getattr(t, "shape", ()))}')
    if t.device != like.device:
        raise RuntimeError(f'{name} is on {t.device}, the other operands on {like.device}')
    return t.detach()


def pvrcnn_head_get_targets(pos_bboxes, pos_gt_bboxes, ious, cfg, pos_batch_cnt=None, roi_batch_cnt=None, clockwise=False, concat=True):
    """`PVRCNNBboxHead.get_targets(sampling_results, rcnn_train_cfg, concat=True)` in one launch.

    pos_bboxes, pos_gt_bboxes, ious : what the reference collects from the sampling results — three lists of per-sample tensors
                  (P_b, 7), (P_b, 7), (N_b,) (concatenated here, the counts made from the shapes) — or already stacked (P, 7), (P, 7),
                  (R,) tensors with integer count tensors pos_batch_cnt / roi_batch_cnt (B,) on the same device.  The kernel clamps
                  every count to the rows left; device-resident counts are never read back.  The list form costs three
                  concatenations and two small host-to-device copies of the counts per call (no read-back either): for the lowest
                  latency, and for graph capture, keep the batch stacked with the counts on the device.
                  PRECONDITION: a sample must not hold more positives than RoIs, pos_batch_cnt[b] <= roi_batch_cnt[b].  The list form
                  checks that (the reference fails on it later, in `loss`); the stacked form cannot without a sync and does not:
                  such a sample gets more target rows than mask positives, and every later positive then pairs with the wrong
                  target in `pvrcnn_head_loss`.
    cfg         : rcnn train_cfg with `cls_pos_thr` and `cls_neg_thr` (a dict or an object).
    Returns (label (R,) f32, bbox_targets (P, 7) f32, pos_gt_bboxes (P, 7), reg_mask (R,) int64, label_weights (R,) f32,
    bbox_weights (R,) f32) as the reference does.  With stacked inputs whose counts do not cover all rows (padded, fixed shapes
    for a captured graph): the RoI rows past the counts' sum get label 0, mask 0 and zero weights, the target rows past it zeros."""
    if not concat:
        raise RuntimeError('pvrcnn_head_get_targets: only the concat=True form of get_targets is implemented')
    pos_thr, neg_thr = float(_get(cfg, 'cls_pos_thr')), float(_get(cfg, 'cls_neg_thr'))
    if isinstance(ious, (list, tuple)):
        if pos_batch_cnt is not None or roi_batch_cnt is not None:
            raise RuntimeError('pvrcnn_head_get_targets: per-sample lists carry their own counts; pos_batch_cnt / roi_batch_cnt go with stacked tensors')
        if not (isinstance(pos_bboxes, (list, tuple)) and isinstance(pos_gt_bboxes, (list, tuple))) or \
                not len(pos_bboxes) == len(pos_gt_bboxes) == len(ious) or len(ious) == 0:
            raise RuntimeError('shape mismatch: pos_bboxes, pos_gt_bboxes and ious must be lists of the same non-zero length')
        for pb, pg, iu in zip(pos_bboxes, pos_gt_bboxes, ious):
            if not (isinstance(pb, torch.Tensor) and isinstance(pg, torch.Tensor) and isinstance(iu, torch.Tensor)):
                raise RuntimeError(f'shape mismatch: every list element must be a tensor, got {type(pb).__name__}, {type(pg).__name__}, '
                                   f'{type(iu).__name__}')
        dev = ious[0].device
        for pb, pg, iu in zip(pos_bboxes, pos_gt_bboxes, ious):
            if pb.dim() != 2 or pb.shape != pg.shape or iu.dim() != 1 or pb.size(0) > iu.size(0):
                raise RuntimeError(f'shape mismatch: a sample needs pos_bboxes (P_b, 7), pos_gt_bboxes (P_b, 7) and ious (N_b,) with '
                                   f'P_b <= N_b, got {tuple(pb.shape)}, {tuple(pg.shape)}, {tuple(iu.shape)}')
            if pb.device != dev or pg.device != dev or iu.device != dev:
                raise RuntimeError(f'pvrcnn_head_get_targets: the samples are on different devices ({pb.device}, {pg.device}, {iu.device} / {dev})')
        pcnt = torch.tensor([p.size(0) for p in pos_bboxes], dtype=torch.int32).to(dev)    # sizes are host data: no read back
        rcnt = torch.tensor([i.size(0) for i in ious], dtype=torch.int32).to(dev)
        pos_bboxes, pos_gt_bboxes, ious = torch.cat(list(pos_bboxes), 0), torch.cat(list(pos_gt_bboxes), 0), torch.cat(list(ious), 0)
    else:
        if pos_batch_cnt is None or roi_batch_cnt is None:
            raise RuntimeError('pvrcnn_head_get_targets: stacked tensors need pos_batch_cnt and roi_batch_cnt')
        if not isinstance(ious, torch.Tensor) or ious.dim() != 1:
            raise RuntimeError(f'shape mismatch: ious must be (R,), got {tuple(getattr(ious, "shape", ()))}')
        pcnt = _host.counts_i32(pos_batch_cnt, ious, 'pos_batch_cnt')
        rcnt = _host.counts_i32(roi_batch_cnt, ious, 'roi_batch_cnt')
        if pcnt.numel() != rcnt.numel():
            raise RuntimeError(f'shape mismatch: pos_batch_cnt has {pcnt.numel()} samples, roi_batch_cnt {rcnt.numel()}')
    if not ious.dtype.is_floating_point:
        raise RuntimeError(f'ious must be a floating-point tensor, got {ious.dtype}')
    iou32 = f32c(ious.detach())
    pb, pg = _rows7(pos_bboxes, 'pos_bboxes', iou32), _rows7(pos_gt_bboxes, 'pos_gt_bboxes', iou32)
    if pb.size(0) != pg.size(0):
        raise RuntimeError(f'shape mismatch: {pb.size(0)} pos_bboxes for {pg.size(0)} pos_gt_bboxes')
    dev, P, R = iou32.device, pb.size(0), iou32.size(0)
    label = torch.empty((R,), dtype=torch.float32, device=dev)
    targets = torch.empty((P, 7), dtype=torch.float32, device=dev)
    reg_mask = torch.empty((R,), dtype=torch.int64, device=dev)
    label_weights = torch.empty((R,), dtype=torch.float32, device=dev)
    bbox_weights = torch.empty((R,), dtype=torch.float32, device=dev)
    _host.call('gd3d_roi_head_targets', dev,
               (_ptr(pb), _ptr(pg), _ptr(iou32), _ptr(pcnt), _ptr(rcnt), pcnt.numel(), P, R, pos_thr, neg_thr, int(bool(clockwise)),
                _ptr(label), _ptr(targets), _ptr(reg_mask), _ptr(label_weights), _ptr(bbox_weights)))
    if ious.dtype != torch.float32:
        label, label_weights, bbox_weights = label.to(ious.dtype), label_weights.to(ious.dtype), bbox_weights.to(ious.dtype)
    if pos_bboxes.dtype != torch.float32:
        targets = targets.to(pos_bboxes.dtype)
    return label, targets, pos_gt_bboxes, reg_mask, label_weights, bbox_weights


def _bce_cfg(loss_cls):
    kind = _get(loss_cls, 'type', type(loss_cls).__name__)
    if kind != 'CrossEntropyLoss' or not _get(loss_cls, 'use_sigmoid', False) or _get(loss_cls, 'use_mask', False):
        raise RuntimeError(f'pvrcnn_head_loss: loss_cls is {kind!r}; the reference head configures CrossEntropyLoss(use_sigmoid=True)')
    if _get(loss_cls, 'reduction', 'mean') != 'sum' or _get(loss_cls, 'class_weight', None) is not None:
        raise RuntimeError("pvrcnn_head_loss: loss_cls must have reduction 'sum' and no class_weight")
    return float(_get(loss_cls, 'loss_weight', 1.0))


def _smooth_l1_cfg(loss_bbox):
    kind = _get(loss_bbox, 'type', type(loss_bbox).__name__)
    if kind != 'SmoothL1Loss':
        raise RuntimeError(f'pvrcnn_head_loss: loss_bbox is {kind!r}; the reference head configures SmoothL1Loss')
    if _get(loss_bbox, 'reduction', 'mean') != 'sum':
        raise RuntimeError("pvrcnn_head_loss: loss_bbox must have reduction 'sum'")
    beta = float(_get(loss_bbox, 'beta', 1.0))
    if not beta > 0:
        raise RuntimeError(f'pvrcnn_head_loss: SmoothL1Loss beta must be positive, got {beta}')
    return beta, float(_get(loss_bbox, 'loss_weight', 1.0))


class _RoiHeadLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cfg, data, cls_score, bbox_pred):
        beta, w_cls, w_bbox, corner, clockwise = cfg
        rois, labels, targets, gts, reg_mask, label_weights, bbox_weights = data
        x, p = f32c(cls_score).reshape(-1), f32c(bbox_pred)
        dev, R, P = x.device, x.size(0), targets.size(0)
        need_c, need_b = ctx.needs_input_grad[2], ctx.needs_input_grad[3]
        gc = torch.empty_like(x) if need_c else None
        # rows: d(loss_bbox + loss_corner), d loss_bbox, d loss_corner — the sum is what a unit upstream gradient returns as it is
        gb = torch.empty((3 if corner else 1, R, 7), dtype=torch.float32, device=dev) if need_b else None
        out = torch.empty(3, dtype=torch.float32, device=dev)
        _host.call('gd3d_roi_head_loss', dev,
                   (_ptr(x), _ptr(p), _ptr(rois), rois.size(1), rois.size(1) - 7, _ptr(labels), _ptr(targets), _ptr(gts), _ptr(reg_mask),
                    _ptr(label_weights), _ptr(bbox_weights), R, P, beta, w_cls, w_bbox, int(corner), int(clockwise), out.data_ptr(),
                    _ptr(gc), None if gb is None else gb[0].data_ptr(), None if gb is None or not corner else gb[1].data_ptr(),
                    None if gb is None or not corner else gb[2].data_ptr()))
        ctx.state = (gc, gb, corner, cls_score.shape, cls_score.dtype, bbox_pred.dtype)
        return out[0], out[1], out[2]

    @staticmethod
    @_host.guard_double_backward
    def backward(ctx, grad_cls, grad_bbox, grad_corner):
        gc, gb, corner, shape, dtc, dtb = ctx.state
        # the library's own constant 1.0 (_host.unit_grad) is known by address: the stored gradients are final, nothing is launched.
        # The tensors returned then ARE the node's stored buffers (as in anchor_cls._ClsDir), which ctx.state keeps alive for a second
        # backward under retain_graph: a caller that takes them from autograd.grad(..., retain_graph=True) must not modify them in place.
        rc = None if gc is None else (gc if _host.is_unit_grad(grad_cls) else gc * grad_cls).reshape(shape).to(dtc)
        if gb is None:
            rb = None
        elif not corner:
            rb = gb[0] if _host.is_unit_grad(grad_bbox) else gb[0] * grad_bbox
        elif _host.is_unit_grad(grad_bbox) and _host.is_unit_grad(grad_corner):
            rb = gb[0]
        else:
            rb = torch.addcmul(gb[1] * grad_bbox, gb[2], grad_corner)
        return None, None, rc, None if rb is None else rb.to(dtb)


def pvrcnn_head_loss(loss_cls, loss_bbox, cls_score, bbox_pred, rois, labels, bbox_targets, pos_gt_bboxes, reg_mask, label_weights,
                     bbox_weights, with_corner_loss=True, clockwise=False):
    """`PVRCNNBboxHead.loss` in one launch, gradients included.

    loss_cls / loss_bbox : the head's modules — mmdet CrossEntropyLoss(use_sigmoid=True, reduction='sum') without class_weight and
                  SmoothL1Loss(beta, reduction='sum') — or their config dicts; each contributes its loss_weight.  Anything else raises.
    cls_score   : (R, 1) or (R,);  bbox_pred (R, 7);  rois (R, 8) [batch id, x, y, z, dx, dy, dz, yaw] as the reference passes them;
    labels, label_weights, bbox_weights (R,), reg_mask (R,) integer, bbox_targets / pos_gt_bboxes (P, 7): `pvrcnn_head_get_targets`'
                  outputs.  The j-th row with reg_mask > 0, in row order, pairs with row j of bbox_targets / pos_gt_bboxes (found by a
                  scan inside the kernel: no nonzero(), no sync); positive rows past the P-th are ignored, and the corner loss's mean
                  runs over the paired rows (P of them whenever reg_mask and bbox_targets belong together, as in the reference).
    Returns {'loss_cls', 'loss_bbox'[, 'loss_corner']}: 0-dim tensors, differentiable with respect to cls_score and bbox_pred only
    (RoIs and targets are data).  Without a positive row loss_bbox and loss_corner are 0 and bbox_pred's gradient is all zeros.
    loss_corner is not weighted by bbox_weights (nor is it in the reference).  Non-fp32 inputs are evaluated in fp32 and cast back.
    The forward launch writes the gradients; backward launches nothing when the upstream gradients are `unit_grad`'s constant."""
    w_cls = _bce_cfg(loss_cls)
    beta, w_bbox = _smooth_l1_cfg(loss_bbox)
    if not isinstance(bbox_pred, torch.Tensor) or bbox_pred.dim() != 2 or bbox_pred.size(1) != 7 or not bbox_pred.dtype.is_floating_point:
        raise RuntimeError(f'shape mismatch: bbox_pred must be a floating-point (R, 7) tensor, got {tuple(getattr(bbox_pred, "shape", ()))}')
    R = bbox_pred.size(0)
    if not isinstance(cls_score, torch.Tensor) or cls_score.shape not in ((R,), (R, 1)) or not cls_score.dtype.is_floating_point:
        raise RuntimeError(f'shape mismatch: cls_score must be a floating-point ({R}, 1) or ({R},) tensor, got {tuple(getattr(cls_score, "shape", ()))}')
    if cls_score.device != bbox_pred.device:
        raise RuntimeError(f'cls_score is on {cls_score.device}, bbox_pred on {bbox_pred.device}')
    if not isinstance(rois, torch.Tensor) or rois.shape != (R, 8) or not rois.dtype.is_floating_point:
        raise RuntimeError(f'shape mismatch: rois must be a floating-point ({R}, 8) tensor, got {tuple(getattr(rois, "shape", ()))}')
    if rois.device != bbox_pred.device:
        raise RuntimeError(f'rois is on {rois.device}, bbox_pred on {bbox_pred.device}')
    targets, gts = _rows7(bbox_targets, 'bbox_targets', bbox_pred), _rows7(pos_gt_bboxes, 'pos_gt_bboxes', bbox_pred)
    if targets.size(0) != gts.size(0):
        raise RuntimeError(f'shape mismatch: {targets.size(0)} bbox_targets for {gts.size(0)} pos_gt_bboxes')
    mask = _vec(reg_mask, 'reg_mask', bbox_pred, R)
    if mask.dtype.is_floating_point:
        raise RuntimeError(f'reg_mask must be an integer or bool tensor, got {mask.dtype}')
    data = (f32c(rois.detach()), f32c(_vec(labels, 'labels', bbox_pred, R)), targets, gts, _host.i64c(mask),
            f32c(_vec(label_weights, 'label_weights', bbox_pred, R)), f32c(_vec(bbox_weights, 'bbox_weights', bbox_pred, R)))
    corner = bool(with_corner_loss)
    l_cls, l_bbox, l_corner = _RoiHeadLoss.apply((beta, w_cls, w_bbox, corner, bool(clockwise)), data, cls_score, bbox_pred)
    if cls_score.dtype != torch.float32:
        l_cls, l_bbox, l_corner = l_cls.to(cls_score.dtype), l_bbox.to(cls_score.dtype), l_corner.to(cls_score.dtype)
    losses = dict(loss_cls=l_cls, loss_bbox=l_bbox)
    if corner:
        losses['loss_corner'] = l_corner
    return losses
