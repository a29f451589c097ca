"""PV-RCNN's RPN proposal stage: `proposal_list = self.rpn_head.get_bboxes(*rpn_outs, img_metas, proposal_cfg)` of the reference's
models/detectors/pv_rcnn.py:115-125 (forward_train) and :143-146 (simple_test), where `rpn_head` is mmdet3d's `PartA2RPNHead`
(configs/kitti/hv_pvrcnn_secfpn_4x4_80e_kitti-3d-3class.py:105-131).

mmdet3d runs one sample at a time: a `topk` over every anchor, a boolean compaction, an NMS with its count read back and a dozen
gathers — B host synchronisations in the middle of a step whose other stages capture.  Here a whole batch is a fill, nine
launches and the batched NMS (csrc/rpn_proposal.hip: a streaming pass makes the order keys, a per-sample radix select finds the
nms_pre best, counting orders them, one launch decodes them, one packs the kept rows) with static shapes and no
read-back, so the call captures in a hipGraph on one stream together with `pvrcnn_assign_and_sample` behind it.  CUDA tensors go
to the kernels on the current stream, CPU tensors to the `_cpu` twin (csrc/rpn_proposal_cpu.cpp), which gives the same bits.

`PartA2RPNHead.get_bboxes_single`, `class_agnostic_nms`, the box coder and `limit_period` are third party, absent here and not
pinned by the reference: they are RESTATED (include/gd3d.h spells the sequence out; INTEGRATION.md §1c lists the deviations).
"""
import torch

from . import _host, _lib
from ._host import cfg_get

MAX_CLASSES, MAX_CANDIDATES, MAX_SAMPLES = 16, 16384, 1024

_workspace_bytes = _host.memo(lambda B, A, C, H, W, nms_pre: int(_lib.load().gd3d_rpn_proposal_workspace_bytes(B, A, C, H, W, nms_pre)))


def _one_level(x, name):
    if isinstance(x, (list, tuple)):
        if len(x) != 1:
            raise RuntimeError(f'rpn_proposals: {name} has {len(x)} levels; the head has one level')
        x = x[0]
    return x


def _head_map(t, name, B, channels, H, W, dev):
    if not isinstance(t, torch.Tensor) or t.dim() != 4:
        raise RuntimeError(f'shape mismatch: {name} must be a (B, channels, H, W) tensor, got {tuple(getattr(t, "shape", ()))}')
    if t.dtype != torch.float32:
        raise RuntimeError(f'{name} must be an fp32 tensor, got {t.dtype}')
    if tuple(t.shape) != (B, channels, H, W):
        raise RuntimeError(f'shape mismatch: {name} must be ({B}, {channels}, {H}, {W}), got {tuple(t.shape)}')
    if t.device != dev:
        raise RuntimeError(f'{name} is on {t.device}, cls_score on {dev}')
    if not t.is_contiguous():
        raise RuntimeError(f'{name} must be contiguous (NCHW): the kernels read the head maps in place')
    return t.detach()


def rpn_proposals(cls_score, bbox_pred, dir_cls_pred, anchors, cfg, num_classes, dir_offset=0.7854, dir_limit_offset=0.0, as_lists=False,
                  input_metas=None, return_candidates=False):
    """`PartA2RPNHead.get_bboxes` for a whole batch, without a host read.

    cls_score (B, A*C, H, W), bbox_pred (B, A*7, H, W), dir_cls_pred (B, A*2, H, W) : the head's maps of its ONE level (or one-element
                  lists of them), fp32, contiguous; the channel of class c of anchor a is a*C + c (likewise a*7 + k, a*2 + d).
    anchors     : (H*W*A, 7) or any shape with that many rows of 7 (the generator's (1, H, W, sizes, rotations, 7)); anchor
                  n = (h*W + w)*A + a.  Non-fp32 anchors are converted.
    cfg         : dict or object with nms_pre (<= 0: every anchor), nms_post, max_num, nms_thr, score_thr, use_rotate_nms.
    num_classes : C (<= 16), sigmoid classification.  At most 16384 candidates min(nms_pre, H*W*A) per sample and 1024 samples.

    Returns a dict of static-shaped tensors, M = min(nms_post, max_num), the samples packed back to back, every element written:
      boxes_3d (B*M, 7), scores_3d (B*M,), labels_3d (B*M,) int64, cls_preds (B*M, C) sigmoid scores, rois (B*M, 8) = [batch id,
      box], batch_cnt (B,) int32 (-1: the NMS scan gave up); rows past the counts' sum hold batch id -1, label -1 and zeros.
      `(boxes_3d, labels_3d, prop_batch_cnt=batch_cnt)` feeds `pvrcnn_assign_and_sample`, `rois` / `cls_preds`
      `multi_class_nms_batch`.  return_candidates=True adds cand_inds (B, cap) int64, the candidates' anchor indices in the selection
      order (-1 past them), and cand_cnt (B,) int32, how many of them passed score_thr.
    as_lists=True reads the counts back ONCE and returns the reference's list of dicts boxes_3d / scores_3d / labels_3d / cls_preds,
      boxes_3d wrapped by `input_metas[i]['box_type_3d']` when metas are given.  The sequence is spelt out in include/gd3d.h."""
    cls_score, bbox_pred, dir_cls_pred = (_one_level(cls_score, 'cls_score'), _one_level(bbox_pred, 'bbox_pred'),
                                          _one_level(dir_cls_pred, 'dir_cls_pred'))
    anchors = _one_level(anchors, 'anchors')
    C = int(num_classes)
    if not 1 <= C <= MAX_CLASSES:
        raise RuntimeError(f'rpn_proposals: num_classes = {num_classes}; 1 to {MAX_CLASSES} are supported')
    if not isinstance(cls_score, torch.Tensor) or cls_score.dim() != 4 or cls_score.size(1) % C != 0 or cls_score.numel() == 0:
        raise RuntimeError(f'shape mismatch: cls_score must be a non-empty (B, A * {C}, H, W) tensor, got '
                           f'{tuple(getattr(cls_score, "shape", ()))}')
    B, AC, H, W = cls_score.shape
    A, dev = AC // C, cls_score.device
    cls_score = _head_map(cls_score, 'cls_score', B, A * C, H, W, dev)
    bbox_pred = _head_map(bbox_pred, 'bbox_pred', B, A * 7, H, W, dev)
    dir_cls_pred = _head_map(dir_cls_pred, 'dir_cls_pred', B, A * 2, H, W, dev)
    N = H * W * A
    if not isinstance(anchors, torch.Tensor) or anchors.dim() < 2 or anchors.size(-1) != 7 or anchors.numel() != N * 7:
        raise RuntimeError(f'shape mismatch: anchors must hold {N} rows of 7, got {tuple(getattr(anchors, "shape", ()))}')
    if anchors.device != dev:
        raise RuntimeError(f'anchors is on {anchors.device}, cls_score on {dev}')
    anchors = _host.f32c(anchors.detach().reshape(N, 7))
    nms_pre, nms_post, max_num = int(cfg_get(cfg, 'nms_pre')), int(cfg_get(cfg, 'nms_post')), int(cfg_get(cfg, 'max_num'))
    nms_thr, score_thr = float(cfg_get(cfg, 'nms_thr')), float(cfg_get(cfg, 'score_thr'))
    rotate = int(bool(cfg_get(cfg, 'use_rotate_nms')))
    if max_num < 1 or nms_post < 1:
        raise RuntimeError(f'rpn_proposals: max_num = {max_num}, nms_post = {nms_post}; both must be at least 1')
    cap = nms_pre if 0 < nms_pre < N else N
    if cap > MAX_CANDIDATES:
        raise RuntimeError(f'rpn_proposals: {cap} candidates per sample (min(nms_pre, H * W * A), nms_pre = {nms_pre}); at most '
                           f'{MAX_CANDIDATES} are supported')
    if B > MAX_SAMPLES or N >= (1 << 30):
        raise RuntimeError(f'rpn_proposals: {B} samples of {N} anchors; at most {MAX_SAMPLES} samples and fewer than 2^30 anchors are supported')
    params = [nms_thr, score_thr, float(dir_offset), float(dir_limit_offset)]
    if any(v != v for v in params):
        raise RuntimeError('rpn_proposals: nms_thr, score_thr, dir_offset and dir_limit_offset must not be NaN')
    M = min(nms_post, max_num)
    f32, i64, i32 = torch.float32, torch.int64, torch.int32
    out = dict(boxes_3d=torch.empty((B * M, 7), dtype=f32, device=dev), scores_3d=torch.empty((B * M,), dtype=f32, device=dev),
               labels_3d=torch.empty((B * M,), dtype=i64, device=dev), cls_preds=torch.empty((B * M, C), dtype=f32, device=dev),
               rois=torch.empty((B * M, 8), dtype=f32, device=dev), batch_cnt=torch.empty((B,), dtype=i32, device=dev))
    if return_candidates:
        out['cand_inds'] = torch.empty((B, cap), dtype=i64, device=dev)
        out['cand_cnt'] = torch.empty((B,), dtype=i32, device=dev)
    ws_bytes = _workspace_bytes(B, A, C, H, W, nms_pre) if dev.type == 'cuda' else 0
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    _host.call('gd3d_rpn_proposals', dev,
               (cls_score.data_ptr(), bbox_pred.data_ptr(), dir_cls_pred.data_ptr(), anchors.data_ptr(), B, A, C, H, W, nms_pre, nms_post,
                max_num, params[0], params[1], rotate, params[2], params[3], out['boxes_3d'].data_ptr(), out['scores_3d'].data_ptr(),
                out['labels_3d'].data_ptr(), out['cls_preds'].data_ptr(), out['rois'].data_ptr(), out['batch_cnt'].data_ptr(),
                _host.ptr(out.get('cand_inds')), _host.ptr(out.get('cand_cnt')), _host.ptr_or_null(ws), ws_bytes))
    if not as_lists:
        return out
    counts = out['batch_cnt'].tolist()          # the one read-back of the list form
    if any(c < 0 for c in counts):
        raise RuntimeError(f'rpn_proposals: the device-side NMS scan gave up (batch_cnt = {counts}); the result is void')
    res, start = [], 0
    for i, c in enumerate(counts):
        boxes = out['boxes_3d'][start:start + c]
        if input_metas is not None:
            boxes = input_metas[i]['box_type_3d'](boxes)
        res.append(dict(boxes_3d=boxes, scores_3d=out['scores_3d'][start:start + c], labels_3d=out['labels_3d'][start:start + c],
                        cls_preds=out['cls_preds'][start:start + c]))
        start += c
    return res


class PartA2RPNHeadProposals(torch.nn.Module):
    """The proposal side of mmdet3d's `PartA2RPNHead`: the attributes `get_bboxes` reads and `get_bboxes` itself over `rpn_proposals`.
    No parameters: the head's convolutions stay where they are."""

    def __init__(self, num_classes, dir_offset=0.7854, dir_limit_offset=0.0):
        super().__init__()
        self.num_classes = num_classes
        self.dir_offset = dir_offset
        self.dir_limit_offset = dir_limit_offset

    def get_bboxes(self, cls_scores, bbox_preds, dir_cls_preds, mlvl_anchors, input_metas, cfg, as_lists=True):
        """The one-element per-level lists the head passes; returns the reference's list of dicts (as_lists=False: the packed dict
        of `rpn_proposals`, no read-back)."""
        return rpn_proposals(cls_scores, bbox_preds, dir_cls_preds, mlvl_anchors, cfg, self.num_classes, dir_offset=self.dir_offset,
                             dir_limit_offset=self.dir_limit_offset, as_lists=as_lists, input_metas=input_metas if as_lists else None)
