"""The assign-and-sample stage of PV-RCNN's RoI head: the reference's mmdet3d_gaussian/models/roi_heads/pvrcnn_roi_head.py:225-297
(`PVRCNNROIHead._assign_and_sample`), and the pairwise 3D IoU its assigner is configured with.

The reference runs, per sample, a Python loop over the classes with a `MaxIoUAssigner` on a `BboxOverlaps3D` matrix, `nonzero` /
`F.pad` / boolean assignment, and the `IoUNegPiecewiseSampler`'s `nonzero` / `randperm` / `randint` / `unique` chain: hundreds of
small launches and a dozen host read-backs on 512 proposals x a few dozen gts.  Here the whole batch is two launches
(csrc/roi_sample.hip: one workgroup per sample, then one workgroup that packs the samples) without a read-back,
so proposals -> sampled RoIs -> `roi_grid_queries` -> `QueryAndGroup` -> head -> `pvrcnn_head_get_targets` -> `pvrcnn_head_loss`
captures in one hipGraph.  CUDA tensors go to the kernels on the current stream, CPU tensors to the `_cpu` twins
(csrc/roi_sample_cpu.cpp), which give the same bits.

mmdet's `MaxIoUAssigner`, mmdet3d's `IoUNegPiecewiseSampler`, `BboxOverlaps3D` and `LiDARInstance3DBoxes.overlaps` are third party,
absent here and not pinned by the reference: they are RESTATED (include/gd3d.h spells the rules out).  All randomness comes from
two tensors of uniform keys, so a call with keys given is a pure function of its inputs.
"""
import ctypes

import torch

from . import _host
from ._host import cfg_get as _get, f32c, i64c, ptr_or_null as _ptr

MAX_PROPOSALS, MAX_GTS, MAX_NUM, MAX_PIECES, MAX_CLASSES = 4096, 1024, 1024, 8, 16


def _boxes7(t, name):
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.size(1) != 7 or not t.dtype.is_floating_point:
        raise RuntimeError(f'shape mismatch: {name} must be a floating-point (rows, 7) tensor, got {getattr(t, "dtype", type(t))} '
                           f'{tuple(getattr(t, "shape", ()))}')
    return f32c(t.detach())


def bbox_overlaps_3d(bboxes1, bboxes2):
    """`BboxOverlaps3D(coordinate='lidar')(bboxes1, bboxes2)`: the (N, M) fp32 matrix of 3D IoUs of rows [x, y, z, dx, dy, dz, yaw],
    z the bottom face — mmdet3d's: the BEV overlap of the iou3d family (`xywhr2xyxyr` + `boxes_iou_bev`'s pair test, the NMS path)
    times the height overlap, over the union of the volumes, floored at 1e-8.  One fp32 operation sequence for the kernel, for
    `pvrcnn_assign_and_sample` and for the CPU twin: the same bits from all three.  Non-fp32 inputs are evaluated in fp32; an
    empty operand gives an empty result.  (`iou_3d` is another arithmetic: the evaluation op's.)"""
    a, b = _boxes7(bboxes1, 'bboxes1'), _boxes7(bboxes2, 'bboxes2')
    if a.device != b.device:
        raise RuntimeError(f'bboxes1 is on {a.device}, bboxes2 on {b.device}')
    n, m = a.size(0), b.size(0)
    if n * m >= (1 << 31) - 256:
        raise RuntimeError(f'bbox_overlaps_3d: {n} x {m} pairs; the kernel takes fewer than 2^31')
    out = torch.empty((n, m), dtype=torch.float32, device=a.device)
    if n and m:
        _host.call('gd3d_roi_iou3d', a.device, (a.data_ptr(), n, b.data_ptr(), m, out.data_ptr()))
    return out


def _assigner_rules(assigner):
    cfgs = list(assigner) if isinstance(assigner, (list, tuple)) else [assigner]
    if not 1 <= len(cfgs) <= MAX_CLASSES:
        raise RuntimeError(f'pvrcnn_assign_and_sample: {len(cfgs)} assigners; 1 to {MAX_CLASSES} are supported')
    pos, neg, low, flags = [], [], [], []
    for c in cfgs:
        kind = _get(c, 'type', 'MaxIoUAssigner')
        if kind != 'MaxIoUAssigner':
            raise RuntimeError(f'pvrcnn_assign_and_sample: assigner is {kind!r}; the reference configures MaxIoUAssigner')
        calc = _get(c, 'iou_calculator', None)
        if calc is not None:
            ckind = _get(calc, 'type', type(calc).__name__)
            if ckind != 'BboxOverlaps3D' or _get(calc, 'coordinate', 'lidar') != 'lidar':
                raise RuntimeError(f"pvrcnn_assign_and_sample: iou_calculator must be BboxOverlaps3D(coordinate='lidar'), got {ckind!r}")
        ign = _get(c, 'ignore_iof_thr', -1)
        if ign is not None and not ign < 0:
            raise RuntimeError(f'pvrcnn_assign_and_sample: ignore_iof_thr = {ign}; ignore regions are not implemented')
        n = _get(c, 'neg_iou_thr')
        if isinstance(n, (list, tuple)):
            raise RuntimeError('pvrcnn_assign_and_sample: neg_iou_thr must be a float (the interval form is not implemented)')
        p = float(_get(c, 'pos_iou_thr'))
        pos.append(p)
        neg.append(float(n))
        low.append(float(_get(c, 'min_pos_iou', 0.0)))
        flags.append((1 if _get(c, 'match_low_quality', True) else 0) | (2 if _get(c, 'gt_max_assign_all', True) else 0))
    return tuple(pos), tuple(neg), tuple(low), tuple(flags)


def _sampler_rules(sampler):
    kind = _get(sampler, 'type', type(sampler).__name__)
    if kind != 'IoUNegPiecewiseSampler':
        raise RuntimeError(f'pvrcnn_assign_and_sample: sampler is {kind!r}; the reference configures IoUNegPiecewiseSampler')
    if _get(sampler, 'neg_pos_ub', -1) != -1 or _get(sampler, 'add_gt_as_proposals', False):
        raise RuntimeError('pvrcnn_assign_and_sample: neg_pos_ub must be -1 and add_gt_as_proposals False')
    num, frac = int(_get(sampler, 'num')), float(_get(sampler, 'pos_fraction'))
    if not 1 <= num <= MAX_NUM or not 0.0 <= frac <= 1.0:
        raise RuntimeError(f'pvrcnn_assign_and_sample: sampler.num must be 1..{MAX_NUM} and pos_fraction in [0, 1], got {num}, {frac}')
    fracs = tuple(float(f) for f in _get(sampler, 'neg_piece_fractions'))
    thrs = tuple(float(t) for t in _get(sampler, 'neg_iou_piece_thrs'))
    if not 1 <= len(thrs) <= MAX_PIECES or len(fracs) != len(thrs):
        raise RuntimeError(f'pvrcnn_assign_and_sample: {len(thrs)} neg_iou_piece_thrs for {len(fracs)} neg_piece_fractions; 1 to {MAX_PIECES} '
                           'pieces, one fraction each')
    if any(not 0.0 <= f <= 1.0 for f in fracs) or thrs[-1] <= 0 or any(a <= b for a, b in zip(thrs, thrs[1:])):
        raise RuntimeError('pvrcnn_assign_and_sample: neg_piece_fractions must lie in [0, 1] and neg_iou_piece_thrs be positive and '
                           f'strictly descending, got {fracs}, {thrs}')
    return num, int(num * frac), fracs, thrs


def _host_arrays(pos, neg, low, flags, fracs, thrs):
    f32, C, K = ctypes.c_float, len(pos), len(thrs)
    return ((f32 * C)(*pos), (f32 * C)(*neg), (f32 * C)(*low), (ctypes.c_int32 * C)(*flags), (ctypes.c_double * K)(*fracs), (f32 * K)(*thrs))


_rules = _host.memo(_host_arrays, limit=64)


def _int_vec(t, name, like, rows):
    if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.size(0) != rows or t.dtype.is_floating_point or t.dtype == torch.bool:
        raise RuntimeError(f'shape mismatch: {name} must be an integer ({rows},) tensor, got {getattr(t, "dtype", type(t))} '
                           f'{tuple(getattr(t, "shape", ()))}')
    if t.device != like.device:
        raise RuntimeError(f'{name} is on {t.device}, the proposals on {like.device}')
    return i64c(t.detach())


def _keys(t, name, like, rows):
    if t is None:
        return torch.rand(rows, dtype=torch.float32, device=like.device)     # no sync; under capture the graph's own generator state
    if not isinstance(t, torch.Tensor) or t.shape != (rows,) or not t.dtype.is_floating_point:
        raise RuntimeError(f'shape mismatch: {name} must be a floating-point ({rows},) tensor, got {tuple(getattr(t, "shape", ()))}')
    if t.device != like.device:
        raise RuntimeError(f'{name} is on {t.device}, the proposals on {like.device}')
    return f32c(t.detach())


def pvrcnn_assign_and_sample(proposals, proposal_labels, gt_bboxes, gt_labels, assigner, sampler, prop_batch_cnt=None, gt_batch_cnt=None,
                             keys=None, fill_keys=None, return_assignment=False, as_lists=False):
    """`PVRCNNROIHead._assign_and_sample` for a whole batch, without a host read.

    proposals, proposal_labels, gt_bboxes, gt_labels : per-sample lists [(N_b, 7)], [(N_b,)], [(G_b, 7)], [(G_b,)] (concatenated
                  here, the counts made from the shapes: no read-back), or stacked (N, 7), (N,), (G, 7), (G,) tensors with integer
                  count tensors prop_batch_cnt / gt_batch_cnt (B,) on the same device.  The kernel clamps every count to the rows
                  left and never reads it back.  Boxes are [x, y, z, dx, dy, dz, yaw], z the bottom face; labels are integers.
                  At most 4096 proposals and 1024 gts per sample: the list form raises beyond, a device count is clamped.
    assigner    : one MaxIoUAssigner config (dict or object), or a list of C of them, one per class as the reference's config
                  ships: pos_iou_thr, neg_iou_thr (a float), min_pos_iou, match_low_quality, gt_max_assign_all.  ignore_iof_thr
                  must be negative or absent and iou_calculator, if present, BboxOverlaps3D: anything else raises.  A proposal with
                  label c in [0, C) meets the gts with label c under assigner c; any other label, on either side, meets nothing.
    sampler     : IoUNegPiecewiseSampler config: num (<= 1024), pos_fraction, neg_piece_fractions, neg_iou_piece_thrs (<= 8,
                  strictly descending), neg_pos_ub = -1, add_gt_as_proposals = False.  Anything else raises.
    keys, fill_keys : (N,) and (B * num,) uniforms in [0, 1), the ONLY source of randomness: "draw k of S" takes the k members with
                  the smallest (key, proposal index), and slot j of sample b's output, when the last piece comes up short, takes
                  member min(floor(fill_keys[b * num + j] * m), m - 1) of the last piece in index order (or, that piece being
                  empty, of the negatives chosen so far).  None: drawn here with torch.rand on the device (no sync, capture-safe).
                  The upstream sampler appends POSITIONS within its negative list, not proposal indices, in that fill; that slip
                  is not reproduced: the fill repeats proposals of the list it draws from.

    Returns a dict of static-shaped tensors, npos = int(num * pos_fraction), the samples packed back to back by the counts
    (positives first, in ascending proposal index, then negatives), rows past the counts' sums written as batch id -1 and zeros:
      rois (B * num, 8) [batch id, box];  ious (B * num,) the rows' max_overlap;  inds (B * num,) int64 the proposal's index within
      its sample;  pos_bboxes, pos_gt_bboxes (B * npos, 7);  pos_assigned_gt_inds (B * npos,) int64 into the sample's full gt list;
      pos_batch_cnt, roi_batch_cnt (B,) int32.
    rois[:, 1:] / pos_bboxes / pos_gt_bboxes / ious with the two counts are the stacked operands of `pvrcnn_head_get_targets`, rois
    that of `pvrcnn_head_loss`.  return_assignment adds gt_inds (N,) int64 (-1 ignored, 0 negative, g + 1 positive), max_overlaps
    (N,) and labels (N,) int64 (the assigned gt's label, -1 where gt_ind <= 0).  as_lists reads the counts back ONCE and returns
    per-sample lists under the same names (rois as (n_b, 7) boxes), the reference's shape; nothing is read back otherwise."""
    pos, neg, low, flags = _assigner_rules(assigner)
    num, npos, fracs, thrs = _sampler_rules(sampler)
    if isinstance(proposals, (list, tuple)):
        if prop_batch_cnt is not None or gt_batch_cnt is not None:
            raise RuntimeError('pvrcnn_assign_and_sample: per-sample lists carry their own counts; prop_batch_cnt / gt_batch_cnt go with stacked tensors')
        groups = (proposals, proposal_labels, gt_bboxes, gt_labels)
        if not all(isinstance(g, (list, tuple)) for g in groups) or len({len(g) for g in groups}) != 1 or len(proposals) == 0:
            raise RuntimeError('shape mismatch: proposals, proposal_labels, gt_bboxes and gt_labels must be lists of the same non-zero length')
        for p, pl, g, gl in zip(*groups):
            if not all(isinstance(t, torch.Tensor) for t in (p, pl, g, gl)):
                raise RuntimeError('shape mismatch: every list element must be a tensor')
            if p.dim() != 2 or g.dim() != 2 or pl.shape != (p.size(0),) or gl.shape != (g.size(0),):
                raise RuntimeError(f'shape mismatch: a sample needs proposals (N_b, 7), labels (N_b,), gts (G_b, 7), labels (G_b,), got '
                                   f'{tuple(p.shape)}, {tuple(pl.shape)}, {tuple(g.shape)}, {tuple(gl.shape)}')
            if p.size(0) > MAX_PROPOSALS or g.size(0) > MAX_GTS:
                raise RuntimeError(f'pvrcnn_assign_and_sample: a sample has {p.size(0)} proposals and {g.size(0)} gts; at most '
                                   f'{MAX_PROPOSALS} and {MAX_GTS} are supported')
            if len({t.device for t in (p, pl, g, gl, proposals[0])}) != 1:
                raise RuntimeError('pvrcnn_assign_and_sample: the samples are on different devices')
        dev = proposals[0].device
        pcnt = torch.tensor([p.size(0) for p in proposals], dtype=torch.int32).to(dev)      # sizes are host data: no read back
        gcnt = torch.tensor([g.size(0) for g in gt_bboxes], dtype=torch.int32).to(dev)
        proposals, proposal_labels = torch.cat(list(proposals), 0), torch.cat(list(proposal_labels), 0)
        gt_bboxes, gt_labels = torch.cat(list(gt_bboxes), 0), torch.cat(list(gt_labels), 0)
    else:
        if prop_batch_cnt is None or gt_batch_cnt is None:
            raise RuntimeError('pvrcnn_assign_and_sample: stacked tensors need prop_batch_cnt and gt_batch_cnt')
        if not isinstance(proposals, torch.Tensor):
            raise RuntimeError(f'shape mismatch: proposals must be a tensor or a list of tensors, got {type(proposals).__name__}')
        pcnt = _host.counts_i32(prop_batch_cnt, proposals, 'prop_batch_cnt')
        gcnt = _host.counts_i32(gt_batch_cnt, proposals, 'gt_batch_cnt')
        if pcnt.numel() != gcnt.numel() or pcnt.numel() == 0:
            raise RuntimeError(f'shape mismatch: prop_batch_cnt has {pcnt.numel()} samples, gt_batch_cnt {gcnt.numel()}')
    props, gts = _boxes7(proposals, 'proposals'), _boxes7(gt_bboxes, 'gt_bboxes')
    if gts.device != props.device:
        raise RuntimeError(f'gt_bboxes is on {gts.device}, the proposals on {props.device}')
    dev, N, G, B = props.device, props.size(0), gts.size(0), pcnt.numel()
    if B > 1024:
        raise RuntimeError(f'pvrcnn_assign_and_sample: {B} samples; at most 1024 are supported')
    plab, glab = _int_vec(proposal_labels, 'proposal_labels', props, N), _int_vec(gt_labels, 'gt_labels', props, G)
    k, fk = _keys(keys, 'keys', props, N), _keys(fill_keys, 'fill_keys', props, B * num)
    f32, i64, i32 = torch.float32, torch.int64, torch.int32
    rois = torch.empty((B * num, 8), dtype=f32, device=dev)
    ious = torch.empty((B * num,), dtype=f32, device=dev)
    inds = torch.empty((B * num,), dtype=i64, device=dev)
    pos_bboxes = torch.empty((B * npos, 7), dtype=f32, device=dev)
    pos_gt_bboxes = torch.empty((B * npos, 7), dtype=f32, device=dev)
    pos_gt_inds = torch.empty((B * npos,), dtype=i64, device=dev)
    pos_cnt = torch.empty((B,), dtype=i32, device=dev)
    roi_cnt = torch.empty((B,), dtype=i32, device=dev)
    gt_inds = torch.empty((N,), dtype=i64, device=dev)
    max_overlaps = torch.empty((N,), dtype=f32, device=dev)
    labels = torch.empty((N,), dtype=i64, device=dev)
    stage = torch.empty((B * (2 + num),), dtype=i32, device=dev)
    a_pos, a_neg, a_low, a_flags, a_fracs, a_thrs = _rules(pos, neg, low, flags, fracs, thrs)
    _host.call('gd3d_roi_assign_sample', dev,
               (_ptr(props), _ptr(plab), pcnt.data_ptr(), N, _ptr(gts), _ptr(glab), gcnt.data_ptr(), G, B, _ptr(k), fk.data_ptr(),
                len(pos), a_pos, a_neg, a_low, a_flags, num, npos, len(thrs), a_fracs, a_thrs,
                rois.data_ptr(), ious.data_ptr(), inds.data_ptr(), _ptr(pos_bboxes), _ptr(pos_gt_bboxes), _ptr(pos_gt_inds),
                pos_cnt.data_ptr(), roi_cnt.data_ptr(), _ptr(gt_inds), _ptr(max_overlaps), _ptr(labels), stage.data_ptr()))
    if proposals.dtype != torch.float32:
        rois, ious, pos_bboxes, max_overlaps = (t.to(proposals.dtype) for t in (rois, ious, pos_bboxes, max_overlaps))
    if gt_bboxes.dtype != torch.float32:
        pos_gt_bboxes = pos_gt_bboxes.to(gt_bboxes.dtype)
    out = dict(rois=rois, ious=ious, inds=inds, pos_bboxes=pos_bboxes, pos_gt_bboxes=pos_gt_bboxes, pos_assigned_gt_inds=pos_gt_inds,
               pos_batch_cnt=pos_cnt, roi_batch_cnt=roi_cnt)
    if return_assignment:
        out.update(gt_inds=gt_inds, max_overlaps=max_overlaps, labels=labels)
    if not as_lists:
        return out
    rc, pc, nc = roi_cnt.tolist(), pos_cnt.tolist(), []      # the one read-back
    for c in pcnt.tolist():                                  # as the kernel clamps them
        nc.append(max(0, min(c, N - sum(nc))))
    lists = dict(pos_batch_cnt=pos_cnt, roi_batch_cnt=roi_cnt)
    for key, cnts in (('rois', rc), ('ious', rc), ('inds', rc), ('pos_bboxes', pc), ('pos_gt_bboxes', pc), ('pos_assigned_gt_inds', pc),
                      ('gt_inds', nc), ('max_overlaps', nc), ('labels', nc)):
        if key in out:
            t = out[key][:, 1:] if key == 'rois' else out[key]
            lists[key] = list(torch.split(t[:sum(cnts)], cnts))
    return lists
