"""The SimOTA BEV assigner and its prior generator: the reference's mmdet3d_gaussian/core/bbox/assigners/sim_ota_3d_assigner.py:11-211
(`SimOTABEVAssigner`) and core/anchor/point_3d_generator.py:6-47 (`Point3DRangeGenerator`).

The reference assigns one sample at a time: `points_in_boxes_all` on infinitely tall boxes, two boolean-mask compactions, a
(valid, G, C) repeat of the scores and of the one-hot labels, `LiDARInstance3DBoxes.overlaps`, and one
`torch.topk(..., k=dynamic_ks[gt_idx].item())` per gt box — a host synchronisation per gt and per sample.  Here a whole batch is a
fill and three launches (csrc/simota.hip: a thread per prior flags the candidates, a workgroup per (sample, gt) makes the two
bounded selections, a workgroup per sample resolves the conflicts) with static shapes and no read-back, so the
call captures in a hipGraph together with the head around it.  CUDA tensors go to the kernels on the current stream, CPU tensors
to the `_cpu` twin (csrc/simota_cpu.cpp), which gives the same bits.

mmdet's `BaseAssigner` / `AssignResult`, the registries, `points_in_boxes_all` and `LiDARInstance3DBoxes.overlaps` are third
party, absent here and not pinned by the reference: they are RESTATED (include/gd3d.h spells the sequence out).  torch leaves the
order of equal costs in `topk` unspecified; here ties go to the lower prior index, and a conflicted prior's tie to the lower gt.
"""
import torch

from . import _host, _lib
from ._host import f32c, i64c, ptr_or_null as _ptr

MAX_GTS, MAX_TOPK, MAX_CLASSES, MAX_SAMPLES, MAX_ROWS, MAX_MATCHES = 1024, 32, 32, 1024, 1 << 24, 16384

_workspace_bytes = _host.memo(lambda P, B, G_cap, K: int(_lib.load().gd3d_simota_workspace_bytes(P, B, G_cap, K)))


def _rows(t, cols, name, exact=True):
    ok = isinstance(t, torch.Tensor) and t.dim() == 2 and t.dtype.is_floating_point and \
        (t.size(1) == cols if exact else t.size(1) >= cols)
    if not ok:
        raise RuntimeError(f'shape mismatch: {name} must be a floating-point (rows, {"" if exact else ">= "}{cols}) tensor, got '
                           f'{getattr(t, "dtype", type(t))} {tuple(getattr(t, "shape", ()))}')
    return t.detach()


def _labels(t, rows, name, dev):
    if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.size(0) != rows or t.dtype.is_floating_point or t.dtype == torch.bool:
        raise RuntimeError(f'shape mismatch: {name} must be an integer ({rows},) tensor, got {getattr(t, "dtype", type(t))} '
                           f'{tuple(getattr(t, "shape", ()))}')
    if t.device != dev:
        raise RuntimeError(f'{name} is on {t.device}, the predictions on {dev}')
    return i64c(t.detach())


def simota_assign(pred_scores, decoded_bboxes, priors, gt_bboxes, gt_labels, prior_batch_cnt=None, gt_batch_cnt=None, center_radius=0.5,
                  candidate_topk=10, iou_weight=3.0, cls_weight=1.0, match_init=2.0, shared_priors=False):
    """`SimOTABEVAssigner.assign` for a whole batch, without a host read.

    pred_scores, decoded_bboxes, priors, gt_bboxes, gt_labels : per-sample lists [(P_b, C)], [(P_b, 7)], [(P_b, >= 2)], [(G_b, 7)],
                  [(G_b,)] (concatenated here, the counts made from the shapes: no read-back), or stacked (P, C), (P, 7), (P, >= 2),
                  (G, 7), (G,) tensors with integer count tensors prior_batch_cnt / gt_batch_cnt (B,) on the same device.  The kernels
                  clamp every count to the rows left and never read it back.  Scores are probabilities (clamped into [0, 1], NaN to 0);
                  boxes are [x, y, z, dx, dy, dz, yaw], z the bottom face; columns 0 and 1 of the priors are x and y, read through the
                  strides (no copy of an fp32 prior tensor is made).  Non-fp32 inputs are evaluated in fp32.
    shared_priors : priors is ONE (P_s, >= 2) tensor, the grid every sample shares; sample b's rows are then predictions for the
                  grid's rows 0 .. (a sample's rows past P_s are background).
    center_radius, candidate_topk (1 .. 32), iou_weight, cls_weight, match_init : the reference's constructor arguments.
    At most 32 classes, 1024 samples, 2^24 rows, 1024 gts per sample and gts x candidate_topk <= 16384: the list form raises beyond;
    in the stacked form the first G_cap = min(G, 1024, 16384 // candidate_topk) gts of a sample take part.

    Returns a dict of static-shaped tensors, every element written by every call:
      gt_inds (P,) int64 — 0 background, g + 1 the gt's index within its sample;  labels (P,) int64 — the gt's label or -1;
      max_overlaps (P,) fp32 — the IoU with the assigned gt or -1e8;  pos_cnt (B,) int32;
      pos_inds, pos_gt_inds (B, G_cap * candidate_topk) int64 — each sample's positives in ascending prior index as rows of the
      stacked operands (`decoded_bboxes[pos_inds]`, `gt_bboxes[pos_gt_inds]`), padded with -1: a head gathers through them
      without `nonzero()`.  The sequence of operations is spelt out in include/gd3d.h."""
    K = int(candidate_topk)
    if not 1 <= K <= MAX_TOPK:
        raise RuntimeError(f'simota_assign: candidate_topk = {candidate_topk}; 1 to {MAX_TOPK} are supported')
    params = [float(center_radius), float(iou_weight), float(cls_weight), float(match_init)]
    if any(v != v for v in params):
        raise RuntimeError('simota_assign: center_radius, iou_weight, cls_weight and match_init must not be NaN')
    if isinstance(pred_scores, (list, tuple)):
        if prior_batch_cnt is not None or gt_batch_cnt is not None:
            raise RuntimeError('simota_assign: per-sample lists carry their own counts; prior_batch_cnt / gt_batch_cnt go with stacked tensors')
        groups = [pred_scores, decoded_bboxes, gt_bboxes, gt_labels] + ([] if shared_priors else [priors])
        if not all(isinstance(g, (list, tuple)) for g in groups) or len({len(g) for g in groups}) != 1 or len(pred_scores) == 0:
            raise RuntimeError('shape mismatch: pred_scores, decoded_bboxes, priors, gt_bboxes and gt_labels must be lists of the same '
                               'non-zero length (priors ONE tensor with shared_priors)')
        if not all(isinstance(t, torch.Tensor) for g in groups for t in g):
            raise RuntimeError('shape mismatch: every list element must be a tensor')
        for i, (s, d, g, gl) in enumerate(zip(pred_scores, decoded_bboxes, gt_bboxes, gt_labels)):
            pr = priors if shared_priors else priors[i]
            if s.dim() != 2 or d.dim() != 2 or g.dim() != 2 or d.size(0) != s.size(0) or gl.shape != (g.size(0),) or \
                    not isinstance(pr, torch.Tensor) or pr.dim() != 2 or pr.size(0) != s.size(0):
                raise RuntimeError(f'shape mismatch: a sample needs scores (P_b, C), boxes (P_b, 7), priors (P_b, >= 2), gts (G_b, 7), labels '
                                   f'(G_b,), got {tuple(s.shape)}, {tuple(d.shape)}, {tuple(getattr(pr, "shape", ()))}, {tuple(g.shape)}, '
                                   f'{tuple(gl.shape)}')
            if g.size(0) > MAX_GTS or g.size(0) * K > MAX_MATCHES:
                raise RuntimeError(f'simota_assign: a sample has {g.size(0)} gts; at most {MAX_GTS}, and gts x candidate_topk <= {MAX_MATCHES}, '
                                   'are supported')
            if len({t.device for t in (s, d, g, gl, pr, pred_scores[0])}) != 1:
                raise RuntimeError('simota_assign: the samples are on different devices')
        dev = pred_scores[0].device
        pcnt = torch.tensor([s.size(0) for s in pred_scores], dtype=torch.int32).to(dev)      # sizes are host data: no read back
        gcnt = torch.tensor([g.size(0) for g in gt_bboxes], dtype=torch.int32).to(dev)
        g_cap = max(g.size(0) for g in gt_bboxes)
        pred_scores, decoded_bboxes = torch.cat(list(pred_scores), 0), torch.cat(list(decoded_bboxes), 0)
        gt_bboxes, gt_labels = torch.cat(list(gt_bboxes), 0), torch.cat(list(gt_labels), 0)
        if not shared_priors:
            if len({p.size(1) for p in priors}) != 1:
                raise RuntimeError('shape mismatch: the samples\' priors differ in their number of columns')
            priors = torch.cat(list(priors), 0)
    else:
        if prior_batch_cnt is None or gt_batch_cnt is None:
            raise RuntimeError('simota_assign: stacked tensors need prior_batch_cnt and gt_batch_cnt')
        if not isinstance(pred_scores, torch.Tensor):
            raise RuntimeError(f'shape mismatch: pred_scores must be a tensor or a list of tensors, got {type(pred_scores).__name__}')
        pcnt = _host.counts_i32(prior_batch_cnt, pred_scores, 'prior_batch_cnt')
        gcnt = _host.counts_i32(gt_batch_cnt, pred_scores, 'gt_batch_cnt')
        if pcnt.numel() != gcnt.numel() or pcnt.numel() == 0:
            raise RuntimeError(f'shape mismatch: prior_batch_cnt has {pcnt.numel()} samples, gt_batch_cnt {gcnt.numel()}')
        g_cap = None
    scores, boxes = f32c(_rows(pred_scores, 1, 'pred_scores', exact=False)), f32c(_rows(decoded_bboxes, 7, 'decoded_bboxes'))
    gts, pri = f32c(_rows(gt_bboxes, 7, 'gt_bboxes')), _rows(priors, 2, 'priors', exact=False)
    dev, P, C, G, B = scores.device, scores.size(0), scores.size(1), gts.size(0), pcnt.numel()
    if boxes.size(0) != P or (not shared_priors and pri.size(0) != P):
        raise RuntimeError(f'shape mismatch: {P} score rows, {boxes.size(0)} box rows, {pri.size(0)} prior rows')
    if any(t.device != dev for t in (boxes, gts, pri)):
        raise RuntimeError(f'simota_assign: the operands are on different devices ({dev}, {boxes.device}, {pri.device}, {gts.device})')
    if C > MAX_CLASSES or B > MAX_SAMPLES or P > MAX_ROWS or G > MAX_ROWS or pri.size(0) > MAX_ROWS:
        raise RuntimeError(f'simota_assign: {C} classes, {B} samples, {P} rows, {G} gts; at most {MAX_CLASSES}, {MAX_SAMPLES}, {MAX_ROWS} and '
                           f'{MAX_ROWS} are supported')
    glab = _labels(gt_labels, G, 'gt_labels', dev)
    if pri.dtype != torch.float32:
        pri = pri.float()
    if pri.numel() and (pri.stride(1) != 1 or pri.stride(0) < 2 or pri.stride(0) > (1 << 20)):
        pri = pri.contiguous()
    stride = pri.stride(0) if pri.size(0) > 1 else max(pri.size(1), 2)
    if g_cap is None:
        g_cap = min(G, MAX_GTS, MAX_MATCHES // K)
    L = g_cap * K
    i64, i32, f32 = torch.int64, torch.int32, torch.float32
    gt_inds = torch.empty((P,), dtype=i64, device=dev)
    labels = torch.empty((P,), dtype=i64, device=dev)
    max_overlaps = torch.empty((P,), dtype=f32, device=dev)
    pos_cnt = torch.empty((B,), dtype=i32, device=dev)
    pos_inds = torch.empty((B, L), dtype=i64, device=dev)
    pos_gt_inds = torch.empty((B, L), dtype=i64, device=dev)
    ws_bytes = _workspace_bytes(P, B, g_cap, K)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    _host.call('gd3d_simota_assign', dev,
               (_ptr(scores), _ptr(boxes), _ptr(pri), pri.size(0), stride, int(bool(shared_priors)), pcnt.data_ptr(), P, _ptr(gts),
                _ptr(glab), gcnt.data_ptr(), G, B, C, g_cap, params[0], K, params[1], params[2], params[3], _ptr(gt_inds), _ptr(labels),
                _ptr(max_overlaps), pos_cnt.data_ptr(), _ptr(pos_inds), _ptr(pos_gt_inds), ws.data_ptr(), ws_bytes))
    return dict(gt_inds=gt_inds, labels=labels, max_overlaps=max_overlaps, pos_cnt=pos_cnt, pos_inds=pos_inds, pos_gt_inds=pos_gt_inds)


class SimOTAAssignResult:
    """What `SimOTABEVAssigner.assign` returns: the four fields of mmdet's `AssignResult` (absent here)."""

    def __init__(self, num_gts, gt_inds, max_overlaps, labels=None):
        self.num_gts = num_gts
        self.gt_inds = gt_inds
        self.max_overlaps = max_overlaps
        self.labels = labels

    @property
    def num_preds(self):
        return len(self.gt_inds)

    def __repr__(self):
        return f'<SimOTAAssignResult(num_gts={self.num_gts}, gt_inds.shape={tuple(self.gt_inds.shape)})>'


class SimOTABEVAssigner:
    """The reference's class (constructor and `assign` of one sample) over `simota_assign`.  `dir_weight` is accepted and unused,
    as in the reference; `debug=True` raises: the matplotlib viewer is not taken."""
    INF = 100000000
    EPS = 0.00000001

    def __init__(self, center_radius=0.5, candidate_topk=10, iou_weight=3.0, dir_weight=0.0, cls_weight=1.0, match_init=2.0, debug=False):
        if debug:
            raise RuntimeError('SimOTABEVAssigner: debug=True (the matplotlib viewer of the reference) is not implemented')
        self.center_radius = center_radius
        self.candidate_topk = candidate_topk
        self.iou_weight = iou_weight
        self.dir_weight = dir_weight
        self.cls_weight = cls_weight
        self.match_init = match_init
        self.debug = debug

    def assign(self, pred_scores, decoded_bboxes, priors, gt_bboxes, gt_bboxes_ignore=None, gt_labels=None):
        """One sample: pred_scores (P, C), decoded_bboxes (P, 7), priors (P, >= 2), gt_bboxes (G, 7), gt_labels (G,).  Returns an object
        with num_gts, gt_inds (P,) int64 (0 background, g + 1), max_overlaps (P,) (the IoU with the assigned gt, -1e8 for background;
        0 when there is no gt or no prior, as in the reference) and labels (P,) int64 (-1 background; None without gt_labels)."""
        num_gt = gt_bboxes.size(0)
        has_labels = gt_labels is not None
        if not has_labels:
            gt_labels = torch.zeros((num_gt,), dtype=torch.int64, device=gt_bboxes.device)
        out = simota_assign([pred_scores], [decoded_bboxes], [priors], [gt_bboxes], [gt_labels], center_radius=self.center_radius,
                            candidate_topk=self.candidate_topk, iou_weight=self.iou_weight, cls_weight=self.cls_weight,
                            match_init=self.match_init)
        max_overlaps = out['max_overlaps']
        if num_gt == 0 or decoded_bboxes.size(0) == 0:
            max_overlaps = torch.zeros_like(max_overlaps)
        return SimOTAAssignResult(num_gt, out['gt_inds'], max_overlaps, labels=out['labels'] if has_labels else None)


class Point3DRangeGenerator:
    """The reference's prior generator: per level a (ny, nx, 3) grid of [x, y, stride] over `ranges[level]` = [x0, y0, x1, y1, ...].
    Plain torch, built on the CPU in fp32 and moved to `device`, so the priors are the same bits wherever they are used; it runs
    once per shape."""

    def __init__(self, ranges, base=1):
        self.ranges = ranges
        self.base = base

    @property
    def num_levels(self):
        return len(self.ranges)

    def grid_anchors(self, featmap_sizes, device='cuda'):
        return self.grid_priors(featmap_sizes, device)

    def grid_priors(self, featmap_sizes, device='cuda'):
        assert self.num_levels == len(featmap_sizes)
        return [self.single_level_grid_priors(featmap_sizes[i], level_idx=i, device=device) for i in range(self.num_levels)]

    def single_level_grid_priors(self, feature_size, level_idx, device='cuda'):
        if len(feature_size) == 2:
            feature_size = [1, feature_size[0], feature_size[1]]
        anchor_range = torch.tensor(self.ranges[level_idx], dtype=torch.float32)
        y_centers = torch.linspace(anchor_range[1], anchor_range[3], feature_size[1])
        x_centers = torch.linspace(anchor_range[0], anchor_range[2], feature_size[2])
        grid_x_centers, grid_y_centers = torch.meshgrid(x_centers, y_centers, indexing='ij')
        stride = self.base * (anchor_range[2] - anchor_range[0]) / (feature_size[2] - 1)
        stride = torch.full_like(grid_x_centers, stride.item())
        priors = torch.stack((grid_x_centers, grid_y_centers, stride), dim=-1)
        return priors.permute((1, 0, 2)).contiguous().to(device)
