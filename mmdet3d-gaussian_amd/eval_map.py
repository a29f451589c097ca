"""The reference's flexible mAP evaluator on this package's kernels, with the reference's surface
(/root/reference/mmdet3d_gaussian/core/evaluation/):

* ``FlexibleStatisticsEval`` / ``eval_map_flexible`` — mean_ap_flexible.py:17-237;
* ``NoBreakdown`` / ``RangeBreakdown`` / ``VolumeBreakdown`` — breakdown.py:5-88;
* ``LidarCenterTransBEV`` / ``LidarIOU3D`` / ``LidarIOUBEV`` — affinity.py:5-32;
* ``MatcherCoCo`` — matcher.py:6-36;

registered in registry.py's EVAL_* registries (builder.py:4-23), so the reference's config dicts build unchanged.

Per frame and class the affinity matrix is computed once (iou_3d / iou_bev / trans_bev), `match_coco` runs once per breakdown and
`tp_records` turns each result into rows of ONE record buffer that lives where the detections live; the dataset's AP of every
(class, breakdown, threshold) is then ONE `ap_accumulate` call and one read-back.  numpy inputs move to the GPU when there is one;
CPU tensors (and numpy without a GPU) run the library's `_cpu` twins.  With `frame_batch=N` the per-frame stage runs for N frames
per `frames_records` call instead — the same records, breakdown-major inside a batch, and the same results.  What differs from the reference is listed in
INTEGRATION.md §1c: ties between scores have a definite order, `nproc` starts no process, the table is plain text.
"""
import logging
from collections import OrderedDict

import numpy as np
import torch

from . import evaluation as _ev
from .iou3d import iou_3d, iou_bev
from .registry import (EVAL_AFFINITYCALS, EVAL_BREAKDOWNS, EVAL_MATCHERS, build_eval_affinity_calculator, build_eval_breakdown,
                       build_eval_matcher, build_eval_tp_metric)


# ---- breakdowns (breakdown.py:5-88): numpy in, numpy out, as in the reference; tensors in, a tensor on their device out ----------

def _is_np(x):
    return not isinstance(x, torch.Tensor)


def _zeros_bool(rows, boxes):
    if _is_np(boxes):
        return np.zeros((rows, len(boxes)), dtype=bool)
    return torch.zeros((rows, len(boxes)), dtype=torch.bool, device=boxes.device)


def _clear_ignored(flags, attrs):
    if attrs is not None and 'ignore' in attrs:
        ign = attrs['ignore']
        if _is_np(flags):
            flags[:, np.asarray(ign, dtype=bool)] = False
        else:
            flags[:, torch.as_tensor(ign, dtype=torch.bool, device=flags.device)] = False
    return flags


@EVAL_BREAKDOWNS.register_module()
class NoBreakdown:

    def __init__(self, classes, apply_to=None, *args, **kwargs):
        if apply_to is None:
            apply_to = classes
        self.classes = classes
        self.apply_to = apply_to
        self.names = ['All']

    def breakdown_flags(self, boxes, attrs=None):
        return _clear_ignored(~_zeros_bool(1, boxes), attrs)

    def breakdown(self, boxes, label, attrs=None):
        flags = self.breakdown_flags(boxes, attrs)
        if self.classes[label] in self.apply_to:
            return flags
        return flags[:0]

    def breakdown_names(self, label):
        if self.classes[label] in self.apply_to:
            return [f'{n}' for n in self.names]
        return []


class _IntervalBreakdown(NoBreakdown):
    """A breakdown by half-open intervals [lo, hi) of one quantity of a box; `ATTR` names the attribute that overrides it."""
    ATTR = None

    def __init__(self, ranges, classes, apply_to=None, *args, **kwargs):
        super().__init__(classes, apply_to, *args, **kwargs)
        self.names = []
        self.ranges = []
        for k in ranges:
            self.names.append(k)
            self.ranges.append(ranges[k])

    def quantity(self, boxes):
        raise NotImplementedError

    def breakdown_flags(self, boxes, attrs=None):
        if attrs is not None and self.ATTR in attrs:
            q = attrs[self.ATTR]
            q = np.asarray(q) if _is_np(boxes) else torch.as_tensor(q, device=boxes.device)
        else:
            q = self.quantity(boxes)
        flags = _zeros_bool(len(self.ranges), boxes)
        for i, (lo, hi) in enumerate(self.ranges):
            flags[i] = (q >= lo) & (q < hi)
        return _clear_ignored(flags, attrs)


@EVAL_BREAKDOWNS.register_module()
class RangeBreakdown(_IntervalBreakdown):
    ATTR = 'distance'

    def quantity(self, boxes):
        xyz = boxes[:, :3]
        return np.linalg.norm(xyz, axis=-1) if _is_np(boxes) else torch.linalg.vector_norm(xyz, dim=-1)


@EVAL_BREAKDOWNS.register_module()
class VolumeBreakdown(_IntervalBreakdown):
    ATTR = 'volumn'     # the reference's spelling (breakdown.py:79)

    def quantity(self, boxes):
        return np.prod(boxes[:, 3:6], axis=-1) if _is_np(boxes) else torch.prod(boxes[:, 3:6], dim=-1)


# ---- affinities (affinity.py:5-32) and the matcher (matcher.py:6-36) ---------------------------------------------------------------

@EVAL_AFFINITYCALS.register_module()
class LidarCenterTransBEV:
    LARGER_CLOSER = False

    def __call__(self, det_bboxes, gt_bboxes, gt_iscrowd=None):
        assert gt_iscrowd is None, 'Does not support crowd annotation yet'
        return _ev.trans_bev(det_bboxes, gt_bboxes)


@EVAL_AFFINITYCALS.register_module()
class LidarIOU3D:
    LARGER_CLOSER = True

    def __init__(self, z_offset=0.5):
        self.z_offset = z_offset

    def __call__(self, det_bboxes, gt_bboxes, gt_iscrowd=None):
        assert gt_iscrowd is None, 'Does not support crowd annotation yet'
        return iou_3d(det_bboxes, gt_bboxes, self.z_offset)


@EVAL_AFFINITYCALS.register_module()
class LidarIOUBEV:
    LARGER_CLOSER = True

    def __call__(self, det_bboxes, gt_bboxes, gt_iscrowd=None):
        assert gt_iscrowd is None, 'Does not support crowd annotation yet'
        return iou_bev(det_bboxes, gt_bboxes)


class BaseMatcher:
    def __init__(self, match_thrs, affinity_cost_negate=True):
        self._match_thrs = match_thrs
        self.negate = affinity_cost_negate

    @property
    def match_thrs(self):
        return self._match_thrs

    def __call__(self, affinity, gt_isignore=None, gt_iscrowd=None):
        num_gt = affinity.shape[1]
        if gt_iscrowd is None:
            gt_iscrowd = np.zeros(num_gt, dtype=bool)
        if gt_isignore is None:
            gt_isignore = np.zeros(num_gt, dtype=bool)
        thrs = np.array(self.match_thrs, np.float32)
        if self.negate:
            return self.match(-affinity, -thrs, gt_isignore, gt_iscrowd)
        return self.match(affinity, thrs, gt_isignore, gt_iscrowd)

    def match(self, affinity, match_thrs, gt_isignore=None, gt_iscrowd=None):
        raise NotImplementedError


@EVAL_MATCHERS.register_module()
class MatcherCoCo(BaseMatcher):

    def match(self, affinity, match_thrs, gt_isignore=None, gt_iscrowd=None):
        return _ev.match_coco(affinity, match_thrs, gt_isignore, gt_iscrowd)


# ---- the record buffer -------------------------------------------------------------------------------------------------------------

class _Records:
    """The four record columns on one device; the capacity doubles, unused rows keep group -1 (they count for nothing)."""
    DTYPES = (torch.int32, torch.float32, torch.int32, torch.int32)

    def __init__(self, device, capacity=4096):
        self.device = device
        self.rows = 0
        self.cols = self._alloc(capacity)

    def _alloc(self, capacity):
        return tuple(torch.full((capacity,), -1, dtype=dt, device=self.device) if i == 0 else
                     torch.zeros((capacity,), dtype=dt, device=self.device) for i, dt in enumerate(self.DTYPES))

    def reserve(self, more):
        need = self.rows + more
        cap = self.cols[0].numel()
        if need > cap:
            while cap < need:
                cap *= 2
            new = self._alloc(cap)
            for n, o in zip(new, self.cols):
                n[:self.rows] = o[:self.rows]
            self.cols = new


def _device_of(det_results):
    """Where the evaluation runs: the device of tensor detections; numpy moves to the current GPU when there is one."""
    for frame in det_results:
        for d in frame:
            if isinstance(d, torch.Tensor):
                return d.device
            return torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else torch.device('cpu')
    return torch.device('cpu')


def _host_np(x, dtype=None):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.asarray(x) if dtype is None else np.asarray(x, dtype=dtype)


class FlexibleStatisticsEval(object):

    def __init__(self, classes, match_thrs, breakdown, affinity_calculator, matcher, tp_metrics, nproc):
        self.classes = classes
        self.breakdown = [build_eval_breakdown({'type': 'NoBreakdown'}, classes=classes)]
        self.breakdown += [build_eval_breakdown(bkd, classes=classes) for bkd in breakdown]
        self.affinity_calculator = build_eval_affinity_calculator(affinity_calculator)
        self.matcher = build_eval_matcher(matcher, match_thrs=match_thrs,
                                          affinity_cost_negate=self.affinity_calculator.LARGER_CLOSER)
        self.tp_metric = [build_eval_tp_metric(m) for m in tp_metrics]
        self.nproc = nproc      # accepted, never starts a process: one process owns the GPU

    # -- the per-frame stage ---------------------------------------------------------------------------------------------------------

    def _frame_records(self, det, anno, rec, group_of, num_gt):
        """mean_ap_flexible.py:37-128 for one frame, appended to `rec`.  group_of(cls, names) -> the group id of the class's first
        breakdown row; num_gt (list) gains the frame's gt counts.  Returns [(cls_name, bkd_name, gt_count, first row, rows)]."""
        dev = rec.device
        num_thrs = len(self.matcher.match_thrs)
        gt_bboxes = _host_np(anno['gt_bboxes'])
        gt_labels = _host_np(anno['gt_labels'])
        gt_attrs = {k: _host_np(v) for k, v in anno['gt_attrs'].items()}
        blocks = []
        for cls in range(len(det)):
            cls_name = self.classes[cls] if self.classes is not None else cls
            d = det[cls]
            if isinstance(d, torch.Tensor):
                d = d.detach().to(device=dev, dtype=torch.float32)
                host_boxes = None
            else:
                host_boxes = np.asarray(d)[:, :-1]
                d = torch.from_numpy(np.ascontiguousarray(d, dtype=np.float32)).to(dev)
            # a stable descending sort: equal scores keep their order (the reference's argsort()[::-1] leaves them to quicksort)
            scores, sort_ind = torch.sort(d[:, -1], descending=True, stable=True)
            boxes = d[:, :-1][sort_ind].contiguous()
            D = scores.numel()

            cls_gt_msk = gt_labels == cls
            cls_gt_bboxes = gt_bboxes[cls_gt_msk]
            cls_gt_attrs = {k: v[cls_gt_msk] for k, v in gt_attrs.items()}
            num_ignore = int(np.count_nonzero(cls_gt_attrs['ignore'])) if 'ignore' in cls_gt_attrs else 0
            crowd = cls_gt_attrs['iscrowd'] if 'iscrowd' in cls_gt_attrs else None
            G = len(cls_gt_bboxes)

            det_bkd, gt_bkd, names = [], [], []
            for fun in self.breakdown:
                # detections given on the host are broken down there, in their own precision, as the reference does
                det_bkd.append(fun.breakdown(host_boxes if host_boxes is not None else boxes, cls))
                gt_bkd.append(fun.breakdown(cls_gt_bboxes, cls, cls_gt_attrs))
                names += fun.breakdown_names(cls)
            gt_bkd = np.concatenate(gt_bkd, axis=0)
            if host_boxes is not None:
                det_bkd = torch.from_numpy(np.concatenate(det_bkd, axis=0).astype(np.uint8)).to(dev)[:, sort_ind]
            else:
                det_bkd = torch.cat(det_bkd, dim=0).to(torch.uint8)
            det_bkd = det_bkd.contiguous()
            num_bkd = gt_bkd.shape[0]
            gid0 = group_of(cls, names)
            for b in range(num_bkd):
                num_gt[gid0 + b] += int(np.count_nonzero(gt_bkd[b]))

            rec.reserve(D * num_bkd)
            first = rec.rows
            if G == 0 or D == 0:
                affinity = None
            else:
                affinity = self.affinity_calculator(boxes, torch.from_numpy(np.ascontiguousarray(cls_gt_bboxes, dtype=np.float32)).to(dev),
                                                    crowd)
            gt_dev = torch.from_numpy(gt_bkd).to(dev)      # flags of every breakdown row, one copy
            for b in range(num_bkd):
                matched = None if affinity is None else self.matcher(affinity, ~gt_dev[b], crowd)
                if D > 0:
                    _ev.tp_records(matched, det_bkd[b], gt_dev[b], scores, gid0 + b, num_thrs=num_thrs, out=rec.cols, row=rec.rows)
                blocks.append((cls_name, names[b], int(np.count_nonzero(gt_bkd[b])), rec.rows, D))
                rec.rows += D
            if affinity is not None and D > 0 and num_bkd > 1:
                # the reference keeps ONE tp array per class and frame (:90) and hands it to every breakdown's tuple (:124-126) after
                # rewriting it in place (:115-116): all breakdowns of the class carry the LAST breakdown's true positives
                tp = rec.cols[2]
                last = tp[first + (num_bkd - 1) * D:first + num_bkd * D]
                tp[first:first + (num_bkd - 1) * D].view(num_bkd - 1, D).copy_(last.expand(num_bkd - 1, D))
        return blocks

    # -- the per-frame stage for a batch of frames: ONE frames_records call ----------------------------------------------------------------

    def _batch_mode(self):
        """The `frames_records` mode of this evaluator.  The batched path replays exactly the built-in classes; a subclass may compute
        anything, so it is refused by name instead of being silently replaced."""
        aff, mode = self.affinity_calculator, None
        for cls, m in ((LidarIOU3D, 'iou3d'), (LidarIOUBEV, 'ioubev'), (LidarCenterTransBEV, 'trans')):
            if type(aff) is cls:
                mode = m
        if mode is None:
            raise ValueError(f'frame_batch > 0 serves LidarIOU3D, LidarIOUBEV and LidarCenterTransBEV, not {type(aff).__name__}')
        if type(self.matcher) is not MatcherCoCo:
            raise ValueError(f'frame_batch > 0 serves MatcherCoCo, not {type(self.matcher).__name__}')
        for fun in self.breakdown:
            if type(fun) not in (NoBreakdown, RangeBreakdown, VolumeBreakdown):
                raise ValueError(f'frame_batch > 0 serves NoBreakdown, RangeBreakdown and VolumeBreakdown, not {type(fun).__name__}')
        return mode

    def _class_rows(self, cls, group_of):
        """(R,) int32: the group of the class's breakdown row b, -1 where the row's breakdown does not apply to the class."""
        names, rows = [], []
        for fun in self.breakdown:
            mine = fun.breakdown_names(cls)
            rows += [len(names) + k if mine else -1 for k in range(len(fun.names))]
            names += mine
        gid0 = group_of(cls, names)
        return np.array([gid0 + r if r >= 0 else -1 for r in rows], np.int32)

    def _batch_records(self, dets, annos, rec, group_of, num_gt, mode):
        """`_frame_records` for a batch of frames in one `frames_records` call.  Problem p = (frame, class), frame-major.  Returns False,
        having done nothing, for a batch this path does not serve: the caller then goes frame by frame, with the same results."""
        dev = rec.device
        num_cls = len(dets[0])
        flat = [d for det in dets for d in det]
        as_tensor = [isinstance(d, torch.Tensor) for d in flat]
        if num_cls == 0 or any(len(det) != num_cls for det in dets) or (any(as_tensor) and not all(as_tensor)):
            return False
        if not all(as_tensor):
            flat = [np.asarray(d) for d in flat]
            if len({d.dtype for d in flat}) != 1:        # broken down in their own precision: one precision per batch
                return False
        keys = set(annos[0]['gt_attrs'].keys())
        if any(set(a['gt_attrs'].keys()) != keys for a in annos) or 'iscrowd' in keys:
            return False           # (an `iscrowd` attribute meets the affinity callables' assertion on the per-frame path)
        # the gts of every problem, packed on the host in their own precision
        gt_boxes, gt_attrs, G_p = [], {k: [] for k in keys}, []
        for anno in annos:
            boxes, labels = _host_np(anno['gt_bboxes']), _host_np(anno['gt_labels'])
            attrs = {k: _host_np(anno['gt_attrs'][k]) for k in keys}
            for cls in range(num_cls):
                msk = labels == cls
                gt_boxes.append(boxes[msk])
                for k in keys:
                    gt_attrs[k].append(attrs[k][msk])
                G_p.append(len(gt_boxes[-1]))
        if max(G_p) > _ev.FRAMES_MAX_GT or len({b.dtype for b in gt_boxes}) != 1 or any(len({a.dtype for a in v}) != 1 for v in gt_attrs.values()):
            return False
        gt_all = np.concatenate(gt_boxes, axis=0)
        attrs_all = {k: np.concatenate(v, axis=0) for k, v in gt_attrs.items()}
        gt_seg = np.concatenate([[0], np.cumsum(G_p)])
        D_p = [len(d) for d in flat]
        det_seg = np.concatenate([[0], np.cumsum(D_p)])
        P, ND = len(flat), int(det_seg[-1])
        # every breakdown's flags ONCE on the packed boxes; a class's rows of a breakdown that does not apply get group -1
        gt_flag = np.concatenate([fun.breakdown_flags(gt_all, attrs_all) for fun in self.breakdown], axis=0)
        rows_of = [self._class_rows(cls, group_of) for cls in range(num_cls)]
        group = np.stack([rows_of[p % num_cls] for p in range(P)])
        counts = np.concatenate([np.zeros((gt_flag.shape[0], 1), np.int64), np.cumsum(gt_flag, axis=1, dtype=np.int64)], axis=1)
        per_problem = counts[:, gt_seg[1:]] - counts[:, gt_seg[:-1]]            # (R, P): the gts of the row in the problem
        for p in range(P):
            for b in np.nonzero(group[p] >= 0)[0]:
                num_gt[group[p, b]] += int(per_problem[b, p])
        if ND == 0:
            return True
        # the detections: packed, then each problem ordered by descending score, stably — two stable sorts (score descending, then
        # problem id), so NaN and +-0 fall where the per-problem torch.sort(descending=True, stable=True) puts them
        if all(as_tensor):
            packed = torch.cat([d.detach().to(device=dev, dtype=torch.float32) for d in flat], dim=0)
            host_boxes = None
        else:
            host = np.concatenate(flat, axis=0)
            host_boxes = host[:, :-1]
            packed = torch.from_numpy(np.ascontiguousarray(host, dtype=np.float32)).to(dev)
        pid = torch.from_numpy(np.repeat(np.arange(P), D_p)).to(dev)
        by_score = torch.sort(packed[:, -1], descending=True, stable=True)[1]
        order = by_score[torch.sort(pid[by_score], stable=True)[1]]
        scores = packed[:, -1][order].contiguous()
        boxes = packed[:, :-1][order].contiguous()
        if host_boxes is not None:
            # detections given on the host are broken down there, in their own precision, as the reference does
            det_flag = np.concatenate([fun.breakdown_flags(host_boxes) for fun in self.breakdown], axis=0)
            det_flag = torch.from_numpy(det_flag.astype(np.uint8)).to(dev)[:, order]
        else:
            det_flag = torch.cat([fun.breakdown_flags(boxes) for fun in self.breakdown], dim=0).to(torch.uint8)
        R = group.shape[1]
        # Rows land breakdown-major inside the batch, (b, detection), where the per-frame path appends (frame, class, b, rank).
        # ap_accumulate depends only on the relative order of the rows of ONE group, and under both layouts that order is frame
        # order, then rank: a group's rows are one breakdown row of one class, and the packed detections are frame-major.
        rec.reserve(R * ND)
        _ev.frames_records(boxes, scores, det_seg, torch.from_numpy(np.ascontiguousarray(gt_all, dtype=np.float32)).to(dev), gt_seg,
                           det_flag.contiguous(), gt_flag, group, np.array(self.matcher.match_thrs, np.float32), mode,
                           z_offset=getattr(self.affinity_calculator, 'z_offset', 0.5), negate=self.matcher.negate, alias_tp=True,
                           out=rec.cols, row=rec.rows)
        rec.rows += R * ND
        return True

    def _group_table(self):
        """Group ids in the reference's tp_score_info order: class-major, NoBreakdown first, breakdowns that do not apply skipped."""
        table, start = [], {}

        def group_of(cls, names):
            if cls not in start:
                start[cls] = len(table)
                cls_name = self.classes[cls] if self.classes is not None else cls
                table.extend((cls_name, n) for n in names)
            return start[cls]
        return table, start, group_of

    def statistics_single(self, input):
        """The reference's per-frame tuples (cls_name, bkd_name, gt_count, scores, tp (T, D) bool, msk (T, D) bool) as numpy: the
        records of the frame read back and unpacked (statistics_eval keeps them on the device instead)."""
        det, anno = input
        rec = _Records(_device_of([det]), 256)
        table, _, group_of = self._group_table()
        num_gt = [0] * (len(det) * sum(len(f.names) for f in self.breakdown))
        blocks = self._frame_records(det, anno, rec, group_of, num_gt)
        _, score, tp, msk = (c[:rec.rows].cpu().numpy() for c in rec.cols)
        bits = np.arange(len(self.matcher.match_thrs), dtype=np.int32)[:, None]
        out = []
        for cls_name, bkd_name, gt_count, row, rows in blocks:
            sl = slice(row, row + rows)
            out.append((cls_name, bkd_name, gt_count, score[sl], ((tp[sl][None, :] >> bits) & 1).astype(bool),
                        ((msk[sl][None, :] >> bits) & 1).astype(bool)))
        return out

    # -- the accumulate stage --------------------------------------------------------------------------------------------------------

    def _results(self, table, num_gt, num_det, recall, ap):
        out = []
        for g, (cls, bkd) in enumerate(table):
            for t, thr in enumerate(self.matcher.match_thrs):
                key = dict(class_name=cls, breakdown=bkd, match_threshold=thr)
                value = dict(num_det=int(num_det[g, t]), num_gt=num_gt[g], recall=recall[g, t], mAP=np.float32(ap[g, t]))
                out.append((key, value))
        return out

    def statistics_accumulate(self, input):
        """One (class, breakdown) group given as the reference's tuple: the same AP through `ap_accumulate` with K = 1."""
        cls, bkd, num_gt, score, tp, bkd_msk = input
        num_thrs = len(self.matcher.match_thrs)
        w = (1 << np.arange(num_thrs, dtype=np.int64))[:, None]
        pack = lambda m: (np.asarray(m, dtype=np.int64) * w).sum(0).astype(np.uint32).view(np.int32)   # noqa: E731
        score = _host_np(score, np.float32)
        nd, rc, ap = _ev.ap_accumulate(np.zeros(len(score), np.int32), score, pack(tp), pack(bkd_msk), np.array([num_gt], np.int64), num_thrs)
        res = torch.stack([nd.double(), rc, ap]).cpu().numpy()
        return self._results([(cls, bkd)], [num_gt], res[0], res[1], res[2])

    def statistics_eval(self, det_results, annotations, frame_batch=0):
        """frame_batch 0 / None: one frame at a time (`_frame_records`); N > 0: N frames per `frames_records` call, the same results."""
        num_thrs = len(self.matcher.match_thrs)
        rec = _Records(_device_of(det_results))
        table, _, group_of = self._group_table()
        num_cls = len(det_results[0]) if len(det_results) else 0
        num_gt = [0] * (num_cls * sum(len(f.names) for f in self.breakdown))
        if not frame_batch:
            for det, anno in zip(det_results, annotations):
                self._frame_records(det, anno, rec, group_of, num_gt)
        else:
            mode = self._batch_mode()
            pairs = list(zip(det_results, annotations))
            for first in range(0, len(pairs), int(frame_batch)):
                batch = pairs[first:first + int(frame_batch)]
                if not self._batch_records([d for d, _ in batch], [a for _, a in batch], rec, group_of, num_gt, mode):
                    for det, anno in batch:
                        self._frame_records(det, anno, rec, group_of, num_gt)
        if not table:
            return []
        num_gt = num_gt[:len(table)]
        # ONE call over the whole buffer (static shape: the unused rows carry group -1) and ONE read-back
        nd, rc, ap = _ev.ap_accumulate(*rec.cols, torch.tensor(num_gt, dtype=torch.int64).to(rec.device), num_thrs)
        res = torch.stack([nd.double(), rc, ap]).cpu().numpy()
        return self._results(table, num_gt, res[0], res[1], res[2])

    def report(self, eval_result_list, group_by):
        report_dict = OrderedDict()
        for name, cond in group_by:
            cond_met_map = []
            for k, v in eval_result_list:
                if cond(k) and v['num_gt'] > 0:
                    cond_met_map.append(v['mAP'])
            cond_met_map = np.mean(cond_met_map)
            report_dict[name] = cond_met_map
        return report_dict


def _plain_table(rows):
    """Aligned plain text: terminaltables is not a dependency of this package."""
    rows = [[str(c) for c in r] for r in rows]
    width = [max(len(r[i]) for r in rows) for i in range(len(rows[0]))]
    line = '+' + '+'.join('-' * (w + 2) for w in width) + '+'
    text = [line, '| ' + ' | '.join(c.ljust(w) for c, w in zip(rows[0], width)) + ' |', line]
    text += ['| ' + ' | '.join(c.ljust(w) for c, w in zip(r, width)) + ' |' for r in rows[1:]]
    return '\n'.join(text + [line])


def _print_log(msg, logger=None):
    """mmcv.utils.print_log's cases: None prints, 'silent' drops, a Logger or a logger's name logs at INFO."""
    if logger is None:
        print(msg)
    elif isinstance(logger, logging.Logger):
        logger.info(msg)
    elif logger != 'silent':
        logging.getLogger(logger).info(msg)


def eval_map_flexible(det_results,
                      annotations,
                      match_thrs=[0.5],
                      breakdowns=[],
                      affinity_calculator=dict(type='LidarIOU3D'),
                      matcher=dict(type='MatcherCoCo'),
                      classes=None,
                      logger=None,
                      report_config=[
                          ('map', lambda x: x['breakdown'] == 'All')
                      ],
                      nproc=None,
                      frame_batch=0):
    assert len(det_results) == len(annotations)

    if nproc is None:
        nproc = 0

    fse = FlexibleStatisticsEval(classes, match_thrs, breakdowns, affinity_calculator, matcher, [], nproc)

    eval_result_list = fse.statistics_eval(det_results, annotations, frame_batch=frame_batch)
    report = fse.report(eval_result_list, report_config)

    table_data = [['Class', 'Breakdown', 'Thres', 'Dets', 'GTs', 'Recall', 'mAP']]
    for k, v in eval_result_list:
        table_data.append([k['class_name'], k['breakdown'], k['match_threshold'], v['num_det'], v['num_gt'],
                           f'{100 * v["recall"]:.3f}', f'{100 * v["mAP"]:.3f}'])
    _print_log('\n' + _plain_table(table_data), logger=logger)

    return report
