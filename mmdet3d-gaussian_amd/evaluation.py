"""Device-side counterparts of the reference's compiled evaluation helpers and of the two array stages of its
flexible mAP above them:

* ``trans_bev`` (and ``iou_3d`` / ``iou_bev`` in iou3d.py) — /root/reference/mmdet3d_gaussian/ops/eval/affinity.cpp:8-105
  as bound in ops/eval/eval_utils.cpp:26-36;
* ``match_coco`` — ops/eval/matcher.cpp:8-74;
* ``tp_records`` — core/evaluation/mean_ap_flexible.py:98-126, one matcher result as rows of a record buffer;
* ``ap_accumulate`` — mean_ap_flexible.py:130-148 with mmdet's average_precision(mode='area'), for every (group, threshold) of
  the buffer in one call (include/gd3d.h "Flexible mAP").

The evaluator that drives them with the reference's surface (FlexibleStatisticsEval, the breakdowns, the affinity and matcher
callables, eval_map_flexible) is eval_map.py.

The reference computes all of this on the CPU from numpy arrays.  Here the affinity matrix is produced and consumed in
HBM; numpy inputs are accepted and moved to the current device, results are returned as tensors on that device.
CPU tensors (and numpy inputs on a machine without a GPU) take the library's `_cpu` twins — the reference's own helpers are CPU code.
"""
import numpy as np
import torch

from . import _host
from .iou3d import iou_3d, iou_bev


def _dev_tensor(x, dtype, name, cpu_ok=False):
    """numpy arrays (what the reference's evaluation passes) go to the current GPU when there is one; torch tensors stay on
    their device.  What ends up on the CPU is legal only where a `_cpu` twin exists (`cpu_ok`)."""
    from_numpy = not isinstance(x, torch.Tensor)
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if not isinstance(x, torch.Tensor):
        x = torch.as_tensor(x)
    if not x.is_cuda:
        if from_numpy and torch.cuda.is_available():
            x = x.cuda()
        elif not cpu_ok:
            raise RuntimeError(f'{name}: this function has no CPU path' + ('' if torch.cuda.is_available() else ' and no GPU is visible'))
    return x.to(dtype).contiguous()


def trans_bev(det_bboxes, gt_bboxes):
    """(D,C>=2),(G,C'>=2) -> (D,G) distance between BEV centres (columns 0,1), affinity.cpp:83-105."""
    d = _dev_tensor(det_bboxes, torch.float32, 'trans_bev', cpu_ok=True)
    g = _dev_tensor(gt_bboxes, torch.float32, 'trans_bev', cpu_ok=True).to(d.device)
    if d.dim() != 2 or g.dim() != 2 or d.shape[1] < 2 or g.shape[1] < 2:
        raise RuntimeError(f'trans_bev: expected (D,>=2) and (G,>=2), got {tuple(d.shape)} and {tuple(g.shape)}')
    out = torch.empty((d.shape[0], g.shape[0]), dtype=torch.float32, device=d.device)
    # (the reference's own helper is CPU code, affinity.cpp:83-105: CPU tensors take the `_cpu` twin)
    _host.call('riou_eval_trans_bev', d.device, (d.data_ptr(), d.shape[0], d.shape[1], g.data_ptr(), g.shape[0], g.shape[1],
                                                 out.data_ptr()), (torch.get_num_threads(),))
    return out


def match_coco(cost_mat, cost_thrs, is_ignore, is_crowd):
    """(D,G) costs, (T) thresholds, (G) bool flags -> (T,D) int32 tensor: matched gt index or -1 (matcher.cpp:8-74)."""
    cost = _dev_tensor(cost_mat, torch.float32, 'match_coco', cpu_ok=True)
    if cost.dim() != 2:
        raise RuntimeError(f'match_coco: cost matrix must be 2-D, got {tuple(cost.shape)}')
    dev = cost.device
    thrs = _dev_tensor(cost_thrs, torch.float32, 'match_coco', cpu_ok=True).to(dev).reshape(-1)
    ign = _dev_tensor(is_ignore, torch.uint8, 'match_coco', cpu_ok=True).to(dev).reshape(-1)
    crowd = _dev_tensor(is_crowd, torch.uint8, 'match_coco', cpu_ok=True).to(dev).reshape(-1)
    D, G = cost.shape
    if ign.numel() != G or crowd.numel() != G:
        raise RuntimeError(f'match_coco: {G} gts but {ign.numel()} ignore / {crowd.numel()} crowd flags')
    T = thrs.numel()
    out = torch.empty((T, D), dtype=torch.int32, device=dev)
    # (the reference's matcher is CPU code, matcher.cpp:8-74: CPU tensors take the `_cpu` twin)
    _host.call('eval_match_coco', dev, (cost.data_ptr(), thrs.data_ptr(), ign.data_ptr(), crowd.data_ptr(), D, G, T, out.data_ptr()),
               (torch.get_num_threads(),))
    return out


MAX_THRS = 32    # one bit of tp_bits / msk_bits per threshold


def tp_records(matched, det_flag, gt_flag, score, group, num_thrs=None, out=None, row=0):
    """One matcher result as D records (mean_ap_flexible.py:115-126; `matched` None: the empty branch :98-104, no match at all).

    matched (T, D) int32 from `match_coco` or None (then `num_thrs` gives T); det_flag (D,) / gt_flag (G,) bool: the detection /
    the gt lies in the breakdown; score (D,) fp32; group: the record's group id.  Returns the four columns (group int32, score
    fp32, tp_bits, msk_bits: int32 words holding one bit per threshold) — fresh tensors, or rows [row, row + D) of the four
    columns given as `out`, which the one launch fills in place."""
    s = _dev_tensor(score, torch.float32, 'tp_records', cpu_ok=True).reshape(-1)
    dev = s.device
    D = s.numel()
    if matched is None:
        if num_thrs is None:
            raise RuntimeError('tp_records: without a matcher result the number of thresholds must be given')
        T, m = int(num_thrs), None
    else:
        m = _dev_tensor(matched, torch.int32, 'tp_records', cpu_ok=True).to(dev)
        if m.dim() != 2 or m.shape[1] != D:
            raise RuntimeError(f'tp_records: matched must be (T, {D}), got {tuple(m.shape)}')
        T = m.shape[0]
        if num_thrs is not None and int(num_thrs) != T:
            raise RuntimeError(f'tp_records: {T} matcher rows for {num_thrs} thresholds')
    if not 1 <= T <= MAX_THRS:
        raise RuntimeError(f'tp_records: {T} thresholds, expected 1..{MAX_THRS}')
    df = _dev_tensor(det_flag, torch.uint8, 'tp_records', cpu_ok=True).to(dev).reshape(-1)
    gf = _dev_tensor(gt_flag, torch.uint8, 'tp_records', cpu_ok=True).to(dev).reshape(-1)
    if df.numel() != D:
        raise RuntimeError(f'tp_records: {D} scores but {df.numel()} detection flags')
    if out is None:
        out = (torch.empty(D, dtype=torch.int32, device=dev), torch.empty(D, dtype=torch.float32, device=dev),
               torch.empty(D, dtype=torch.int32, device=dev), torch.empty(D, dtype=torch.int32, device=dev))
        row = 0
    cols = []
    for c, dt in zip(out, (torch.int32, torch.float32, torch.int32, torch.int32)):
        if c.dtype != dt or c.device != dev or c.dim() != 1 or not c.is_contiguous() or row < 0 or row + D > c.numel():
            raise RuntimeError(f'tp_records: every column of `out` must be a contiguous 1-D {dt} tensor on {dev} with rows '
                               f'[{row}, {row + D})')
        cols.append(c[row:row + D])
    _host.call('eval_tp_records', dev, (_host.ptr(m), df.data_ptr(), _host.ptr_or_null(gf), s.data_ptr(), int(group), D, gf.numel(), T,
                                        cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(), cols[3].data_ptr()))
    return tuple(cols)


_ap_workspace_bytes = _host.memo(lambda n, K, T: _lib_query('eval_ap_workspace_bytes', n, K, T))


def _lib_query(name, *args):
    from . import _lib
    return getattr(_lib.load(), name)(*args)


def ap_tile_rows():
    """Sorted rows per workgroup of the accumulate kernels (a compile-time capacity of the library)."""
    return _lib_query('eval_ap_tile_rows')


def ap_scan_chunk_tiles():
    """Tiles per trip of the carry scans between tiles: a loop, so no capacity — another trip every that many tiles."""
    return _lib_query('eval_ap_scan_chunk_tiles')


def ap_accumulate(group, score, tp_bits, msk_bits, num_gt, num_thrs):
    """(num_det (K, T) int64, recall (K, T) fp64, ap (K, T) fp64) of every (group, threshold) over n records: the definition in
    include/gd3d.h — rank order by descending score with ties in row order, rows of a group outside [0, K) count for nothing,
    ap = the exactly summed precision envelope over the true positives / max(num_gt, 1e-7).  K = len(num_gt).  One call, no
    read-back; the results stay on the records' device."""
    g = _dev_tensor(group, torch.int32, 'ap_accumulate', cpu_ok=True).reshape(-1)
    dev = g.device
    s = _dev_tensor(score, torch.float32, 'ap_accumulate', cpu_ok=True).to(dev).reshape(-1)
    tp = _dev_tensor(tp_bits, torch.int32, 'ap_accumulate', cpu_ok=True).to(dev).reshape(-1)
    mk = _dev_tensor(msk_bits, torch.int32, 'ap_accumulate', cpu_ok=True).to(dev).reshape(-1)
    ng = _dev_tensor(num_gt, torch.int64, 'ap_accumulate', cpu_ok=True).to(dev).reshape(-1)
    n, K, T = g.numel(), ng.numel(), int(num_thrs)
    if s.numel() != n or tp.numel() != n or mk.numel() != n:
        raise RuntimeError(f'ap_accumulate: columns of {n}, {s.numel()}, {tp.numel()} and {mk.numel()} rows')
    if not 1 <= T <= MAX_THRS:
        raise RuntimeError(f'ap_accumulate: {T} thresholds, expected 1..{MAX_THRS}')
    if not 1 <= K <= (1 << 20):
        raise RuntimeError(f'ap_accumulate: {K} groups, expected 1..{1 << 20}')
    num_det = torch.empty((K, T), dtype=torch.int64, device=dev)
    recall = torch.empty((K, T), dtype=torch.float64, device=dev)
    ap = torch.empty((K, T), dtype=torch.float64, device=dev)
    args = (_host.ptr_or_null(g), _host.ptr_or_null(s), _host.ptr_or_null(tp), _host.ptr_or_null(mk), ng.data_ptr(), n, K, T,
            num_det.data_ptr(), recall.data_ptr(), ap.data_ptr())
    if dev.type == 'cuda':
        ws = torch.empty(_ap_workspace_bytes(n, K, T), dtype=torch.uint8, device=dev)   # the caching allocator aligns to 512 bytes
        _host.call('eval_ap_accumulate', dev, args + (ws.data_ptr(),))
    else:
        _host.call('eval_ap_accumulate', dev, args, (torch.get_num_threads(),))
    return num_det, recall, ap
