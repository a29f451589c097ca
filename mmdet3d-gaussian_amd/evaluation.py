"""Device-side counterparts of the reference's compiled evaluation helpers and of the two array stages of its
flexible mAP above them:

* ``trans_bev`` (and ``iou_3d`` / ``iou_bev`` in iou3d.py) — /root/reference/mmdet3d_gaussian/ops/eval/affinity.cpp:8-105
  as bound in ops/eval/eval_utils.cpp:26-36;
* ``match_coco`` — ops/eval/matcher.cpp:8-74;
* ``tp_records`` — core/evaluation/mean_ap_flexible.py:98-126, one matcher result as rows of a record buffer;
* ``ap_accumulate`` — mean_ap_flexible.py:130-148 with mmdet's average_precision(mode='area'), for every (group, threshold) of
  the buffer in one call (include/gd3d.h "Flexible mAP").;
* ``frames_records`` — mean_ap_flexible.py:37-126 for every (frame, class) problem, breakdown row and threshold of a BATCH of frames in
  three launches: affinities, matcher and records, the same bits as the three calls above per problem.

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


FRAMES_MODES = {'iou3d': 0, 'ioubev': 1, 'trans': 2}
FRAMES_MAX_GT = 2048     # gts of one problem; beyond it eval_frames_records answers GD3D_E_TOOLARGE

_frames_workspace_bytes = _host.memo(lambda ND, pairs, R, T: _lib_query('eval_frames_workspace_bytes', ND, pairs, R, T))


def _host_table(x, dtype):
    """A small table whose contents the host knows (segment bounds, groups): a contiguous numpy array."""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(x), dtype=dtype)


def frames_records(det, score, det_seg, gt, gt_seg, det_flag, gt_flag, group, thrs, mode, z_offset=0.5, negate=None, gt_crowd=None,
                   alias_tp=True, out=None, row=0):
    """Every record of a batch of frames in a fixed number of launches (include/gd3d.h "Flexible mAP, a batch of frames").

    A problem is one (frame, class) pair.  Problem p owns rows [det_seg[p], det_seg[p+1]) of det (ND, 7) and score (ND,), already in
    the problem's rank order, and rows [gt_seg[p], gt_seg[p+1]) of gt (NG, 7).  det_flag (R, ND) / gt_flag (R, NG) bool: the box lies
    in breakdown row b (ignored gts cleared); group (P, R): the record group of problem p's row b, -1 where the row does not apply;
    thrs (T,) fp32; mode 'iou3d' (with z_offset) | 'ioubev' | 'trans'; negate (default: True for the two IoUs) hands the matcher
    -affinity and -thrs; gt_crowd (NG,) bool or None.  det_seg, gt_seg and group are host tables (lists, numpy, CPU tensors).

    Returns the four columns (group int32, score fp32, tp_bits, msk_bits) of R * ND rows, the row of (b, i) at b * ND + i — fresh
    tensors, or rows [row, row + R * ND) of the four columns given as `out`.  What `tp_records` gives for `match_coco` on the
    problem's affinity, per problem and row, bit for bit; alias_tp: every applicable row of a problem carries the tp bits of the
    problem's last applicable row (the reference's one-array aliasing).  CPU tensors take the `_cpu` twin."""
    d = _dev_tensor(det, torch.float32, 'frames_records', cpu_ok=True)
    dev = d.device
    s = _dev_tensor(score, torch.float32, 'frames_records', cpu_ok=True).to(dev).reshape(-1)
    g = _dev_tensor(gt, torch.float32, 'frames_records', cpu_ok=True).to(dev)
    df = _dev_tensor(det_flag, torch.uint8, 'frames_records', cpu_ok=True).to(dev)
    gf = _dev_tensor(gt_flag, torch.uint8, 'frames_records', cpu_ok=True).to(dev)
    th = _dev_tensor(thrs, torch.float32, 'frames_records', cpu_ok=True).to(dev).reshape(-1)
    if mode not in FRAMES_MODES:
        raise RuntimeError(f'frames_records: mode must be one of {sorted(FRAMES_MODES)}, got {mode!r}')
    dseg, gseg = _host_table(det_seg, np.int64).reshape(-1), _host_table(gt_seg, np.int64).reshape(-1)
    grp = _host_table(group, np.int32)
    ND, NG, T = s.numel(), g.shape[0] if g.dim() == 2 else -1, th.numel()
    P = dseg.size - 1
    if d.dim() != 2 or d.shape != (ND, 7) or g.dim() != 2 or g.shape[1] != 7:
        raise RuntimeError(f'frames_records: expected det ({ND}, 7) and gt (NG, 7), got {tuple(d.shape)} and {tuple(g.shape)}')
    if P < 0 or gseg.size != P + 1 or grp.ndim != 2 or grp.shape[0] != P or grp.shape[1] < 1:
        raise RuntimeError(f'frames_records: det_seg ({dseg.size},), gt_seg ({gseg.size},) and group {grp.shape} do not describe one set of problems')
    R = grp.shape[1]
    D_p, G_p = np.diff(dseg), np.diff(gseg)
    if dseg[0] != 0 or gseg[0] != 0 or dseg[-1] != ND or gseg[-1] != NG or (D_p < 0).any() or (G_p < 0).any():
        raise RuntimeError(f'frames_records: the segment tables must ascend from 0 to {ND} detections and {NG} gts')
    if df.shape != (R, ND) or gf.shape != (R, NG):
        raise RuntimeError(f'frames_records: flags must be ({R}, {ND}) and ({R}, {NG}), got {tuple(df.shape)} and {tuple(gf.shape)}')
    if not 1 <= T <= MAX_THRS:
        raise RuntimeError(f'frames_records: {T} thresholds, expected 1..{MAX_THRS}')
    crowd = None
    if gt_crowd is not None:
        crowd = _dev_tensor(gt_crowd, torch.uint8, 'frames_records', cpu_ok=True).to(dev).reshape(-1)
        if crowd.numel() != NG:
            raise RuntimeError(f'frames_records: {NG} gts but {crowd.numel()} crowd flags')
    pair_off = np.zeros(P + 1, np.int64)
    np.cumsum(D_p * G_p, out=pair_off[1:])
    pairs, max_gt = int(pair_off[-1]), int(G_p.max()) if P else 0
    rows = R * ND
    if out is None:
        out = (torch.empty(rows, dtype=torch.int32, device=dev), torch.empty(rows, dtype=torch.float32, device=dev),
               torch.empty(rows, dtype=torch.int32, device=dev), torch.empty(rows, dtype=torch.int32, device=dev))
        row = 0
    cols = []
    for c, dt in zip(out, (torch.int32, torch.float32, torch.int32, torch.int32)):
        if c.dtype != dt or c.device != dev or c.dim() != 1 or not c.is_contiguous() or row < 0 or row + rows > c.numel():
            raise RuntimeError(f'frames_records: every column of `out` must be a contiguous 1-D {dt} tensor on {dev} with rows '
                               f'[{row}, {row + rows})')
        cols.append(c[row:row + rows])
    # the small tables: built on the host from shapes, one packed copy per call
    table = np.concatenate([pair_off.view(np.int32), dseg.astype(np.int32), gseg.astype(np.int32), grp.reshape(-1)])
    tab = torch.from_numpy(table).to(dev)
    p_off = tab.data_ptr()                    # int64 words first: 8-byte aligned
    p_dseg = p_off + 8 * (P + 1)
    p_gseg = p_dseg + 4 * (P + 1)
    p_grp = p_gseg + 4 * (P + 1)
    neg = FRAMES_MODES[mode] != 2 if negate is None else bool(negate)
    args = (FRAMES_MODES[mode], float(z_offset), int(neg), _host.ptr_or_null(d), _host.ptr_or_null(s), p_dseg, ND, _host.ptr_or_null(g), p_gseg,
            NG, _host.ptr(crowd), p_off, pairs, max_gt, _host.ptr_or_null(df), _host.ptr_or_null(gf), p_grp, th.data_ptr(), P, R, T,
            int(bool(alias_tp)), _host.ptr_or_null(cols[0]), _host.ptr_or_null(cols[1]), _host.ptr_or_null(cols[2]), _host.ptr_or_null(cols[3]))
    if dev.type == 'cuda':
        ws = torch.empty(_frames_workspace_bytes(ND, pairs, R, T) or 256, dtype=torch.uint8, device=dev)   # the allocator aligns to 512 bytes
        _host.call('eval_frames_records', dev, args + (ws.data_ptr(),))
    else:
        _host.call('eval_frames_records', dev, args, (torch.get_num_threads(),))
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
