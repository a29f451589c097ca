"""Cases, oracle and runners of `eval_frames_records` for tests/test_cpu_eval_frames.py and tests/test_gpu_eval_frames.py (not part of
the product).

* `build_cases`  — the case table: single problems at the edges of the matcher forms (G_p = 64 / 256 / 2048) and of the 32-row register
                   blocks and 64-detection stores (D_p = 32 / 64), and mixed batches of about 40 problems under one max_gt;
* `oracle`       — the COMPOSITION of the existing `_cpu` twins per problem: the affinity twin -> `match_coco` per breakdown row (all
                   thresholds) -> `tp_records` -> the alias copy; computed once per case and kept;
* `run_entry`    — the entry itself through ctypes, on host memory (the twin) or on device tensors, into the middle of poisoned
                   columns; the guard rows are checked here.
"""
import numpy as np
import torch

from mmdet3d_gaussian_amd import _lib, evaluation
from mmdet3d_gaussian_amd.iou3d import iou_3d, iou_bev

MODES = ('iou3d', 'ioubev', 'trans')
PAD = 5                                   # guard rows before and after the block of every column
POISON = (-77, -77.0, 0x5eadbeef, 0x5eadbeef)
DTYPES = (torch.int32, torch.float32, torch.int32, torch.int32)


def _boxes(rng, n, lim):
    return np.concatenate([rng.uniform(-lim, lim, (n, 2)), rng.uniform(-1.5, 0.5, (n, 1)), rng.uniform(1.2, 4.5, (n, 3)),
                           rng.uniform(-3.1, 3.1, (n, 1))], axis=1).astype(np.float32)


def _problem(rng, D, G, lim):
    """G gts (some duplicated: exact affinity ties) and D detections: jittered copies of gts, exact copies, and strays"""
    gt = _boxes(rng, G, lim)
    if G >= 2:
        dup = rng.integers(1, G, max(1, G // 8))
        gt[dup] = gt[dup - 1]
    det = _boxes(rng, D, lim)
    if G and D:
        near = rng.uniform(0, 1, D) < 0.7
        src = rng.integers(0, G, D)
        jitter = det.copy()
        jitter[:] = gt[src]
        jitter[:, :2] += rng.normal(0, 0.3, (D, 2)).astype(np.float32)
        jitter[:, 3:6] *= rng.uniform(0.9, 1.1, (D, 3)).astype(np.float32)
        exact = rng.uniform(0, 1, D) < 0.15
        jitter[exact] = gt[src[exact]]
        det[near] = jitter[near]
    return det, gt


def affinity(case, det, gt):
    """the existing twin of the case's mode on CPU tensors -> (D, G) fp32 numpy"""
    d, g = torch.from_numpy(np.ascontiguousarray(det)), torch.from_numpy(np.ascontiguousarray(gt))
    if case['mode'] == 'iou3d':
        return iou_3d(d, g, case['z_offset']).numpy()
    if case['mode'] == 'ioubev':
        return iou_bev(d, g).numpy()
    return evaluation.trans_bev(d, g).numpy()


def make_case(name, seed, sizes, R, T, mode, alias, crowd, group=None, lim=40.0, nan_det=False, thr_on_affinity=True):
    """sizes: [(D_p, G_p)].  group: None -> every row applies (distinct ids); or a (P, R) array with -1 entries."""
    rng = np.random.default_rng(seed)
    P = len(sizes)
    dets, gts = zip(*[_problem(rng, D, G, lim) for D, G in sizes]) if P else ((), ())
    det = np.concatenate(dets, axis=0) if P else np.zeros((0, 7), np.float32)
    gt = np.concatenate(gts, axis=0) if P else np.zeros((0, 7), np.float32)
    det_seg = np.concatenate([[0], np.cumsum([s[0] for s in sizes])]).astype(np.int32)
    gt_seg = np.concatenate([[0], np.cumsum([s[1] for s in sizes])]).astype(np.int32)
    ND, NG = len(det), len(gt)
    score = np.round(rng.uniform(0, 1, ND), 2).astype(np.float32)
    for p in range(P):
        score[det_seg[p]:det_seg[p + 1]] = -np.sort(-score[det_seg[p]:det_seg[p + 1]])
    if nan_det and ND:
        case_nan = rng.integers(0, ND, max(1, ND // 16))
        det[case_nan, rng.integers(0, 2)] = np.nan          # a centre coordinate: the detection can match nothing
    det_flag = (rng.uniform(0, 1, (R, ND)) < 0.7).astype(np.uint8)
    gt_flag = (rng.uniform(0, 1, (R, NG)) < 0.7).astype(np.uint8) * np.uint8(3)       # any non-zero byte is a set flag
    det_flag[0], gt_flag[0] = 1, (rng.uniform(0, 1, NG) < 0.85)                        # row 0 is 'All': ignored gts cleared
    if group is None:
        group = np.arange(P * R, dtype=np.int32).reshape(P, R) if P else np.zeros((0, R), np.int32)
    if mode == 'trans':
        thrs = np.array([0.5, 2.0][:T], np.float32) if T <= 2 else np.linspace(0.1, 6.0, T).astype(np.float32)
    else:
        thrs = np.array([0.5, 0.7][:T], np.float32) if T <= 2 else np.linspace(0.02, 0.95, T).astype(np.float32)
    case = dict(name=name, mode=mode, z_offset=0.5 if seed % 2 else 0.0, negate=mode != 'trans', det=det, score=score, det_seg=det_seg, gt=gt,
                gt_seg=gt_seg, gt_crowd=(rng.uniform(0, 1, NG) < 0.2).astype(np.uint8) if crowd else None, det_flag=det_flag, gt_flag=gt_flag,
                group=np.ascontiguousarray(group, dtype=np.int32), thrs=thrs, P=P, R=R, T=T, alias=int(alias), sizes=list(sizes),
                nan_rows=case_nan if nan_det and ND else np.zeros(0, np.int64))
    if thr_on_affinity:
        # the last threshold becomes an affinity that occurs in the largest problem (`<=` is inclusive)
        live = [p for p in range(P) if sizes[p][0] and sizes[p][1]]
        if live:
            p = max(live, key=lambda q: sizes[q][0] * sizes[q][1])
            a = affinity(case, det[det_seg[p]:det_seg[p + 1]], gt[gt_seg[p]:gt_seg[p + 1]])
            ok = a[np.isfinite(a) & (a > (0.05 if case['negate'] else 0.0)) & (a < (0.999 if case['negate'] else 8.0))]
            if ok.size:
                case['thrs'][-1] = np.sort(ok)[ok.size // 2]
                case['thr_hits'] = int((a == case['thrs'][-1]).sum())
    pair_off = np.zeros(P + 1, np.int64)
    np.cumsum([d * g for d, g in sizes], out=pair_off[1:])
    case['pair_off'], case['max_gt'] = pair_off, max([g for _, g in sizes], default=0)
    return case


def _mixed_sizes(rng, d_set, g_set, big=()):
    """about 40 problems; empty ones first, last and adjacent; `big`: (D, G) problems placed in the middle"""
    body = [(int(rng.choice(d_set)), int(rng.choice(g_set))) for _ in range(32)]
    body[5:5] = [(0, 3), (0, 0), (7, 0)]
    body[20:20] = list(big)
    return [(0, 0), (0, 4)] + body + [(9, 0), (0, 0)]


def _mixed_group(rng, P, R):
    """-1 entries: a whole problem, the LAST row of some problems (b_last < R - 1), a middle row of others"""
    g = np.arange(P * R, dtype=np.int32).reshape(P, R)
    g[3::9] = -1
    g[4::5, R - 1] = -1
    g[6::7, 1] = -1
    g[8::11, R - 2:] = -1
    return g


def build_cases():
    D_SET, cases = [0, 1, 31, 32, 33, 63, 64, 65, 129], []
    singles = [(0, 0), (1, 0), (0, 5), (1, 1), (31, 63), (32, 64), (33, 65), (129, 10), (63, 255), (64, 256), (65, 257), (129, 256), (65, 2047),
               (64, 2048), (129, 64), (33, 1)]
    for k, (D, G) in enumerate(singles):
        R = 4 if k % 2 else 1
        group = None
        if R == 4 and k % 4 == 3:
            group = np.array([[7, -1, 3, -1]], np.int32)                 # the last row does not apply: b_last = 2
        cases.append(make_case(f'single_D{D}_G{G}', 100 + k, [(D, G)], R, (1, 2, 32)[k % 3], MODES[k % 3], alias=k % 2 == 1 or k % 4 == 0,
                               crowd=k % 3 == 1, group=group, nan_det=k % 5 == 2))
    cases.append(make_case('single_whole_problem_off', 150, [(33, 9)], 4, 2, 'iou3d', True, False, group=np.full((1, 4), -1, np.int32)))
    cases.append(make_case('no_problem', 151, [], 4, 2, 'ioubev', True, False))
    rng = np.random.default_rng(77)
    n = 0
    for form, (g_set, big) in enumerate((([0, 1, 10, 63, 64], ()), ([0, 1, 63, 64, 65, 255, 256], ()),
                                         ([0, 1, 64, 65, 256, 257], ((65, 2047), (33, 2048), (1, 257))))):
        for mode in MODES:
            for R, T, alias in ((4, 2, True), (1, 32, False)) if mode == 'iou3d' else ((4, (2, 1, 32)[form], form != 1),):
                sizes = _mixed_sizes(rng, D_SET, g_set, big)
                group = _mixed_group(rng, len(sizes), R) if R == 4 else None
                cases.append(make_case(f'mixed_form{form}_{mode}_R{R}_T{T}', 200 + n, sizes, R, T, mode, alias, crowd=n % 2 == 0, group=group,
                                       nan_det=n % 3 == 0))
                n += 1
    for c in cases:     # the conditions the table is built for
        assert c['max_gt'] <= 2048
    forms = {0 if c['max_gt'] <= 64 else 1 if c['max_gt'] <= 256 else 2 for c in cases if c['name'].startswith('mixed')}
    assert forms == {0, 1, 2}
    assert any(c.get('thr_hits', 0) > 0 for c in cases)
    return cases


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


def oracle(case):
    """the four columns (R * ND rows) from the existing twins, problem by problem"""
    if 'want' in case:
        return case['want']
    ND, R, T = len(case['det']), case['R'], case['T']
    cols = (np.full(R * ND, -1, np.int32), np.zeros(R * ND, np.float32), np.zeros(R * ND, np.int32), np.zeros(R * ND, np.int32))
    thrs = -case['thrs'] if case['negate'] else case['thrs']
    for p in range(case['P']):
        ds, de, gs, ge = case['det_seg'][p], case['det_seg'][p + 1], case['gt_seg'][p], case['gt_seg'][p + 1]
        D, G = de - ds, ge - gs
        if D == 0:
            continue
        cost = None
        if G > 0:
            cost = affinity(case, case['det'][ds:de], case['gt'][gs:ge])
            cost = -cost if case['negate'] else cost
        crowd = case['gt_crowd'][gs:ge] if case['gt_crowd'] is not None else np.zeros(G, np.uint8)
        applies = [b for b in range(R) if case['group'][p, b] >= 0]
        for b in range(R):
            sl = slice(b * ND + ds, b * ND + de)
            if case['group'][p, b] < 0:
                cols[1][sl] = case['score'][ds:de]
                continue
            gf = case['gt_flag'][b, gs:ge]
            matched = None if cost is None else evaluation.match_coco(torch.from_numpy(cost), torch.from_numpy(thrs), torch.from_numpy(gf == 0),
                                                                      torch.from_numpy(crowd))
            got = evaluation.tp_records(matched, torch.from_numpy(case['det_flag'][b, ds:de]), torch.from_numpy(gf),
                                        torch.from_numpy(case['score'][ds:de]), int(case['group'][p, b]), num_thrs=T)
            for c, g in zip(cols, got):
                c[sl] = g.numpy()
        if case['alias'] and applies:
            last = applies[-1]
            for b in applies[:-1]:
                cols[2][b * ND + ds:b * ND + de] = cols[2][last * ND + ds:last * ND + de]
    case['want'] = cols
    return cols


# ---- the entry through ctypes ---------------------------------------------------------------------------------------------------------

INPUTS = ('det', 'score', 'det_seg', 'gt', 'gt_seg', 'gt_crowd', 'pair_off', 'det_flag', 'gt_flag', 'group', 'thrs')


def to_device(case, device):
    """the case's arrays as tensors on `device` (gt_crowd may be None)"""
    return {k: None if case[k] is None else torch.from_numpy(np.ascontiguousarray(case[k])).to(device) for k in INPUTS}


def fresh_columns(rows, device):
    return [torch.full((rows + 2 * PAD,), v, dtype=dt, device=device) for v, dt in zip(POISON, DTYPES)]


def _p(t):
    return None if t is None or t.numel() == 0 else t.data_ptr()


def entry_args(case, ten, cols):
    ND, NG = len(case['det']), len(case['gt'])
    outs = [c[PAD:].data_ptr() if ND else None for c in cols]
    return (evaluation.FRAMES_MODES[case['mode']], case['z_offset'], int(case['negate']), _p(ten['det']), _p(ten['score']), ten['det_seg'].data_ptr(),
            ND, _p(ten['gt']), ten['gt_seg'].data_ptr(), NG, _p(ten['gt_crowd']), ten['pair_off'].data_ptr(), int(case['pair_off'][-1]),
            case['max_gt'], _p(ten['det_flag']), _p(ten['gt_flag']), ten['group'].data_ptr() if case['P'] else ten['det_seg'].data_ptr(),
            ten['thrs'].data_ptr(), case['P'], case['R'], case['T'], case['alias'], *outs)


def workspace_bytes(case):
    return _lib.load().eval_frames_workspace_bytes(len(case['det']), int(case['pair_off'][-1]), case['R'], case['T'])


def launch(case, ten, cols, ws=None, stream=None, nthreads=3):
    """one call of the entry: the device entry when `ws` is given, else the twin; returns the return code"""
    lib = _lib.load()
    args = entry_args(case, ten, cols)
    if ws is not None:
        return lib.eval_frames_records(*args, ws.data_ptr(), stream if stream is not None else torch.cuda.current_stream().cuda_stream)
    return lib.eval_frames_records_cpu(*args, nthreads)


def check_columns(case, cols, what=''):
    """the block equals the oracle bit for bit and the guard rows still hold the poison"""
    rows = case['R'] * len(case['det'])
    want = oracle(case)
    for k, (c, w, poison) in enumerate(zip(cols, want, POISON)):
        got = c.cpu().numpy()
        guard = np.concatenate([got[:PAD], got[PAD + rows:]])
        assert (guard == np.asarray(poison, got.dtype)).all(), (case['name'], what, 'guard rows of column', k)
        assert got.size == rows + 2 * PAD
        bad = np.nonzero(bits(got[PAD:PAD + rows]) != bits(w))[0]
        assert bad.size == 0, (case['name'], what, 'column', k, 'rows', bad[:8], got[PAD:PAD + rows][bad[:8]], w[bad[:8]])


def run_entry(case, device, nthreads=3):
    """-> the poisoned columns after one call on `device` ('cpu': the twin)"""
    ten = to_device(case, device)
    cols = fresh_columns(case['R'] * len(case['det']), device)
    if device == 'cpu':
        rc = launch(case, ten, cols, nthreads=nthreads)
    else:
        ws = torch.empty(max(256, workspace_bytes(case)), dtype=torch.uint8, device=device)
        rc = launch(case, ten, cols, ws=ws)
        torch.cuda.synchronize()
    assert rc == 0, (case['name'], rc)
    return cols
