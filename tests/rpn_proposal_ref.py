"""TEST INFRASTRUCTURE: a numpy float32 restatement of the RPN proposal stage as include/gd3d.h spells it out (gd3d_rpn_proposals:
mmdet3d's PartA2RPNHead.get_bboxes_single + class_agnostic_nms, third party, restated) and of fx_expf (csrc/fx_exp.h), one numpy
operation per fp32 operation of the header's sequence, so the bits are the compiled twin's.  The NMS is a plain greedy loop: over
this package's CPU pairwise IoU (`boxes_iou_bev`) when rotated, over a numpy restatement of the axis-aligned IoU otherwise.  Also
the named cases tests/test_cpu_rpn_proposal.py and tests/test_gpu_rpn_proposal.py share."""
import numpy as np
import torch

f32 = np.float32
PI = f32(3.14159265358979323846)
KEYS = ('boxes_3d', 'scores_3d', 'labels_3d', 'cls_preds', 'rois', 'batch_cnt', 'cand_inds', 'cand_cnt')
HI_CUT, LO_CUT = f32(88.72283172607422), f32(-87.33654022216797)      # 0x42b17217, 0xc2aeac4f


def fx_expf(x):
    x = np.asarray(x, f32)
    with np.errstate(all='ignore'):
        ln2_hi, ln2_lo, inv_ln2 = f32(6.9313812256e-01), f32(9.0580006145e-06), f32(1.4426950216e+00)
        p1, p2 = f32(1.6666625440e-01), f32(-2.7667332906e-03)
        nan, big, small = x != x, x > HI_CUT, x < LO_CUT
        xs = np.where(nan | big | small, f32(0), x)
        k = (inv_ln2 * xs + np.where(xs < 0, f32(-0.5), f32(0.5))).astype(np.int32)       # truncation
        kf = k.astype(f32)
        hi = xs - kf * ln2_hi
        lo = kf * ln2_lo
        r = hi - lo
        t = r * r
        c = r - t * (p1 + t * p2)
        y = f32(1.0) + (hi - (lo - (r * c) / (f32(2.0) - c)))
        yb = y.view(np.uint32)
        e = ((yb >> np.uint32(23)).astype(np.int32) & 255) + k
        out = (yb.astype(np.int64) + (k.astype(np.int64) << 23)).astype(np.uint32).view(f32)
        out = np.where(e <= 0, f32(0), out)
        out = np.where((e >= 255) | big, f32(np.inf), out)
        out = np.where(small, f32(0), out)
        out = np.where(nan, x, out)
    return out.astype(f32)


def fx_expf_sample():
    """the sample csrc/fx_exp.h documents: 2^20 uniform arguments over the finite-result range, every integer multiple of ln 2 / 2
    in range +- 4 neighbours, 4096 values either side of 0"""
    rng = np.random.default_rng(0)
    tiny, big = np.float64(np.finfo(f32).tiny), np.float64(np.finfo(f32).max)
    x = rng.uniform(np.log(tiny), np.log(big), 1 << 20).astype(f32)
    m = (np.arange(-260, 260, dtype=np.float64) * (np.log(2.0) / 2)).astype(f32)
    parts, up, dn = [x, m], m.copy(), m.copy()
    for _ in range(4):
        up, dn = np.nextafter(up, f32(np.inf)), np.nextafter(dn, f32(-np.inf))
        parts += [up.copy(), dn.copy()]
    z = np.arange(1, 4097, dtype=np.uint32).view(f32)
    x = np.concatenate(parts + [z, -z, f32([0.0, -0.0])])
    want = np.exp(x.astype(np.float64))
    return x[(want >= tiny) & (want <= big)]


def sigmoid(x):
    with np.errstate(all='ignore'):
        return (f32(1.0) / (f32(1.0) + fx_expf(-np.asarray(x, f32)))).astype(f32)


def key_of(v):
    u = np.asarray(v, f32).view(np.uint32).copy()
    u[u == np.uint32(0x80000000)] = 0
    neg = (u & np.uint32(0x80000000)) != 0
    return np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def decode(an, t):
    with np.errstate(all='ignore'):
        xa, ya, za, wa, la, ha, ra = (an[:, j] for j in range(7))
        za = za + ha / f32(2.0)
        diagonal = np.sqrt(la * la + wa * wa)
        xg = t[:, 0] * diagonal + xa
        yg = t[:, 1] * diagonal + ya
        zg = t[:, 2] * ha + za
        lg = fx_expf(t[:, 4]) * la
        wg = fx_expf(t[:, 3]) * wa
        hg = fx_expf(t[:, 5]) * ha
        rg = t[:, 6] + ra
        zg = zg - hg / f32(2.0)
        box = np.stack([xg, yg, zg, wg, lg, hg, rg], 1).astype(f32)
        hw, hl = wg / f32(2.0), lg / f32(2.0)
        bev = np.stack([xg - hw, yg - hl, xg + hw, yg + hl, rg], 1).astype(f32)
    return box, bev


def dir_fix(yaw, d, dir_offset, dir_limit_offset):
    val = yaw - f32(dir_offset)
    dir_rot = val - np.floor(val / PI + f32(dir_limit_offset)) * PI
    return (dir_rot + f32(dir_offset) + PI * d.astype(f32)).astype(f32)


def _iou_normal(a, b):
    left, right = max(a[0], b[0]), min(a[2], b[2])
    top, bottom = max(a[1], b[1]), min(a[3], b[3])
    width, height = max(right - left, f32(0)), max(bottom - top, f32(0))
    inter = f32(width * height)
    sa, sb = f32((a[2] - a[0]) * (a[3] - a[1])), f32((b[2] - b[0]) * (b[3] - b[1]))
    return f32(inter / max(f32(f32(sa + sb) - inter), f32(1e-8)))


def greedy_nms(bev, thr, rotate):
    """kept positions of the score-ordered (n, 5) rows: box i is kept iff no kept j < i has IoU(j, i) > thr"""
    n = len(bev)
    if n == 0:
        return np.zeros((0,), np.int64)
    thr = f32(thr)
    if rotate:
        import mmdet3d_gaussian_amd as amd
        t = torch.from_numpy(np.ascontiguousarray(bev))
        iou = amd.boxes_iou_bev(t, t).numpy()
    keep = []
    for i in range(n):
        if rotate:
            dead = any(iou[j, i] > thr for j in keep)
        else:
            dead = any(_iou_normal(bev[j], bev[i]) > thr for j in keep)
        if not dead:
            keep.append(i)
    return np.asarray(keep, np.int64)


def anchor_rows(x, per):
    """(B, A*per, H, W) -> (B, N, per), anchor n = (h W + w) A + a, channel a per + k"""
    B, ch, H, W = x.shape
    A = ch // per
    return x.reshape(B, A, per, H * W).transpose(0, 3, 1, 2).reshape(B, H * W * A, per)


def select(logits, cap):
    """logits (N, C) -> (candidate anchor indices in the selection order, their best logit, their label)"""
    nan = np.isnan(logits).any(1)
    safe = np.where(nan[:, None], f32(0), logits)
    best = safe.max(1)
    label = safe.argmax(1)                      # the first maximum: the lowest class
    key = key_of(best).astype(np.int64)
    valid = np.nonzero(~nan)[0]
    order = valid[np.argsort(-key[valid], kind='stable')][:cap]
    return order, best[order], label[order]


def expected(cls, bbox, dirp, anchors, cfg, C, dir_offset=0.7854, dir_limit_offset=0.0, nms=greedy_nms):
    B, AC, H, W = cls.shape
    A, N = AC // C, H * W * AC // C
    cap = cfg['nms_pre'] if 0 < cfg['nms_pre'] < N else N
    M = min(cfg['nms_post'], cfg['max_num'])
    L, T, D = anchor_rows(cls, C), anchor_rows(bbox, 7), anchor_rows(dirp, 2)
    anchors = anchors.reshape(N, 7)
    out = dict(boxes_3d=np.zeros((B * M, 7), f32), scores_3d=np.zeros((B * M,), f32), labels_3d=np.full((B * M,), -1, np.int64),
               cls_preds=np.zeros((B * M, C), f32), rois=np.zeros((B * M, 8), f32), batch_cnt=np.zeros((B,), np.int32),
               cand_inds=np.full((B, cap), -1, np.int64), cand_cnt=np.zeros((B,), np.int32))
    out['rois'][:, 0] = -1
    row = 0
    for b in range(B):
        sel, best, label = select(L[b], cap)
        out['cand_inds'][b, :len(sel)] = sel
        score = sigmoid(best)
        d = (D[b][sel, 1] > D[b][sel, 0]).astype(np.int32)
        box, bev = decode(anchors[sel], T[b][sel])
        cnt = int((score > f32(cfg['score_thr'])).sum())
        out['cand_cnt'][b] = cnt
        keep = nms(bev[:cnt], cfg['nms_thr'], cfg['use_rotate_nms'])[:M]
        m = len(keep)
        out['batch_cnt'][b] = m
        kb = box[keep].copy()
        if m:
            kb[:, 6] = dir_fix(kb[:, 6], d[keep], dir_offset, dir_limit_offset)
        out['boxes_3d'][row:row + m] = kb
        out['scores_3d'][row:row + m] = score[keep]
        out['labels_3d'][row:row + m] = label[keep]
        out['cls_preds'][row:row + m] = sigmoid(L[b][sel[keep]])
        out['rois'][row:row + m, 0] = b
        out['rois'][row:row + m, 1:] = kb
        row += m
    return out


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def make_anchors(H, W, A, pitch=0.8):
    """(H W A, 7): a BEV grid of the KITTI sizes in two rotations, cycled over the A anchors of a cell"""
    sizes = f32([[1.6, 3.9, 1.56], [0.6, 0.8, 1.73], [0.6, 1.76, 1.73]])
    an = np.zeros((H, W, A, 7), f32)
    an[..., 0] = (np.arange(W, dtype=f32) * f32(pitch))[None, :, None]
    an[..., 1] = (np.arange(H, dtype=f32) * f32(pitch) - f32(H * pitch / 2))[:, None, None]
    for a in range(A):
        an[:, :, a, 2] = f32(-1.78) if (a // 2) % 3 == 0 else f32(-0.6)
        an[:, :, a, 3:6] = sizes[(a // 2) % 3]
        an[:, :, a, 6] = f32(0.0) if a % 2 == 0 else f32(1.57)
    return an.reshape(-1, 7)


def make_inputs(seed, B, H, W, A, C, pitch=0.8, delta=0.3):
    rng = np.random.default_rng(seed)
    cls = rng.normal(0, 1.5, (B, A * C, H, W)).astype(f32)
    bbox = (rng.normal(0, delta, (B, A * 7, H, W))).astype(f32)
    dirp = rng.normal(0, 1, (B, A * 2, H, W)).astype(f32)
    return dict(cls=cls, bbox=bbox, dirp=dirp, anchors=make_anchors(H, W, A, pitch), C=C)


def cfg_of(nms_pre, nms_post=100, max_num=100, nms_thr=0.7, score_thr=0.3, rotate=True):
    return dict(nms_pre=nms_pre, nms_post=nms_post, max_num=max_num, nms_thr=nms_thr, score_thr=score_thr, use_rotate_nms=rotate)


def _set_anchor(x, per, b, n, A, W, values):
    """the `per` channels of anchor n of sample b"""
    cell, a = divmod(n, A)
    for k, v in enumerate(values):
        x[b, a * per + k, cell // W, cell % W] = v


def _case_ties():
    """six anchors share the k-th key; nms_pre takes three of them: the three lowest indices (both samples carry the same class map,
    so one nms_pre cuts inside the group in both; their boxes differ)"""
    c = make_inputs(11, 2, 8, 11, 6, 3)
    c['cls'][1] = c['cls'][0]
    N = 8 * 11 * 6
    group = [17, 100, 101, 260, 400, 527]
    for b in range(2):
        for n in group:
            _set_anchor(c['cls'], 3, b, n, 6, 11, [f32(0.25), f32(-1.0), f32(0.25) if n == 101 else f32(-2.0)])
    best = anchor_rows(c['cls'], 3)[0].max(1)
    above = int((best > f32(0.25)).sum())
    c.update(cfg=cfg_of(above + 3, 60, 80), note=dict(group=group, above=above))
    assert N > above + 6
    return c


def _case_equal_class_and_dir():
    """the best anchors carry an equal class maximum (lowest class wins) and equal direction logits (bin 0)"""
    c = make_inputs(12, 1, 5, 7, 6, 3)
    for i, n in enumerate([3, 50, 121, 209]):
        _set_anchor(c['cls'], 3, 0, n, 6, 7, [f32(-1.0), f32(6.0 + i), f32(6.0 + i)])
        _set_anchor(c['dirp'], 2, 0, n, 6, 7, [f32(0.5), f32(0.5)])
    c.update(cfg=cfg_of(100, 50, 40, nms_thr=0.1), note=dict(anchors=[3, 50, 121, 209]))
    return c


def _case_empty_sample():
    """B = 3, the middle sample entirely under the threshold: count 0, the last sample packed right behind the first"""
    c = make_inputs(13, 3, 5, 7, 6, 3)
    c['cls'][1] = -f32(2.0) - np.abs(c['cls'][1])
    c.update(cfg=cfg_of(150, 30, 30))
    return c


def _case_nan():
    c = make_inputs(14, 2, 5, 7, 6, 3)
    _set_anchor(c['cls'], 3, 0, 77, 6, 7, [f32(9.0), f32(np.nan), f32(1.0)])
    _set_anchor(c['cls'], 3, 1, 5, 6, 7, [f32(np.nan), f32(np.nan), f32(np.nan)])
    c.update(cfg=cfg_of(0, 64, 64), note=dict(nan=[(0, 77), (1, 5)]))
    return c


def _simple(seed, B, H, W, A, C, cfg, **kw):
    def build():
        c = make_inputs(seed, B, H, W, A, C)
        c.update(cfg=dict(cfg), **kw)
        return c
    return build


N57, N811 = 5 * 7 * 6, 8 * 11 * 6
BUILDERS = {
    'pre_N_minus_1': _simple(1, 2, 5, 7, 6, 3, cfg_of(N57 - 1)),
    'pre_N': _simple(2, 2, 5, 7, 6, 3, cfg_of(N57)),
    'pre_N_plus_1': _simple(3, 2, 5, 7, 6, 3, cfg_of(N57 + 1)),
    'pre_0': _simple(4, 2, 5, 7, 6, 3, cfg_of(0)),
    'pre_minus_1': _simple(5, 2, 5, 7, 6, 3, cfg_of(-1)),
    'ties_at_the_boundary': _case_ties,
    'equal_class_and_dir': _case_equal_class_and_dir,
    'axis_aligned_nms': _simple(6, 2, 8, 11, 6, 3, cfg_of(300, 80, 90, nms_thr=0.5, rotate=False)),
    'rotated_nms': _simple(6, 2, 8, 11, 6, 3, cfg_of(300, 80, 90, nms_thr=0.5, rotate=True)),
    'post_below_max_more_kept_than_M': _simple(7, 2, 8, 11, 6, 3, cfg_of(400, 12, 40, nms_thr=0.8)),
    'post_above_max_more_kept_than_M': _simple(8, 2, 8, 11, 6, 3, cfg_of(400, 40, 9, nms_thr=0.8)),
    'fewer_kept_than_M': _simple(9, 2, 5, 7, 6, 3, cfg_of(0, 500, 400, nms_thr=0.01, score_thr=0.9)),
    'empty_middle_sample': _case_empty_sample,
    'nan_logit': _case_nan,
    'dir_limit_offset_1': _simple(10, 2, 5, 7, 6, 3, cfg_of(120, 50, 50), dir_offset=0.0, dir_limit_offset=1.0),
    'dir_limit_offset_0': _simple(10, 2, 5, 7, 6, 3, cfg_of(120, 50, 50), dir_offset=0.7854, dir_limit_offset=0.0),
    'one_class': _simple(15, 2, 5, 7, 6, 1, cfg_of(100, 50, 50)),
    'sixteen_classes': _simple(16, 2, 5, 7, 6, 16, cfg_of(100, 50, 50)),
    'one_anchor_per_cell': _simple(17, 2, 8, 11, 1, 3, cfg_of(50, 30, 30, nms_thr=0.3)),
}
_CASES, _EXPECTED = {}, {}


def case(name):
    if name not in _CASES:
        _CASES[name] = BUILDERS[name]()
    return _CASES[name]


def case_expected(name):
    """computed once per process and shared: never modified by a test"""
    if name not in _EXPECTED:
        c = case(name)
        _EXPECTED[name] = expected(c['cls'], c['bbox'], c['dirp'], c['anchors'], c['cfg'], c['C'], c.get('dir_offset', 0.7854),
                                   c.get('dir_limit_offset', 0.0))
    return _EXPECTED[name]


def run_case(amd, name, dev='cpu'):
    c = case(name)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out = amd.rpn_proposals(t(c['cls']), t(c['bbox']), t(c['dirp']), t(c['anchors']), c['cfg'], c['C'], dir_offset=c.get('dir_offset', 0.7854),
                            dir_limit_offset=c.get('dir_limit_offset', 0.0), return_candidates=True)
    return {k: v.cpu().numpy() for k, v in out.items()}


def same(got, want, what):
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape, want[k].shape)
        a, b = (got[k].view(np.uint32), want[k].view(np.uint32)) if got[k].dtype == np.float32 else (got[k], want[k])
        bad = np.nonzero((a != b).reshape(-1))[0]
        assert bad.size == 0, (what, k, bad[:8], got[k].reshape(-1)[bad[:8]], want[k].reshape(-1)[bad[:8]])
