"""PV-RCNN's RPN proposal stage without a GPU: the `_cpu` twin (csrc/rpn_proposal_cpu.cpp) against the numpy restatement of
include/gd3d.h (tests/rpn_proposal_ref.py) — EXACT on every named case — and against the torch statements in fp64 within a derived
bound; the error and the special values of the fixed-sequence exponential; the wrapper's arguments, list form and hand-over to
`pvrcnn_assign_and_sample`; the twin under the address and undefined-behaviour sanitizers as a stand-alone program."""
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import mmdet3d_gaussian_amd as amd
import pvrcnn_sample_ref as sref
import rpn_proposal_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def t(a, dev='cpu'):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _host_driver(tmp_path, sanitize):
    from mmdet3d_gaussian_amd import _lib
    cxx = _lib._build.host_cxx_path()
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'rpn_proposal_sanitize')
    csrc = os.path.join(ROOT, 'mmdet3d-gaussian_amd', 'csrc')
    flags = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'] if sanitize else []
    cmd = [cxx, '-std=c++17', '-O1', '-g', *flags, '-ffp-contract=off', '-pthread', os.path.join(ROOT, 'tests', 'hostmath', 'rpn_proposal_sanitize.cpp'),
           os.path.join(csrc, 'rpn_proposal_cpu.cpp'), os.path.join(csrc, 'rbox_cpu.cpp'), '-o', exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
    return exe


FX_EXPF_WORST_ULP = 0.90     # the figure include/gd3d.h, csrc/fx_exp.h and DESIGN.md §3.25 document; below 1: faithful


def test_fx_expf_error_against_fp64_and_the_host_libm(tmp_path):
    """2^20 uniform fp32 arguments over the finite-result range, every integer multiple of ln 2 / 2 in range with 4 neighbours either
    side and the 4096 values either side of 0: the compiled sequence equals the numpy restatement bit for bit, and its worst error
    against fp64 exp, in ulps of the correctly rounded result, is below 1 (faithful) and at most the documented figure."""
    x = ref.fx_expf_sample()
    exe = _host_driver(tmp_path, sanitize=False)
    x.tofile(str(tmp_path / 'x.bin'))
    subprocess.run([exe, 'expf', str(tmp_path / 'x.bin'), str(tmp_path / 'y.bin')], check=True, timeout=120)
    y = np.fromfile(str(tmp_path / 'y.bin'), f32)
    fx, libm = y[:len(x)], y[len(x):]
    want = np.exp(x.astype(np.float64))
    ulp = np.spacing(np.abs(want.astype(f32))).astype(np.float64)
    e_fx, e_libm = np.abs(fx - want) / ulp, np.abs(libm - want) / ulp
    print(f'fx_expf worst {e_fx.max():.4f} ulp at {x[e_fx.argmax()]!r}; libm expf worst {e_libm.max():.4f} ulp; {len(x)} values')
    assert np.array_equal(ref.fx_expf(x).view(np.uint32), fx.view(np.uint32))
    assert e_fx.max() < 1.0
    assert e_fx.max() <= FX_EXPF_WORST_ULP


def test_fx_expf_special_values_and_cut_offs(tmp_path):
    """NaN -> NaN, +inf -> +inf, -inf -> +0; the last finite result at 0x42b17217 and +inf from the next value up; the last (normal)
    result at 0xc2aeac4f and +0 EXACTLY from the next value down: never a subnormal.  Twin and restatement agree on all of them."""
    hi, lo = ref.HI_CUT, ref.LO_CUT
    assert hi.view(np.uint32) == 0x42b17217 and lo.view(np.uint32) == 0xc2aeac4f
    # the cut-offs are where fp64 exp says: exp(hi) is finite in fp32 and exp(next up) is not; exp(lo) is normal, exp(next down) is not
    big, tiny = np.float64(np.finfo(f32).max), np.float64(np.finfo(f32).tiny)
    assert np.exp(np.float64(hi)) <= big < np.exp(np.float64(np.nextafter(hi, f32(np.inf))))
    assert np.exp(np.float64(np.nextafter(lo, f32(-np.inf)))) < tiny <= np.exp(np.float64(lo))
    x = f32([np.nan, np.inf, -np.inf, hi, np.nextafter(hi, f32(np.inf)), 100.0, 3e38, lo, np.nextafter(lo, f32(-np.inf)), -100.0, -104.0,
             -3e38, 0.0, -0.0, 1.0])
    exe = _host_driver(tmp_path, sanitize=False)
    x.tofile(str(tmp_path / 'x.bin'))
    subprocess.run([exe, 'expf', str(tmp_path / 'x.bin'), str(tmp_path / 'y.bin')], check=True, timeout=120)
    y = np.fromfile(str(tmp_path / 'y.bin'), f32)[:len(x)]
    for got in (y, ref.fx_expf(x)):
        assert np.isnan(got[0]) and got[1] == np.inf and got[2] == 0 and not np.signbit(got[2])
        assert np.isfinite(got[3]) and got[3] > f32(3.4e38) and np.all(got[4:7] == np.inf)
        assert got[7] >= np.finfo(f32).tiny and got[7] < f32(1.1755e-38)
        assert np.all(got[8:12].view(np.uint32) == 0)               # +0 exactly
        assert got[12] == 1.0 and got[13] == 1.0 and abs(float(got[14]) - math.e) < 3e-7
    assert np.array_equal(y.view(np.uint32)[1:], ref.fx_expf(x).view(np.uint32)[1:])


@pytest.mark.parametrize('name', sorted(ref.BUILDERS))
def test_twin_equals_the_restatement(name):
    ref.same(ref.run_case(amd, name), ref.case_expected(name), name)


def test_cases_reach_what_they_are_named_for():
    """the restatement's own bookkeeping: ties straddle the boundary and the lowest indices win, the lowest class and bin 0 win,
    an empty sample leaves no gap, a NaN anchor is never selected, more and fewer rows than M occur"""
    c, e = ref.case('ties_at_the_boundary'), ref.case_expected('ties_at_the_boundary')
    group = c['note']['group']
    for b in range(2):
        sel = set(e['cand_inds'][b].tolist())
        assert [n in sel for n in group] == [True, True, True, False, False, False]
        assert e['cand_inds'][b, -3:].tolist() == group[:3]
    c, e = ref.case('equal_class_and_dir'), ref.case_expected('equal_class_and_dir')
    assert e['cand_inds'][0, :4].tolist() == c['note']['anchors'][::-1] and e['labels_3d'][0] == 1
    an = ref.make_anchors(5, 7, 6)[e['cand_inds'][0, 0]]
    bb = ref.anchor_rows(c['bbox'], 7)[0][e['cand_inds'][0, 0]]
    raw = ref.decode(an[None], bb[None])[0][0, 6]
    assert e['boxes_3d'][0, 6] == ref.dir_fix(f32([raw]), np.zeros(1, np.int32), 0.7854, 0.0)[0]        # bin 0
    e = ref.case_expected('empty_middle_sample')
    assert e['batch_cnt'].tolist() == [30, 0, 30] and e['cand_cnt'][1] == 0
    assert e['rois'][:60, 0].tolist() == [0.0] * 30 + [2.0] * 30 and np.all(e['rois'][60:, 0] == -1) and np.all(e['labels_3d'][60:] == -1)
    c, e = ref.case('nan_logit'), ref.case_expected('nan_logit')
    for b, n in c['note']['nan']:
        assert n not in e['cand_inds'][b].tolist() and e['cand_inds'][b, -1] == -1
    for name in ('post_below_max_more_kept_than_M', 'post_above_max_more_kept_than_M'):
        cfg = ref.case(name)['cfg']
        assert ref.case_expected(name)['batch_cnt'].tolist() == [min(cfg['nms_post'], cfg['max_num'])] * 2
    e = ref.case_expected('fewer_kept_than_M')
    assert 0 < e['batch_cnt'].max() < 400 and np.all(e['cand_cnt'] < 210)
    assert not np.array_equal(ref.case_expected('axis_aligned_nms')['boxes_3d'], ref.case_expected('rotated_nms')['boxes_3d'])
    assert not np.array_equal(ref.case_expected('dir_limit_offset_0')['boxes_3d'][:, 6], ref.case_expected('dir_limit_offset_1')['boxes_3d'][:, 6])


def test_no_score_lies_within_4_ulp_of_the_threshold():
    """score_thr = 0.3 decides on a rounded sigmoid: the cases' own logits keep every score more than 4 ulp away from it"""
    thr = f32(0.3).view(np.int32)
    for name in sorted(ref.BUILDERS):
        c = ref.case(name)
        if c['cfg']['score_thr'] != 0.3:
            continue
        L = ref.anchor_rows(c['cls'], c['C'])
        best = np.where(np.isnan(L).any(2), f32(0), np.nan_to_num(L, nan=0.0).max(2))
        s = ref.sigmoid(best.reshape(-1))
        assert np.abs(s.view(np.int32).astype(np.int64) - int(thr)).min() > 4, name


def _fp64_statements(c, b):
    """the torch statements of get_bboxes_single + class_agnostic_nms for sample b in fp64 (NMS decisions by this package's CPU NMS on
    the fp32-rounded fp64 boxes: the inputs keep every IoU far from the threshold)"""
    cfg, C = c['cfg'], c['C']
    cls, bbox, dirp = (torch.from_numpy(c[k][b]).double() for k in ('cls', 'bbox', 'dirp'))
    anchors = torch.from_numpy(c['anchors']).double()
    dir_cls = torch.max(dirp.permute(1, 2, 0).reshape(-1, 2), dim=-1)[1]
    scores = cls.permute(1, 2, 0).reshape(-1, C).sigmoid()
    deltas = bbox.permute(1, 2, 0).reshape(-1, 7)
    max_scores, labels = scores.max(dim=1)
    order = max_scores.topk(min(cfg['nms_pre'], scores.shape[0]))[1]
    a, d = anchors[order], deltas[order]
    za = a[:, 2] + a[:, 5] / 2
    diag = torch.sqrt(a[:, 4] ** 2 + a[:, 3] ** 2)
    hg = torch.exp(d[:, 5]) * a[:, 5]
    boxes = torch.stack([d[:, 0] * diag + a[:, 0], d[:, 1] * diag + a[:, 1], d[:, 2] * a[:, 5] + za - hg / 2, torch.exp(d[:, 3]) * a[:, 3],
                         torch.exp(d[:, 4]) * a[:, 4], hg, d[:, 6] + a[:, 6]], 1)
    sc, lb, dr, cp = max_scores[order], labels[order], dir_cls[order], scores[order]
    m = sc > cfg['score_thr']
    boxes, sc, lb, dr, cp, an = boxes[m], sc[m], lb[m], dr[m], cp[m], a[m]
    bev = torch.stack([boxes[:, 0] - boxes[:, 3] / 2, boxes[:, 1] - boxes[:, 4] / 2, boxes[:, 0] + boxes[:, 3] / 2, boxes[:, 1] + boxes[:, 4] / 2,
                       boxes[:, 6]], 1)
    keep = amd.nms_gpu(bev.float(), sc.float(), cfg['nms_thr'])[:min(cfg['nms_post'], cfg['max_num'])]
    boxes, sc, lb, dr, cp, an = boxes[keep], sc[keep], lb[keep], dr[keep], cp[keep], an[keep]
    v = boxes[:, 6] - c['dir_offset']
    turns = v / math.pi + c['dir_limit_offset']
    boxes[:, 6] = v - torch.floor(turns) * math.pi + c['dir_offset'] + math.pi * dr.double()
    return boxes.numpy(), sc.numpy(), lb.numpy(), cp.numpy(), an.numpy(), turns.numpy()


def test_twin_against_the_fp64_torch_statements():
    """Boxes and scores against the published statements evaluated in fp64.  The bound, from the operation count, not from the output:
      score = 1 / (1 + fx_expf(-x)): fx_expf is within 0.90 ulp <= 0.90 * 2^-23 relative, the sum and the quotient add 2^-24 each, and
        d score / score = -(e / (1 + e)) de / e, so |d score| <= (1.8 + 2) * 2^-24 * score < 4 * 2^-24 (score <= 1); the class scores alike.
      a box coordinate passes through at most 10 separately rounded operations (z: /, +, *, +, fx_expf's product, /, -; yaw: +, -, /, +,
        *, -, +, *, +), each within 2^-24 of an intermediate no larger than S = the sum of the magnitudes of the anchor's entries, the
        row's outputs and the 3 pi the direction fix can add; fx_expf contributes 1.8 more half-ulps: 12 * 2^-24 * S.  The fp32 pi
        differs from pi by 8.75e-8, which the direction fix multiplies by at most |floor| + 1 turns.
    The inputs are made so that the decisions agree: anchors 10 m apart with small deltas (every IoU is near 0, near 0.26 or above
    0.85: far from nms_thr), logits spaced 2^-6 apart, and the test asserts that no kept yaw sits within 1e-4 turns of a fold."""
    B, H, W, A, C = 2, 5, 7, 6, 3
    c = ref.make_inputs(21, B, H, W, A, C, pitch=10.0, delta=0.01)
    N = H * W * A
    rng = np.random.default_rng(22)
    for b in range(B):      # separated by construction: a permutation of a 2^-6 grid for the class maxima, the other classes well below
        L = np.full((N, C), -9.0, f32)
        L[np.arange(N), rng.integers(0, C, N)] = (rng.permutation(N).astype(f32) - f32(N / 2)) * f32(2.0 ** -6)
        c['cls'][b] = L.reshape(H * W, A, C).transpose(1, 2, 0).reshape(A * C, H, W)
    c.update(cfg=ref.cfg_of(120, 60, 70, nms_thr=0.6, score_thr=0.31), dir_offset=0.7854, dir_limit_offset=0.0)
    got = amd.rpn_proposals(t(c['cls']), t(c['bbox']), t(c['dirp']), t(c['anchors']), c['cfg'], C)
    got = {k: v.numpy() for k, v in got.items()}
    row = 0
    for b in range(B):
        boxes, sc, lb, cp, an, turns = _fp64_statements(c, b)
        assert np.abs(turns - np.round(turns)).min() > 1e-4
        m = len(boxes)
        assert got['batch_cnt'][b] == m and 10 < m <= 60
        assert np.array_equal(got['labels_3d'][row:row + m], lb)
        assert np.abs(got['scores_3d'][row:row + m] - sc).max() < 4 * 2.0 ** -24
        assert np.abs(got['cls_preds'][row:row + m] - cp).max() < 4 * 2.0 ** -24
        S = np.abs(an).sum(1) + np.abs(boxes).sum(1) + 3 * math.pi
        tol = 12 * 2.0 ** -24 * S[:, None] + 8.75e-8 * (np.abs(np.floor(turns)) + 1)[:, None]
        err = np.abs(got['boxes_3d'][row:row + m] - boxes)
        print(f'sample {b}: {m} rows, worst box error {err.max():.3e} (bound {tol.min():.3e}), score {np.abs(got["scores_3d"][row:row + m] - sc).max():.3e}')
        assert np.all(err <= tol)
        row += m


def test_argument_errors():
    B, A, C, H, W = 2, 6, 3, 5, 7
    c = ref.make_inputs(30, B, H, W, A, C)
    cls, bbox, dirp, an = t(c['cls']), t(c['bbox']), t(c['dirp']), t(c['anchors'])
    cfg = ref.cfg_of(100, 20, 20)
    ok = amd.rpn_proposals(cls, bbox, dirp, an, cfg, C)
    assert ok['boxes_3d'].shape == (B * 20, 7) and ok['rois'].shape == (B * 20, 8) and ok['cls_preds'].shape == (B * 20, C)
    assert ok['labels_3d'].dtype == torch.int64 and ok['batch_cnt'].dtype == torch.int32 and ok['scores_3d'].shape == (B * 20,)

    class Cfg:      # an object instead of a dict
        nms_pre, nms_post, max_num, nms_thr, score_thr, use_rotate_nms = 100, 20, 20, 0.7, 0.3, True
    for k, v in amd.rpn_proposals([cls], [bbox], [dirp], [an.reshape(1, H, W, 3, 2, 7)], Cfg(), C).items():
        assert torch.equal(v, ok[k]), k
    with pytest.raises(RuntimeError, match='levels'):
        amd.rpn_proposals([cls, cls], [bbox, bbox], [dirp, dirp], [an, an], cfg, C)
    with pytest.raises(RuntimeError, match='num_classes'):
        amd.rpn_proposals(torch.zeros(1, 17, 2, 2), torch.zeros(1, 7, 2, 2), torch.zeros(1, 2, 2, 2), torch.zeros(4, 7), cfg, 17)
    with pytest.raises(RuntimeError, match='cls_score'):
        amd.rpn_proposals(cls[:, :17], bbox, dirp, an, cfg, C)
    with pytest.raises(RuntimeError, match='cls_score'):
        amd.rpn_proposals(cls[0], bbox, dirp, an, cfg, C)
    with pytest.raises(RuntimeError, match='bbox_pred'):
        amd.rpn_proposals(cls, bbox[:, :-1], dirp, an, cfg, C)
    with pytest.raises(RuntimeError, match='dir_cls_pred'):
        amd.rpn_proposals(cls, bbox, dirp[:1], an, cfg, C)
    with pytest.raises(RuntimeError, match='anchors'):
        amd.rpn_proposals(cls, bbox, dirp, an[:-1], cfg, C)
    with pytest.raises(RuntimeError, match='fp32'):
        amd.rpn_proposals(cls.double(), bbox, dirp, an, cfg, C)
    with pytest.raises(RuntimeError, match='bbox_pred must be an fp32'):
        amd.rpn_proposals(cls, bbox.half(), dirp, an, cfg, C)
    with pytest.raises(RuntimeError, match='contiguous'):
        amd.rpn_proposals(cls, bbox, dirp.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2), an, cfg, C)
    with pytest.raises(RuntimeError, match='max_num'):
        amd.rpn_proposals(cls, bbox, dirp, an, dict(cfg, max_num=0), C)
    with pytest.raises(RuntimeError, match='NaN'):
        amd.rpn_proposals(cls, bbox, dirp, an, dict(cfg, score_thr=float('nan')), C)
    with pytest.raises(KeyError):
        amd.rpn_proposals(cls, bbox, dirp, an, dict(nms_pre=10), C)
    big = torch.zeros(1, 6 * 3, 40, 80)          # 19 200 anchors
    with pytest.raises(RuntimeError, match='candidates'):
        amd.rpn_proposals(big, torch.zeros(1, 42, 40, 80), torch.zeros(1, 12, 40, 80), torch.zeros(19200, 7), dict(cfg, nms_pre=16385), C)
    with pytest.raises(RuntimeError, match='candidates'):
        amd.rpn_proposals(big, torch.zeros(1, 42, 40, 80), torch.zeros(1, 12, 40, 80), torch.zeros(19200, 7), dict(cfg, nms_pre=0), C)
    lib = amd.load_library()
    assert lib.gd3d_rpn_proposal_workspace_bytes(4, 6, 3, 200, 176, 9000) > 4 * 211200 * 4
    assert lib.gd3d_rpn_proposal_workspace_bytes(4, 6, 17, 200, 176, 9000) == 0 and lib.gd3d_rpn_proposal_workspace_bytes(4, 6, 3, 200, 176, 0) == 0
    assert lib.gd3d_rpn_proposals_cpu(*([None] * 4), 1, 1, 1, 1, 1, 0, 1, 1, 0.5, 0.5, 1, 0.0, 0.0, *([None] * 9), 0) == 10001
    assert lib.gd3d_rpn_proposals_cpu(*([None] * 4), 1, 1, 17, 1, 1, 0, 1, 1, 0.5, 0.5, 1, 0.0, 0.0, *([None] * 9), 0) == 10002


def test_list_form_round_trips_and_feeds_assign_and_sample():
    name = 'empty_middle_sample'
    c, e = ref.case(name), ref.case_expected(name)
    args = (t(c['cls']), t(c['bbox']), t(c['dirp']), t(c['anchors']), c['cfg'], c['C'])
    packed = amd.rpn_proposals(*args)

    class Box:
        def __init__(self, tensor):
            self.tensor = tensor
    metas = [dict(box_type_3d=Box)] * 3
    head = amd.PartA2RPNHeadProposals(num_classes=c['C'], dir_offset=0.7854, dir_limit_offset=0.0)
    lists = head.get_bboxes([args[0]], [args[1]], [args[2]], [args[3]], metas, c['cfg'])
    assert (head.num_classes, head.dir_offset, head.dir_limit_offset) == (3, 0.7854, 0.0) and len(lists) == 3
    start = 0
    for b, d in enumerate(lists):
        m = int(e['batch_cnt'][b])
        assert isinstance(d['boxes_3d'], Box) and d['boxes_3d'].tensor.shape == (m, 7) and sorted(d) == ['boxes_3d', 'cls_preds', 'labels_3d', 'scores_3d']
        for k in ('scores_3d', 'labels_3d', 'cls_preds'):
            assert torch.equal(d[k], packed[k][start:start + m]), (b, k)
        assert torch.equal(d['boxes_3d'].tensor, packed['boxes_3d'][start:start + m])
        start += m
    plain = amd.rpn_proposals(*args, as_lists=True)
    assert isinstance(plain[0]['boxes_3d'], torch.Tensor) and plain[1]['boxes_3d'].shape == (0, 7)
    # the packed outputs are pvrcnn_assign_and_sample's stacked operands; the list form gives the same assignment and draw
    g = torch.Generator().manual_seed(3)
    gts = [packed['boxes_3d'][i * 30:i * 30 + 4].clone() + 0.05 * torch.rand(4, 7, generator=g) for i in (0, 0, 1)]
    glab = [packed['labels_3d'][i * 30:i * 30 + 4].clone() for i in (0, 0, 1)]
    sampler = sref._sampler(16)
    keys, fill = torch.rand(3 * 30, generator=g), torch.rand(3 * 16, generator=g)
    stacked = amd.pvrcnn_assign_and_sample(packed['boxes_3d'], packed['labels_3d'], torch.cat(gts), torch.cat(glab), sref.SHIPPED, sampler,
                                           prop_batch_cnt=packed['batch_cnt'], gt_batch_cnt=torch.tensor([4, 4, 4], dtype=torch.int32),
                                           keys=keys, fill_keys=fill, return_assignment=True)
    listed = amd.pvrcnn_assign_and_sample([d['boxes_3d'] for d in plain], [d['labels_3d'] for d in plain], gts, glab, sref.SHIPPED, sampler,
                                          keys=keys[:60], fill_keys=fill, return_assignment=True)
    assert int(stacked['pos_batch_cnt'].sum()) > 0
    for k in ('rois', 'ious', 'inds', 'pos_bboxes', 'pos_gt_bboxes', 'pos_assigned_gt_inds', 'pos_batch_cnt', 'roi_batch_cnt'):
        assert torch.equal(stacked[k], listed[k]), k
    for k in ('gt_inds', 'max_overlaps', 'labels'):
        assert torch.equal(stacked[k][:60], listed[k]), k
    # rois / cls_preds are multi_class_nms_batch's operands: the padding rows (batch id -1) belong to no sample
    with pytest.raises(RuntimeError, match='no CPU path'):
        amd.multi_class_nms_batch(packed['cls_preds'], amd.xywhr2xyxyr(packed['rois'][:, [1, 2, 4, 5, 7]]), packed['rois'][:, 0], 3, 0.1, 0.1)


def test_host_twin_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """csrc/rpn_proposal_cpu.cpp compiled together with a stand-alone driver (tests/hostmath/rpn_proposal_sanitize.cpp, its own main)
    and the CPU NMS it calls under -fsanitize=address,undefined and run as a program on the CPU: exactly sized heap blocks, one cell,
    nms_pre round the anchor count, dead samples, NaN and +-inf logits, deltas of +-100.  The device kernels share that code.  A
    sanitizer build belongs on a CPU-only machine: with a GPU present the test skips before it compiles or starts anything."""
    if torch.cuda.is_available():
        pytest.skip('sanitizer builds run on a CPU-only machine, never where a GPU is present')
    exe = _host_driver(tmp_path, sanitize=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.rstrip().endswith('OK') and 'runtime error' not in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
