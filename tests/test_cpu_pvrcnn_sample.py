"""PV-RCNN's RoI assign-and-sample stage through the `_cpu` twins (csrc/roi_sample_cpu.cpp): `bbox_overlaps_3d` against an fp64
evaluation of the same boxes, `pvrcnn_assign_and_sample` EQUAL to the plain-torch restatement of tests/pvrcnn_sample_ref.py on every
case in the list, the stacked and the padded stacked form, device counts past the limits, the cheap overlap tests against the full
sequence, hostile values, the default keys, the wrapper's refusals, and the twin's source under ASan + UBSan as a stand-alone program.  tests/test_gpu_pvrcnn_sample.py runs the same checks on the MI355X."""
import os
import subprocess

import numpy as np
import pytest
import torch

import mmdet3d_gaussian_amd as amd
import pvrcnn_sample_ref as ref

INT_KEYS = ('inds', 'pos_assigned_gt_inds', 'pos_batch_cnt', 'roi_batch_cnt', 'gt_inds', 'labels')
ROW_KEYS = ('rois', 'ious', 'pos_bboxes', 'pos_gt_bboxes', 'max_overlaps')
PAD_P, PAD_G = 5, 3


def run_package(case, dev='cpu', form='lists', **kw):
    """the package on one case; `stacked`: concatenated tensors with device counts; `padded`: the same with junk rows past the counts"""
    to = lambda ts: [t.to(dev) for t in ts]
    props, plab, gts, glab = to(case['proposals']), to(case['proposal_labels']), to(case['gt_bboxes']), to(case['gt_labels'])
    keys, fill = case['keys'].to(dev), case['fill_keys'].to(dev)
    kw = dict(dict(keys=keys, fill_keys=fill, return_assignment=True), **kw)
    if form == 'lists':
        out = amd.pvrcnn_assign_and_sample(props, plab, gts, glab, case['assigner'], case['sampler'], **kw)
    else:
        pc = torch.tensor([p.shape[0] for p in props], dtype=torch.int32, device=dev)
        gc = torch.tensor([g.shape[0] for g in gts], dtype=torch.int64, device=dev)
        if form == 'padded':
            g = torch.Generator().manual_seed(5)
            props = props + [(torch.rand(PAD_P, 7, generator=g) + 0.5).to(dev)]
            plab = plab + [torch.zeros(PAD_P, dtype=torch.int64, device=dev)]
            gts = gts + [(torch.rand(PAD_G, 7, generator=g) + 0.5).to(dev)]
            glab = glab + [torch.zeros(PAD_G, dtype=torch.int64, device=dev)]
            kw['keys'] = torch.cat([keys, torch.rand(PAD_P, generator=g).to(dev)])
        out = amd.pvrcnn_assign_and_sample(torch.cat(props), torch.cat(plab), torch.cat(gts), torch.cat(glab), case['assigner'],
                                           case['sampler'], prop_batch_cnt=pc, gt_batch_cnt=gc, **kw)
    return {k: v.cpu() for k, v in out.items()}


def check_equal(got, want, padded=False):
    for k in INT_KEYS + ROW_KEYS:
        g = got[k]
        if padded and k in ('gt_inds', 'labels', 'max_overlaps'):        # rows of no sample: -1 / -1 / 0
            tail, g = g[-PAD_P:], g[:-PAD_P]
            assert (tail == (0 if k == 'max_overlaps' else -1)).all(), k
        assert g.dtype == want[k].dtype and torch.equal(g, want[k]), k


@pytest.mark.parametrize('name', ref.CASES)
def test_twin_equals_the_restatement(name):
    case, want, _ = ref.reference(name)
    lists = run_package(case, form='lists')
    check_equal(lists, want)
    stacked = run_package(case, form='stacked')
    for k in lists:
        assert torch.equal(lists[k], stacked[k]), k
    check_equal(run_package(case, form='padded'), want, padded=True)


def iou_tolerance(dev):
    """4x the worst deviation of the evaluation op `iou_3d(..., z_offset=0.5)` — the arithmetic pinned to the reference's own compiled
    C++ — from the fp64 values on the same rectangles (it turns counter-clockwise by yaw, the iou3d family clockwise: yaw negated)"""
    a, b, exact, ha, hb, hexact = ref.iou_inputs()
    flip = torch.tensor([1, 1, 1, 1, 1, 1, -1], dtype=torch.float32)
    dev_eval = (amd.iou_3d((a * flip).to(dev), (b * flip).to(dev), z_offset=0.5).cpu().double() - exact).abs().max().item()
    dev_hand = (amd.iou_3d((ha * flip).to(dev), (hb * flip).to(dev), z_offset=0.5).cpu().double().diagonal() - hexact).abs().max().item()
    return max(dev_eval, dev_hand)


def check_iou_values(dev):
    a, b, exact, ha, hb, hexact = ref.iou_inputs()
    yard = iou_tolerance(dev)
    got = amd.bbox_overlaps_3d(a.to(dev), b.to(dev)).cpu()
    hand = amd.bbox_overlaps_3d(ha.to(dev), hb.to(dev)).cpu().diagonal()
    err = max((got.double() - exact).abs().max().item(), (hand.double() - hexact).abs().max().item())
    print(f'bbox_overlaps_3d on {dev}: worst deviation from fp64 {err:.3e}; iou_3d on the same inputs {yard:.3e}; ratio {err / yard:.3f}')
    assert (exact > 0.05).sum() > 20 and yard > 0
    assert err <= 4 * yard
    assert hand[0] == 1.0 and hand[1] == 0.0 and hand[3] == 0.0                # identical; touching in z; disjoint in z only
    return got, hand


def test_iou_values_against_fp64():
    got, _ = check_iou_values('cpu')
    a, b = ref.iou_inputs()[:2]
    assert torch.equal(amd.bbox_overlaps_3d(a.double(), b.half().float().double()), amd.bbox_overlaps_3d(a, b.half().float()))   # evaluated in fp32
    assert amd.bbox_overlaps_3d(a[:0], b).shape == (0, 33) and amd.bbox_overlaps_3d(a, b[:0]).shape == (65, 0)
    assert got.dtype == torch.float32 and got.shape == (65, 33)


def hostile_case(base):
    case = dict(ref.reference(base)[0])
    p = case['proposals'][0].clone()
    p[::7, 0] = float('nan')
    p[3::11, 5] = float('nan')
    p[5::13, 3] = -1.0
    p[6::17, 6] = float('inf')
    g = case['gt_bboxes'][0].clone()
    g[2] = float('nan')
    keys = case['keys'].clone()
    keys[::5] = float('nan')
    keys[1::5] = -3.0
    keys[2::5] = 7.5
    fill = case['fill_keys'].clone()
    fill[::3] = float('nan')
    fill[1::3] = 1e30
    fill[2::3] = -1.0
    case.update(proposals=[p], gt_bboxes=[g], keys=keys, fill_keys=fill)
    return case


HOSTILE = ('b1_512_33', 'last_piece_short', 'dense_three_rounds')


def same_bits(a, b):
    """equal as bit patterns: NaN rows of a hostile proposal are copied into the outputs"""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                                     b.view(torch.int32) if b.dtype == torch.float32 else b)


def check_hostile(dev):
    """NaN / negative / infinite boxes and NaN / out-of-range keys: counts within [0, num], indices within their sample, every row of
    its stratum; on the small case the fill with replacement runs on the hostile fill keys, on the dense one the NaN rows (which
    pass both cheap tests with every gt) go through three rounds of the pair queue.  Returns the outputs by case."""
    outs = {}
    for base in HOSTILE:
        case = hostile_case(base)
        out = run_package(case, dev=dev)
        num, n, ng = 128, case['proposals'][0].shape[0], case['gt_bboxes'][0].shape[0]
        rows, pos = int(out['roi_batch_cnt'][0]), int(out['pos_batch_cnt'][0])
        assert 0 <= pos <= 64 and pos <= rows <= num and (base != 'last_piece_short' or rows == num)
        assert ((out['inds'] >= 0) & (out['inds'] < n)).all() and (out['rois'][:rows, 0] == 0).all() and (out['rois'][rows:, 0] == -1).all()
        assert ((out['gt_inds'] >= -1) & (out['gt_inds'] <= ng)).all() and not torch.isnan(out['max_overlaps']).any()
        assert ((out['pos_assigned_gt_inds'] >= 0) & (out['pos_assigned_gt_inds'] < ng)).all()
        assert (out['gt_inds'][out['inds'][:pos]] > 0).all() and (out['gt_inds'][out['inds'][pos:rows]] == 0).all()
        outs[base] = out
    return outs


def test_hostile_values_stay_in_bounds():
    outs = check_hostile('cpu')
    case = hostile_case('dense_three_rounds')        # the situation: the hostile rows leave the queue fuller than the clean case does
    q = ref.queued_pairs([case[k][0] for k in ('proposals', 'proposal_labels', 'gt_bboxes', 'gt_labels')], 3)
    assert q[0] > 2 * ref.WL_CAP and outs['dense_three_rounds']['pos_batch_cnt'][0] == 64


def check_clamped(dev):
    """device counts past the limits: 4100 proposals on 1030 gts in sample 0, 65 on 5 in sample 1.  Every sampled output equals the
    restatement of rows [:4096] on gts [:1024]; rows 4096..4099 are of no sample's assignment (-1 / -1 / 0); sample 1 starts after
    ALL of sample 0's rows and comes out as the restatement has it.  Returns the outputs."""
    full, want = ref.clamped_call()
    pc = torch.tensor([4100, 65], dtype=torch.int32, device=dev)
    gc = torch.tensor([1030, 5], dtype=torch.int32, device=dev)
    cat = lambda k: torch.cat(full[k]).to(dev)
    out = amd.pvrcnn_assign_and_sample(cat('proposals'), cat('proposal_labels'), cat('gt_bboxes'), cat('gt_labels'), full['assigner'],
                                       full['sampler'], prop_batch_cnt=pc, gt_batch_cnt=gc, keys=full['keys'].to(dev),
                                       fill_keys=full['fill_keys'].to(dev), return_assignment=True)
    out = {k: v.cpu() for k, v in out.items()}
    for k in INT_KEYS + ROW_KEYS:
        g = out[k]
        if k in ('gt_inds', 'labels', 'max_overlaps'):
            assert (g[4096:4100] == (0 if k == 'max_overlaps' else -1)).all(), k
            g = torch.cat([g[:4096], g[4100:]])
        assert g.dtype == want[k].dtype and torch.equal(g, want[k]), k
    rows = out['roi_batch_cnt'].tolist()
    assert rows[0] == 128 and rows[1] > 0 and (out['rois'][128:128 + rows[1], 0] == 1).all() and (out['inds'][:128] < 4096).all()
    assert (out['pos_assigned_gt_inds'][:int(out['pos_batch_cnt'][0])] < 1024).all()
    return out


def test_device_counts_past_the_limits_are_clamped():
    check_clamped('cpu')


@pytest.mark.parametrize('name', ['dense_two_rounds', 'dense_three_rounds', 'dense_2049', 'dense_4096', 'boundary_pairs'])
def test_cheap_tests_exclude_only_pairs_without_overlap(name):
    """the header's claim about `may_overlap`, on the twin (which never takes the shortcut): a pair the numpy restatement of the
    two cheap tests excludes has a cleaned IoU of exactly 0 in the full sequence"""
    case, _, _ = ref.reference(name)
    props, gts = case['proposals'][0], case['gt_bboxes'][0]
    may = torch.from_numpy(ref.may_overlap_np(props.numpy(), gts.numpy()))
    iou = amd.bbox_overlaps_3d(props, gts)
    assert (~may).any() and may.any() and not (iou[~may] > 0).any()
    print(name, ref.FACTS[name])


def check_default_keys(dev):
    case, _, _ = ref.reference('b3_num8')
    run = lambda: run_package(case, dev=dev, keys=None, fill_keys=None)
    torch.manual_seed(11)
    a = run()
    torch.manual_seed(11)
    b = run()
    c = run()
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a['inds'], c['inds'])
    start = 0
    for s, (rows, pos) in enumerate(zip(a['roi_batch_cnt'].tolist(), a['pos_batch_cnt'].tolist())):
        off = sum(p.shape[0] for p in case['proposals'][:s])
        gi = a['gt_inds'][off:off + case['proposals'][s].shape[0]]
        inds = a['inds'][start:start + rows]
        assert (gi[inds[:pos]] > 0).all() and (gi[inds[pos:]] == 0).all()
        start += rows


def test_default_keys_follow_the_seed():
    check_default_keys('cpu')


def test_lists_of_the_reference_shape():
    case, want, _ = ref.reference('b3_middle_empty')
    out = run_package_lists(case)
    rc, pc = want['roi_batch_cnt'].tolist(), want['pos_batch_cnt'].tolist()
    assert [t.shape for t in out['rois']] == [(r, 7) for r in rc] and [t.shape[0] for t in out['pos_gt_bboxes']] == pc
    assert torch.equal(torch.cat(out['rois']), want['rois'][:sum(rc), 1:]) and torch.equal(torch.cat(out['inds']), want['inds'][:sum(rc)])
    assert [t.shape[0] for t in out['gt_inds']] == [p.shape[0] for p in case['proposals']]


def run_package_lists(case):
    return amd.pvrcnn_assign_and_sample(case['proposals'], case['proposal_labels'], case['gt_bboxes'], case['gt_labels'], case['assigner'],
                                        case['sampler'], keys=case['keys'], fill_keys=case['fill_keys'], return_assignment=True, as_lists=True)


def test_refusals():
    case, _, _ = ref.reference('b4_tiny')
    args = (case['proposals'], case['proposal_labels'], case['gt_bboxes'], case['gt_labels'])
    ok_a, ok_s = case['assigner'], case['sampler']
    for bad in (dict(ok_a[0], ignore_iof_thr=0.5), dict(ok_a[0], iou_calculator=dict(type='BboxOverlapsNearest3D')), dict(ok_a[0], type='ATSS'),
                dict(ok_a[0], neg_iou_thr=(0.1, 0.3)), [ok_a[0]] * 17):
        with pytest.raises(RuntimeError, match='pvrcnn_assign_and_sample'):
            amd.pvrcnn_assign_and_sample(*args, bad, ok_s)
    for bad in (dict(ok_s, type='RandomSampler'), dict(ok_s, neg_pos_ub=3), dict(ok_s, add_gt_as_proposals=True), dict(ok_s, num=1025),
                dict(ok_s, neg_iou_piece_thrs=[0.1, 0.55]), dict(ok_s, neg_piece_fractions=[1.0]),
                dict(ok_s, neg_iou_piece_thrs=[0.1 * k for k in range(9, 0, -1)], neg_piece_fractions=[0.1] * 9)):
        with pytest.raises(RuntimeError, match='pvrcnn_assign_and_sample'):
            amd.pvrcnn_assign_and_sample(*args, ok_a, bad)
    big = [torch.zeros(4097, 7)] + list(case['proposals'][1:]), [torch.zeros(4097, dtype=torch.int64)] + list(case['proposal_labels'][1:])
    with pytest.raises(RuntimeError, match='at most'):
        amd.pvrcnn_assign_and_sample(big[0], big[1], case['gt_bboxes'], case['gt_labels'], ok_a, ok_s)
    with pytest.raises(RuntimeError, match='at most'):
        amd.pvrcnn_assign_and_sample(case['proposals'], case['proposal_labels'], [torch.zeros(1025, 7)] + list(case['gt_bboxes'][1:]),
                                     [torch.zeros(1025, dtype=torch.int64)] + list(case['gt_labels'][1:]), ok_a, ok_s)
    with pytest.raises(RuntimeError, match='shape mismatch'):
        amd.pvrcnn_assign_and_sample(*args, ok_a, ok_s, keys=torch.zeros(3))
    with pytest.raises(RuntimeError, match='stacked tensors need'):
        amd.pvrcnn_assign_and_sample(torch.cat(args[0]), torch.cat(args[1]), torch.cat(args[2]), torch.cat(args[3]), ok_a, ok_s)
    with pytest.raises(RuntimeError, match='shape mismatch'):
        amd.bbox_overlaps_3d(torch.zeros(3, 5), torch.zeros(3, 7))
    assert 'pvrcnn_assign_and_sample' in amd.__all__ and 'bbox_overlaps_3d' in amd.__all__


def write_case(path, case):
    """a case as the flat text the sanitizer driver reads: counts, then every operand in order"""
    a = case['assigner'] if isinstance(case['assigner'], list) else [case['assigner']]
    s = case['sampler']
    props, gts = torch.cat(case['proposals']), torch.cat(case['gt_bboxes'])
    with open(path, 'w') as f:
        put = lambda vals: f.write(' '.join(repr(float(v)) if isinstance(v, float) else str(int(v)) for v in vals) + '\n')
        put([len(case['proposals']), props.shape[0], gts.shape[0], len(a), s['num'], int(s['num'] * s['pos_fraction']), len(s['neg_iou_piece_thrs'])])
        put([p.shape[0] for p in case['proposals']])
        put([g.shape[0] for g in case['gt_bboxes']])
        for key in ('pos_iou_thr', 'neg_iou_thr', 'min_pos_iou'):
            put([float(c[key]) for c in a])
        put([(1 if c.get('match_low_quality', True) else 0) | (2 if c.get('gt_max_assign_all', True) else 0) for c in a])
        put([float(v) for v in s['neg_piece_fractions']])
        put([float(v) for v in s['neg_iou_piece_thrs']])
        put(np.frombuffer(props.numpy().tobytes(), np.uint32).tolist())            # fp32 operands as their bit patterns
        put(torch.cat(case['proposal_labels']).tolist())
        put(np.frombuffer(gts.numpy().tobytes(), np.uint32).tolist())
        put(torch.cat(case['gt_labels']).tolist())
        put(np.frombuffer(case['keys'].numpy().tobytes(), np.uint32).tolist())
        put(np.frombuffer(case['fill_keys'].numpy().tobytes(), np.uint32).tolist())


def test_host_twin_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """csrc/roi_sample_cpu.cpp compiled together with a stand-alone driver (tests/hostmath/roi_sample_sanitize.cpp, its own main) under
    -fsanitize=address,undefined and run as a program on the CPU: the pairwise IoU and the whole stage on three of the cases, exactly
    sized heap buffers, and the driver's checksums of the integer outputs compared with the restatement's.  A sanitizer build
    belongs on a CPU-only machine: with a GPU present the test skips before it compiles or starts anything."""
    if torch.cuda.is_available():
        pytest.skip('sanitizer builds run on a CPU-only machine, never where a GPU is present')
    from mmdet3d_gaussian_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = _lib._build.host_cxx_path()
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'roi_sample_sanitize')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-ffp-contract=off', '-march=x86-64-v3',
           os.path.join(root, 'tests', 'hostmath', 'roi_sample_sanitize.cpp'),
           os.path.join(root, 'mmdet3d-gaussian_amd', 'csrc', 'roi_sample_cpu.cpp'), '-o', exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
    for name in ref.SANITIZED:
        case, want, _ = ref.reference(name)
        path = str(tmp_path / (name + '.txt'))
        write_case(path, case)
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and 'runtime error' not in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
        sums = dict(line.split() for line in r.stdout.strip().splitlines() if len(line.split()) == 2)
        assert sums.pop('status') == 'OK'
        for k in ('inds', 'pos_assigned_gt_inds', 'pos_batch_cnt', 'roi_batch_cnt', 'gt_inds', 'labels'):
            w = want[k].long()
            assert int(sums[k]) == int(((w + 2) * (torch.arange(w.numel()) % 1009 + 1)).sum()), (name, k)
        assert int(sums['iou_bits']) == int(torch.cat([amd.bbox_overlaps_3d(p, g).reshape(-1).view(torch.int32).long()
                                                       for p, g in zip(case['proposals'], case['gt_bboxes'])]).sum()), name
