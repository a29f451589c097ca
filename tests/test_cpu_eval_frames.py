"""The per-frame stage of the flexible mAP for a batch of frames on the host: the `_cpu` twin of csrc/eval_frames.hip against the
COMPOSITION of the existing twins per problem (tests/eval_frames_cases.py), its argument rules, the `frames_records` wrapper, and the
evaluator's `frame_batch` keyword against today's path (`frame_batch=0`), bit for bit.  No GPU needed.

Every comparison of records is on bits: the entry promises the per-frame path's own bits, so no tolerance applies.  The evaluator's
results are held exactly as tests/test_cpu_eval_ap.py::check_golden holds today's path, and to equality with `frame_batch=0`.
"""
import os
import subprocess

import numpy as np
import pytest
import torch

import eval_ap_ref as ref
import eval_frames_cases as fc
import mmdet3d_gaussian_amd as amd
import test_cpu_eval_ap as base
from mmdet3d_gaussian_amd import _lib, evaluation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = fc.build_cases()
BADARG, TOOLARGE = 10001, 10002


def case_named(name):
    return next(c for c in CASES if c['name'].startswith(name))


# ---- the entry ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', CASES, ids=lambda c: c['name'])
def test_twin_equals_the_composition_of_the_existing_twins(case):
    fc.check_columns(case, fc.run_entry(case, 'cpu'))


def test_case_table_reaches_what_it_is_built_for():
    """matches exist, the alias copy changes bits, a threshold sits on an affinity, rows of group -1 and NaN detections occur"""
    hits = alias_changes = off_rows = nan_rows = 0
    for c in CASES:
        want = fc.oracle(c)
        hits += int(np.count_nonzero(want[2]))
        off_rows += int(np.count_nonzero(want[0] == -1))
        nan_rows += len(c['nan_rows'])
        if c['alias'] and c['R'] > 1:
            plain = fc.oracle({**{k: v for k, v in c.items() if k != 'want'}, 'alias': 0})
            alias_changes += int(np.count_nonzero(plain[2] != want[2]))
    assert hits > 1000 and alias_changes > 100 and off_rows > 100 and nan_rows > 50
    assert sum(c.get('thr_hits', 0) for c in CASES) >= 20
    assert {c['T'] for c in CASES} == {1, 2, 32} and {c['R'] for c in CASES} == {1, 4} and {c['mode'] for c in CASES} == set(fc.MODES)
    assert any(c['gt_crowd'] is not None and c['gt_crowd'].any() for c in CASES) and any(c['gt_crowd'] is None for c in CASES)


def test_a_detection_with_a_nan_coordinate_is_unmatched():
    seen = 0
    for c in CASES:
        if len(c['nan_rows']) == 0:
            continue
        ND = len(c['det'])
        got = fc.run_entry(c, 'cpu')
        tp = got[2].numpy()[fc.PAD:fc.PAD + c['R'] * ND].reshape(c['R'], ND)
        assert (tp[:, c['nan_rows']] == 0).all(), c['name']
        seen += len(c['nan_rows'])
    assert seen > 50


def test_an_exact_tie_goes_to_the_later_gt_and_the_threshold_is_inclusive():
    """one detection on two identical gts: the later one is taken, so a second identical detection finds the earlier one; the gt
    flags tell which is which through msk.  The threshold equals the affinity (IoU 1, distance 0)."""
    box = np.array([[1, 2, 0, 2, 4, 1.5, 0.3]], np.float32)
    for mode in fc.MODES:
        for flags in ([1, 3], [1, 0], [0, 1]):
            c = fc.make_case('tie', 1, [(2, 2)], 1, 1, mode, False, False, thr_on_affinity=False)
            c['det'][:], c['gt'][:], c['thrs'][:] = box, box, fc.affinity(c, box, box)[0, 0]
            c['det_flag'][:], c['gt_flag'][0] = 1, flags
            got = [x.numpy()[fc.PAD:fc.PAD + 2] for x in fc.run_entry(c, 'cpu')]
            fc.check_columns(c, fc.run_entry(c, 'cpu'))
            if flags == [1, 3]:          # both gts count: detection 0 takes gt 1 (the later), detection 1 takes gt 0
                assert got[2].tolist() == [1, 1] and got[3].tolist() == [1, 1], (mode, got)
            elif flags == [1, 0]:        # gt 1 is ignored: a non-ignore gt beats it, detection 0 takes gt 0, detection 1 the ignored gt 1
                assert got[2].tolist() == [1, 1] and got[3].tolist() == [1, 0], (mode, got)
            else:                        # gt 0 is ignored: detection 0 takes gt 1, detection 1 the ignored gt 0
                assert got[2].tolist() == [1, 1] and got[3].tolist() == [1, 0], (mode, got)


@pytest.mark.parametrize('name', ['mixed_form0_iou3d_R4', 'mixed_form2_trans', 'single_D65_G2047'])
def test_every_thread_count_gives_the_same_bits(name):
    case = case_named(name)
    for nthreads in (1, 2, 0):
        fc.check_columns(case, fc.run_entry(case, 'cpu', nthreads=nthreads), f'{nthreads} threads')


def _call(case, ten, cols, device_entry, **over):
    """the entry with some arguments replaced by position name"""
    names = ('mode', 'z_offset', 'negate', 'det', 'score', 'det_seg', 'ND', 'gt', 'gt_seg', 'NG', 'gt_crowd', 'pair_off', 'pairs', 'max_gt',
             'det_flag', 'gt_flag', 'group', 'thrs', 'P', 'R', 'T', 'alias_tp', 'o_group', 'o_score', 'o_tp', 'o_msk')
    args = dict(zip(names, fc.entry_args(case, ten, cols)))
    args.update(over)
    lib = _lib.load()
    if device_entry:
        return lib.eval_frames_records(*args.values(), None, None)
    return lib.eval_frames_records_cpu(*args.values(), 1)


@pytest.mark.parametrize('device_entry', [False, True], ids=['twin', 'device_entry'])
def test_argument_errors(device_entry):
    """Host-checkable nonsense is refused before anything is touched: the device entry returns before its first launch, so its rules are
    checked here too, on host pointers it never follows."""
    case = case_named('single_D33_G65')
    ten = fc.to_device(case, 'cpu')
    cols = fc.fresh_columns(case['R'] * 33, 'cpu')
    call = lambda **over: _call(case, ten, cols, device_entry, **over)      # noqa: E731
    assert call(max_gt=2049) == TOOLARGE
    assert call(max_gt=1 << 40) == TOOLARGE
    assert call(pairs=1 << 31) == TOOLARGE
    assert call(R=1 << 30) == TOOLARGE                                    # R * ND beyond int32
    for over in (dict(T=0), dict(T=33), dict(R=0), dict(P=-1), dict(mode=3), dict(mode=-1), dict(ND=-1), dict(NG=-1), dict(pairs=-1),
                 dict(max_gt=-1), dict(det=None), dict(score=None), dict(det_seg=None), dict(gt=None), dict(gt_seg=None), dict(pair_off=None),
                 dict(det_flag=None), dict(gt_flag=None), dict(group=None), dict(thrs=None), dict(o_group=None), dict(o_score=None),
                 dict(o_tp=None), dict(o_msk=None), dict(P=0)):
        assert call(**over) == BADARG, over
    if device_entry:
        assert call() == BADARG                                            # no workspace
    else:
        assert call() == 0
        assert call(max_gt=64) == BADARG                                   # a problem has 65 gts: the host tables are checked
        assert call(ND=32) == BADARG and call(pairs=33 * 65 - 1) == BADARG
    if device_entry:    # nothing was written by a refused call
        assert all((c.numpy() == np.asarray(p, c.numpy().dtype)).all() for c, p in zip(cols, fc.POISON))
    else:               # the one good call wrote its block only
        fc.check_columns(case, cols)
    # no rows: nothing to do, whatever else is null
    empty = case_named('single_D0_G5')
    ten0 = fc.to_device(empty, 'cpu')
    assert _call(empty, ten0, fc.fresh_columns(0, 'cpu'), device_entry) == 0


def test_workspace_size_is_the_carve():
    lib = _lib.load()
    up = lambda x: (x + 255) // 256 * 256      # noqa: E731
    for ND, pairs, R, T in ((0, 0, 1, 1), (1, 1, 1, 1), (1000, 12345, 4, 2), (65, 65 * 2048, 4, 32)):
        assert lib.eval_frames_workspace_bytes(ND, pairs, R, T) == max(256, up(4 * pairs) + up(4 * R * T * ND))
    for bad in ((-1, 0, 1, 1), (0, -1, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (1, 1, 1, 33), (1 << 31, 1, 1, 1), (1, 1 << 31, 1, 1), (1 << 30, 1, 4, 1)):
        assert lib.eval_frames_workspace_bytes(*bad) == 0


# ---- the wrapper -------------------------------------------------------------------------------------------------------------------------

def _wrapper_args(case, conv):
    return dict(det=conv(case['det']), score=conv(case['score']), det_seg=case['det_seg'], gt=conv(case['gt']), gt_seg=case['gt_seg'].tolist(),
                det_flag=conv(case['det_flag'].astype(bool)), gt_flag=conv(case['gt_flag']), group=case['group'], thrs=case['thrs'],
                mode=case['mode'], z_offset=case['z_offset'], negate=case['negate'],
                gt_crowd=None if case['gt_crowd'] is None else conv(case['gt_crowd']), alias_tp=bool(case['alias']))


@pytest.mark.parametrize('name', ['mixed_form0_ioubev', 'mixed_form1_trans', 'single_D64_G2048', 'single_D1_G0', 'no_problem'])
def test_frames_records_wrapper_on_cpu_tensors(name):
    case = case_named(name)
    rows = case['R'] * len(case['det'])
    want = fc.oracle(case)
    got = amd.frames_records(**_wrapper_args(case, lambda a: torch.from_numpy(np.ascontiguousarray(a))))
    assert [g.dtype for g in got] == list(fc.DTYPES) and all(g.shape == (rows,) and g.device.type == 'cpu' for g in got)
    for g, w in zip(got, want):
        assert np.array_equal(fc.bits(g.numpy()), fc.bits(w))
    # into rows [row, row + R * ND) of the caller's columns
    cols = fc.fresh_columns(rows, 'cpu')
    back = amd.frames_records(**_wrapper_args(case, lambda a: torch.from_numpy(np.ascontiguousarray(a))), out=cols, row=fc.PAD)
    assert all(b.data_ptr() == c[fc.PAD:].data_ptr() or rows == 0 for b, c in zip(back, cols))
    fc.check_columns(case, cols, 'out=')


def test_frames_records_wrapper_refuses_what_it_cannot_serve():
    case = case_named('single_D33_G65')
    conv = lambda a: torch.from_numpy(np.ascontiguousarray(a))      # noqa: E731
    good = _wrapper_args(case, conv)
    assert 'frames_records' in amd.__all__ and amd.frames_records is evaluation.frames_records
    for over, word in ((dict(mode='giou'), 'mode'), (dict(det_seg=[0, 32]), 'segment'), (dict(gt_seg=[0, 65, 66]), 'describe'),
                       (dict(group=np.zeros((2, 4), np.int32)), 'describe'), (dict(det_flag=conv(case['det_flag'][:, :-1])), 'flags'),
                       (dict(thrs=np.zeros(33, np.float32)), 'thresholds'), (dict(gt_crowd=conv(np.zeros(3, np.uint8))), 'crowd'),
                       (dict(out=fc.fresh_columns(5, 'cpu'), row=0), 'out')):
        with pytest.raises(RuntimeError, match=word):
            amd.frames_records(**dict(good, **over))
    big = fc.make_case('too_many_gts', 3, [(1, 2049)], 1, 1, 'trans', False, False, thr_on_affinity=False)
    with pytest.raises(RuntimeError, match='too large'):
        amd.frames_records(**_wrapper_args(big, conv))


# ---- the twin under sanitizers -------------------------------------------------------------------------------------------------------------

def test_host_twin_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """csrc/eval_frames_cpu.cpp and the twins it calls compiled together with a stand-alone driver (tests/hostmath/eval_frames_sanitize.cpp,
    its own main) under -fsanitize=address,undefined and run as a program on the CPU: exactly sized heap blocks, empty problems, rows of
    group -1, G = 0, all three modes, crowd flags given and NULL, 1, 3 and all threads.  A sanitizer build belongs on a CPU-only machine:
    with a GPU present the test skips before it compiles or starts anything."""
    if torch.cuda.is_available():
        pytest.skip('sanitizer builds run on a CPU-only machine, never where a GPU is present')
    cxx = _lib._build.host_cxx_path()
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'eval_frames_sanitize')
    csrc = os.path.join(ROOT, 'mmdet3d-gaussian_amd', 'csrc')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-ffp-contract=off', '-march=x86-64-v3',
           '-pthread', os.path.join(ROOT, 'tests', 'hostmath', 'eval_frames_sanitize.cpp'), os.path.join(csrc, 'eval_frames_cpu.cpp'),
           os.path.join(csrc, 'eval_ap_cpu.cpp'), os.path.join(csrc, 'rbox_cpu.cpp'), '-o', exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.rstrip().endswith('OK') and 'runtime error' not in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]


# ---- the evaluator: frame_batch against today's path -----------------------------------------------------------------------------------------

def same_results(got, want):
    """num_det, num_gt, recall and mAP equal, bit for bit"""
    assert len(got) == len(want)
    for (gk, gv), (wk, wv) in zip(got, want):
        assert gk == wk
        assert gv['num_det'] == wv['num_det'] and gv['num_gt'] == wv['num_gt'], (gk, gv, wv)
        assert np.float64(gv['recall']).view(np.int64) == np.float64(wv['recall']).view(np.int64), (gk, gv, wv)
        assert isinstance(gv['mAP'], np.float32) and gv['mAP'].view(np.int32) == wv['mAP'].view(np.int32), (gk, gv, wv)


def golden_frame_batches(device, convert):
    """the golden fixture at every frame_batch: held as check_golden holds today's path, and equal to frame_batch=0; returns the results"""
    z, det, anno, classes, ranges, thrs = base.load_golden()
    out = {}
    for cfg in ('iou3d', 'ioubev', 'trans'):
        fse = amd.FlexibleStatisticsEval(classes, thrs, [dict(type='RangeBreakdown', ranges=ranges)], dict(type=base.AFFINITY_TYPES[cfg]),
                                         dict(type='MatcherCoCo'), [], 0)
        today = fse.statistics_eval(convert(det), anno)
        for fb in (1, 7, 30, 64):
            got = fse.statistics_eval(convert(det), anno, frame_batch=fb)
            base.check_against_literal(got, base.golden_results(z, cfg))
            same_results(got, today)
            out[cfg, fb] = got
        same_results(fse.statistics_eval(convert(det), anno, frame_batch=None), today)
    return out


@pytest.mark.parametrize('inputs', ['numpy', 'cpu_tensors'])
def test_golden_fixture_at_every_frame_batch(inputs):
    golden_frame_batches('cpu', (lambda d: d) if inputs == 'numpy' else (lambda d: base.as_tensors(d, 'cpu')))


RANGE_EDGES = {'0-30m': (0, 30), '30-50m': (30, 50), '50m+': (50, 1e9)}
VOLUME_EDGES = {'small': (0, 20), 'large': (20, 1e9)}
BREAKDOWNS = [dict(type='RangeBreakdown', ranges=RANGE_EDGES), dict(type='VolumeBreakdown', ranges=VOLUME_EDGES),
              dict(type='RangeBreakdown', ranges={'near': (0, 30), 'far': (30, 1e9)}, apply_to=['Car'])]


def tie_dataset():
    """seed 0 of the generator with the scores rounded to two decimals: ties abound within and across frames.  Packed and per-frame
    torch reductions may round a norm or a product differently in the last bit, so every box's fp64 distance and volume must lie at
    least 1e-5 (relative) from every interval edge — asserted here, no case dropped."""
    det, anno = ref.random_dataset(0, 60, 3, 24, 8)
    det = [[np.concatenate([d[:, :-1], np.round(d[:, -1:], 2)], axis=1).astype(np.float32) for d in frame] for frame in det]
    boxes = np.concatenate([d[:, :7] for frame in det for d in frame] + [a['gt_bboxes'] for a in anno], axis=0).astype(np.float64)
    dist, vol = np.linalg.norm(boxes[:, :3], axis=1), np.prod(boxes[:, 3:6], axis=1)
    for q, edges in ((dist, (30.0, 50.0)), (vol, (20.0,))):
        for e in edges:
            assert (np.abs(q - e) / e).min() >= 1e-5, (e, (np.abs(q - e) / e).min())
    scores = np.concatenate([d[:, -1] for frame in det for d in frame])
    assert len(np.unique(scores)) <= 101 and len(scores) > 1000
    assert any(len(np.unique(d[:, -1])) < len(d) for frame in det for d in frame)       # ties inside one problem too
    return det, anno


TIE_DATA = {}


def tie_results(convert, frame_batch, cfg='iou3d', key=None):
    if 'data' not in TIE_DATA:
        TIE_DATA['data'] = tie_dataset()
    det, anno = TIE_DATA['data']
    fse = amd.FlexibleStatisticsEval(base.CLASSES, [0.5, 0.7], BREAKDOWNS, dict(type=base.AFFINITY_TYPES[cfg]), dict(type='MatcherCoCo'), [], 0)
    return fse.statistics_eval(convert(det), anno, frame_batch=frame_batch)


@pytest.mark.parametrize('cfg', ['iou3d', 'trans'])
def test_tied_scores_keep_their_order_under_the_batched_layout(cfg):
    """The batched path lays a batch's rows out breakdown-major; ap_accumulate sees the rows of one group in frame order, then rank,
    under both layouts, so with ties everywhere every result stays bit-equal."""
    convert = lambda d: base.as_tensors(d, 'cpu')      # noqa: E731
    today = tie_results(convert, 0, cfg)
    assert len(today) == 3 * 2 * (1 + 3 + 2) + 2 * 2 and sum(v['num_det'] for _, v in today) > 3000 and any(v['mAP'] > 0.1 for _, v in today)
    for fb in (5, 60):
        same_results(tie_results(convert, fb, cfg), today)


def test_batches_the_path_does_not_serve_go_frame_by_frame():
    det, anno = ref.random_dataset(5, 12, 3, 20, 6)
    fse = amd.FlexibleStatisticsEval(base.CLASSES, [0.5], [dict(type='RangeBreakdown', ranges=RANGE_EDGES)], dict(type='LidarCenterTransBEV'),
                                     dict(type='MatcherCoCo'), [], 0)
    tens = base.as_tensors(det, 'cpu')
    # frames that disagree on the key set of gt_attrs
    mixed = [dict(a, gt_attrs=dict(a['gt_attrs'], distance=np.linalg.norm(a['gt_bboxes'][:, :3], axis=1) + 1.0)) if i % 3 == 1 else a
             for i, a in enumerate(anno)]
    today = fse.statistics_eval(tens, mixed)
    for fb in (4, 12):
        same_results(fse.statistics_eval(tens, mixed, frame_batch=fb), today)
    # one frame with 2049 gts of a class: beyond the entry's limit
    rng = np.random.default_rng(8)
    crowd = dict(gt_bboxes=ref._boxes(rng, 2049, 60.0), gt_labels=np.full(2049, 1), gt_attrs=dict(ignore=rng.uniform(0, 1, 2049) < 0.1))
    big = anno[:5] + [crowd] + anno[6:]
    today = fse.statistics_eval(tens, big)
    assert sum(v['num_gt'] for k, v in today if k['class_name'] == 'Pedestrian' and k['breakdown'] == 'All') > 1800
    for fb in (5, 12):
        same_results(fse.statistics_eval(tens, big, frame_batch=fb), today)


def test_only_the_built_in_classes_are_batched():
    class MyIOU(amd.LidarIOU3D):
        pass

    class MyMatcher(amd.MatcherCoCo):
        pass

    class MyRange(amd.RangeBreakdown):
        pass
    det, anno = ref.random_dataset(5, 3, 3, 20, 6)
    tens = base.as_tensors(det, 'cpu')
    fse = amd.FlexibleStatisticsEval(base.CLASSES, [0.5], [], dict(type='LidarIOU3D'), dict(type='MatcherCoCo'), [], 0)
    good = fse.statistics_eval(tens, anno, frame_batch=2)
    for attr, obj, name in (('affinity_calculator', MyIOU(), 'MyIOU'), ('matcher', MyMatcher([0.5]), 'MyMatcher')):
        other = amd.FlexibleStatisticsEval(base.CLASSES, [0.5], [], dict(type='LidarIOU3D'), dict(type='MatcherCoCo'), [], 0)
        setattr(other, attr, obj)
        with pytest.raises(ValueError, match=name):
            other.statistics_eval(tens, anno, frame_batch=2)
        same_results(other.statistics_eval(tens, anno), good)          # frame_batch=0 serves any class, as today
    other = amd.FlexibleStatisticsEval(base.CLASSES, [0.5], [], dict(type='LidarIOU3D'), dict(type='MatcherCoCo'), [], 0)
    other.breakdown.append(MyRange({'a': (0, 1e9)}, base.CLASSES))
    with pytest.raises(ValueError, match='MyRange'):
        other.statistics_eval(tens, anno, frame_batch=2)


def test_eval_map_flexible_takes_frame_batch_last_and_an_iscrowd_attribute_still_raises(capsys):
    det, anno = ref.random_dataset(3, 12, 3, 20, 6)
    tens = base.as_tensors(det, 'cpu')
    kw = dict(match_thrs=[0.5], classes=base.CLASSES, breakdowns=[dict(type='RangeBreakdown', ranges=RANGE_EDGES, apply_to=['Car'])], logger='silent')
    today = amd.eval_map_flexible(tens, anno, **kw)
    assert amd.eval_map_flexible(tens, anno, frame_batch=5, **kw) == today
    assert amd.eval_map_flexible(tens, anno, [0.5], kw['breakdowns'], dict(type='LidarIOU3D'), dict(type='MatcherCoCo'), base.CLASSES, 'silent',
                                 [('map', lambda x: x['breakdown'] == 'All')], None, 5) == today
    k = next(i for i in range(len(anno)) if len(anno[i]['gt_labels']) and all(len(d) for d in det[i]))
    bad = dict(anno[k], gt_attrs=dict(anno[k]['gt_attrs'], iscrowd=np.zeros(len(anno[k]['gt_labels']), bool)))
    with pytest.raises(AssertionError, match='crowd'):
        amd.eval_map_flexible(tens[k:k + 1], [bad], classes=base.CLASSES, logger='silent', frame_batch=4)
