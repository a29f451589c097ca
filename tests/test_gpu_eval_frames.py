"""The batched per-frame stage of the flexible mAP (csrc/eval_frames.hip) on the device: all four columns against the `_cpu` twin and the
composition of the existing twins, bit for bit, on the case table of tests/eval_frames_cases.py; outputs written into the middle of
poisoned columns; two layouts over one dirty workspace; the call captured in a graph on one stream and replayed over other inputs; and
the evaluator's `frame_batch` keyword on device tensors against the golden fixture, against `frame_batch=0` and against its run on CPU
tensors.  The twin and the oracle are held to each other in tests/test_cpu_eval_frames.py."""
import numpy as np
import pytest
import torch

import eval_frames_cases as fc
import test_cpu_eval_ap as base
import test_cpu_eval_frames as cpu

pytestmark = pytest.mark.gpu

CASES = cpu.CASES


@pytest.fixture(scope='module')
def amd():
    import mmdet3d_gaussian_amd as m
    assert torch.cuda.is_available()
    m.load_library()
    return m


@pytest.mark.parametrize('case', CASES, ids=lambda c: c['name'])
def test_device_equals_twin_on_the_case_table(amd, case):
    """into the middle of poisoned columns: the block equals the oracle and the twin, the guard rows stay intact"""
    cols = fc.run_entry(case, 'cuda')
    fc.check_columns(case, cols, 'device')
    for d, t in zip(cols, fc.run_entry(case, 'cpu')):
        assert np.array_equal(fc.bits(d.cpu().numpy()), fc.bits(t.numpy()))


def test_two_layouts_back_to_back_over_one_dirty_workspace(amd):
    """Nothing is read before it is written: the workspace starts as 0xff bytes and is never cleared between layouts that share nothing
    (other problem sizes, another matcher form, other R and T)."""
    names = ['mixed_form2_iou3d_R4', 'mixed_form0_trans', 'single_D129_G256', 'mixed_form1_iou3d_R1', 'mixed_form2_iou3d_R4']
    cases = [cpu.case_named(n) for n in names]
    ws = torch.empty(max(fc.workspace_bytes(c) for c in cases), dtype=torch.uint8, device='cuda').fill_(0xff)
    for c in cases:
        ten = fc.to_device(c, 'cuda')
        cols = fc.fresh_columns(c['R'] * len(c['det']), 'cuda')
        assert fc.launch(c, ten, cols, ws=ws) == 0
        torch.cuda.synchronize()
        fc.check_columns(c, cols, 'shared workspace')


@pytest.mark.parametrize('name', ['mixed_form0_iou3d_R4', 'mixed_form1_ioubev', 'mixed_form2_trans'])
def test_graph_capture_and_replay(amd, name):
    """Capturable on one stream (no parallel branch): the captured call, replayed after EVERY input was overwritten with another case
    of the same layout, gives that case's records; replayed over the first inputs again, the eager call's."""
    case = cpu.case_named(name)
    other = fc.make_case(case['name'] + '_other', 991, case['sizes'], case['R'], case['T'], case['mode'], case['alias'],
                         case['gt_crowd'] is not None, group=np.where(case['group'] < 0, -1, case['group'][::-1] + 5))
    other['z_offset'] = case['z_offset']
    assert all(np.array_equal(case[k], other[k]) for k in ('det_seg', 'gt_seg', 'pair_off')) and not np.array_equal(case['det'], other['det'])
    ten = fc.to_device(case, 'cuda')
    rows = case['R'] * len(case['det'])
    cols = fc.fresh_columns(rows, 'cuda')
    ws = torch.empty(fc.workspace_bytes(case), dtype=torch.uint8, device='cuda')
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert fc.launch(case, ten, cols, ws=ws) == 0
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    fc.check_columns(case, cols, 'eager')
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert fc.launch(case, ten, cols, ws=ws) == 0
    for replay, c in enumerate((other, case)):
        for k in fc.INPUTS:
            if ten[k] is not None:
                ten[k].copy_(torch.from_numpy(np.ascontiguousarray(c[k])))
        for col, fresh in zip(cols, fc.fresh_columns(rows, 'cuda')):
            col.copy_(fresh)
        ws.fill_(0xff)
        graph.replay()
        torch.cuda.synchronize()
        fc.check_columns(c, cols, f'replay {replay}')


@pytest.mark.parametrize('name', ['mixed_form0_ioubev', 'single_D64_G2048', 'single_D1_G0', 'no_problem'])
def test_frames_records_wrapper_on_device_tensors_and_numpy(amd, name):
    case = cpu.case_named(name)
    want = fc.oracle(case)
    for conv in (lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda(), lambda a: a):      # numpy moves to the GPU
        got = amd.frames_records(**cpu._wrapper_args(case, conv))
        assert all(g.is_cuda for g in got)
        for g, w in zip(got, want):
            assert np.array_equal(fc.bits(g.cpu().numpy()), fc.bits(w))
    big = fc.make_case('too_many_gts', 3, [(1, 2049)], 1, 1, 'trans', False, False, thr_on_affinity=False)
    with pytest.raises(RuntimeError, match='too large'):
        amd.frames_records(**cpu._wrapper_args(big, lambda a: a))


# ---- the evaluator --------------------------------------------------------------------------------------------------------------------------

def test_golden_fixture_at_every_frame_batch_on_the_device(amd):
    """device tensors: held as check_golden holds today's path, equal to frame_batch=0 on the device, and equal to the CPU-tensor run"""
    on_device = cpu.golden_frame_batches('cuda', lambda d: base.as_tensors(d, 'cuda'))
    on_host = cpu.golden_frame_batches('cpu', lambda d: base.as_tensors(d, 'cpu'))
    assert on_device.keys() == on_host.keys() and len(on_device) == 12
    for key in on_device:
        cpu.same_results(on_device[key], on_host[key])


def test_golden_fixture_on_numpy_inputs_moved_to_the_device(amd):
    cpu.golden_frame_batches('cuda', lambda d: d)


@pytest.mark.parametrize('cfg', ['iou3d', 'ioubev'])
def test_tied_scores_keep_their_order_on_the_device(amd, cfg):
    convert = lambda d: base.as_tensors(d, 'cuda')      # noqa: E731
    today = cpu.tie_results(convert, 0, cfg)
    assert sum(v['num_det'] for _, v in today) > 3000
    for fb in (5, 60):
        cpu.same_results(cpu.tie_results(convert, fb, cfg), today)
    cpu.same_results(cpu.tie_results(lambda d: base.as_tensors(d, 'cpu'), 60, cfg), today)
