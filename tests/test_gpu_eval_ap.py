"""The flexible mAP's kernels (csrc/eval_ap.hip) on the device against their `_cpu` twins, bit for bit on all three outputs, on the case
table of tests/eval_ap_ref.py — computed from the library's own tile size and scan chunk — and the evaluator end to end on device
tensors against the fixture recorded from the reference and against its own run on CPU tensors.  The twins are held to the
definition, to exact fractions and to the reference's literal lines in tests/test_cpu_eval_ap.py."""
import numpy as np
import pytest
import torch

import eval_ap_ref as ref
import test_cpu_eval_ap as cpu
from mmdet3d_gaussian_amd import _host, _lib, evaluation

pytestmark = pytest.mark.gpu

R, CHUNK = evaluation.ap_tile_rows(), evaluation.ap_scan_chunk_tiles()
CASES = ref.build_cases(R, CHUNK, big=True)


@pytest.fixture(scope='module')
def amd():
    import mmdet3d_gaussian_amd as m
    assert torch.cuda.is_available()
    m.load_library()
    return m


def same(got, want, what):
    for g, w, name in zip(got, want, ('num_det', 'recall', 'ap')):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape
        diff = g.view(np.int64) != w.view(np.int64)
        assert not diff.any(), f'{what}: {name} differs at (group, t) = {np.argwhere(diff)[0]}: {g[diff][0]!r} != {w[diff][0]!r}'


@pytest.mark.parametrize('case', CASES, ids=lambda c: c['name'])
def test_device_equals_twin_on_the_case_table(amd, case):
    got = cpu.run(case, 'cuda')
    same(got, cpu.run(case, 'cpu'), case['name'])
    if case['name'].endswith('second_scan_trip'):        # the one case the CPU suite leaves out: the definition itself, vectorised
        assert len(case['score']) == CHUNK * R + 1
        same(got, ref.vector_accumulate(case)[:3], case['name'] + ' (definition)')
    if case.get('big'):                                   # the other cases the CPU suite leaves out
        assert len(case['score']) > CHUNK * R
        same(got, ref.vector_accumulate(case)[:3], case['name'] + ' (definition)')


def device_args(case):
    dev = torch.device('cuda', torch.cuda.current_device())
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32) if a.dtype == np.uint32 else np.ascontiguousarray(a)).to(dev)  # noqa: E731
    cols = [t(case[k]) for k in ('group', 'score', 'tp', 'msk', 'num_gt')]
    n, K, T = len(case['score']), case['K'], case['T']
    ws_bytes = _lib.load().eval_ap_workspace_bytes(n, K, T)
    assert ws_bytes >= 256 and ws_bytes % 256 == 0 and ws_bytes >= n * (8 + 8 + 4 + 4 + 12)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    outs = (torch.empty((K, T), dtype=torch.int64, device=dev), torch.empty((K, T), dtype=torch.float64, device=dev),
            torch.empty((K, T), dtype=torch.float64, device=dev))

    def launch():
        _host.call('eval_ap_accumulate', dev, tuple(c.data_ptr() for c in cols) + (n, K, T) + tuple(o.data_ptr() for o in outs) + (ws.data_ptr(),))
    return cols, ws, outs, launch


def case_named(name):
    return next(c for c in CASES if c['name'].startswith(name))


@pytest.mark.parametrize('name', ['size_0', 'size_1', f'size_{3 * R + 5}', 'empty_groups', 'best_precision_in_last_tile', 'thresholds_32',
                                  'singletons', 'segments_dense_shift1', 'tile_edge_paths', 'max_groups'])
def test_poisoned_outputs_and_workspace(amd, name):
    """Nothing is read before it is written: outputs and workspace start as NaN bytes; a second run over the dirty workspace agrees."""
    case = case_named(name)
    cols, ws, outs, launch = device_args(case)
    want = cpu.run(case, 'cpu')
    for round_ in range(2):
        if round_ == 0:
            ws.fill_(0xff)
        for o in outs:
            o.view(torch.uint8).fill_(0xff)
        launch()
        same([o.cpu().numpy() for o in outs], want, f'{name} run {round_}')


def test_graph_capture_and_replay(amd):
    """Capturable on one stream: the captured call, replayed twice over fresh inputs of the same shape, equals the eager call."""
    case = case_named(f'size_{3 * R + 5}')
    other = dict(case, score=np.random.default_rng(9).permutation(case['score']), name='permuted')
    cols, ws, outs, launch = device_args(case)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = [o.cpu().numpy() for o in outs]
    same(eager, cpu.run(case, 'cpu'), 'eager')
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for replay, c in enumerate((other, case)):
        cols[1].copy_(torch.from_numpy(c['score']))
        for o in outs:
            o.view(torch.uint8).fill_(0xff)
        graph.replay()
        torch.cuda.synchronize()
        same([o.cpu().numpy() for o in outs], cpu.run(c, 'cpu'), f'replay {replay}')
    same([o.cpu().numpy() for o in outs], eager, 'replay against the eager call')


def _two_layouts():
    """Two cases of one (n, K, T) whose sorted layouts share nothing.  A: `segments_dense_shift1`, its group ids spread over K = 640
    (id + id // 5, so that empty groups lie between the occupied ones; its stray rows of group K take the new K).
    B: five occupied groups, one of them nearly all rows, every other group empty."""
    a = case_named('segments_dense_shift1')
    K, K_a, n, T = 640, a['K'], len(a['score']), a['T']
    g = a['group'].astype(np.int64)
    live = (g >= 0) & (g < K_a)
    assert K_a + K_a // 5 < K
    group = np.where(live, g + g // 5, np.where(g == K_a, K, g)).astype(np.int32)
    rng = np.random.default_rng(640)
    num_gt = rng.integers(0, 6, K)
    A = dict(a, name='layout_A', group=group, num_gt=num_gt, K=K)
    strays = 37
    B = ref._layout_case('layout_B', rng, [5, n - strays - 17, 1, 9, 2], T, K=K, ids=[3, 77, 78, 400, 639], strays=strays)
    assert len(B['score']) == n and B['T'] == T and B['K'] == K
    occupied_a = np.unique(group[(group >= 0) & (group < K)])
    assert len(occupied_a) >= 500 and len(np.setdiff1d(occupied_a, [3, 77, 78, 400, 639])) >= 500       # occupied in A, empty in B
    return A, B


def _load(cols, case):
    for col, k in zip(cols, ('group', 'score', 'tp', 'msk', 'num_gt')):
        a = np.ascontiguousarray(case[k])
        col.copy_(torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a))


def test_another_layout_over_the_same_dirty_workspace(amd):
    """A, B, A over one workspace that is never refilled: whatever the run before left in `range`, `total`, `inner` and `edge` —
    in bounds for this n, but of other groups — must not reach a result.  Each run equals the twin."""
    A, B = _two_layouts()
    want = {c['name']: cpu.run(c, 'cpu') for c in (A, B)}
    assert any((want['layout_A'][i] != want['layout_B'][i]).any() for i in range(3))
    cols, ws, outs, launch = device_args(A)
    ws.fill_(0xff)
    for step, c in enumerate((A, B, A, B)):
        _load(cols, c)
        for o in outs:
            o.view(torch.uint8).fill_(0xff)
        launch()
        same([o.cpu().numpy() for o in outs], want[c['name']], f"run {step} ({c['name']})")


def test_another_layout_in_graph_replays(amd):
    """The same sequence as replays of one captured call: every input column is copied in between, so the segment layout changes
    under the captured launches."""
    A, B = _two_layouts()
    want = {c['name']: cpu.run(c, 'cpu') for c in (A, B)}
    cols, ws, outs, launch = device_args(A)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    same([o.cpu().numpy() for o in outs], want['layout_A'], 'eager')
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for replay, c in enumerate((B, A, B, A)):
        _load(cols, c)
        for o in outs:
            o.view(torch.uint8).fill_(0xff)
        graph.replay()
        torch.cuda.synchronize()
        same([o.cpu().numpy() for o in outs], want[c['name']], f"replay {replay} ({c['name']})")


@pytest.mark.parametrize('G', [0, 9])
@pytest.mark.parametrize('D', [0, 1, 255, 256, 257])
def test_tp_records_block_edges_and_guard_rows_on_the_device(amd, D, G):
    """D around the workgroup size and G = 0: the device equals the twin, and writing rows [row, row + D) of a larger buffer leaves
    the rows around them alone."""
    rng = np.random.default_rng(1000 * G + D)
    T, row, pad = 3, 4, 9
    matched = rng.integers(-1, max(G, 1), (T, D)).astype(np.int32)
    matched[rng.uniform(0, 1, (T, D)) < 0.2] = G + 2
    args = (torch.from_numpy(matched), torch.from_numpy(rng.uniform(0, 1, D) < 0.6), torch.from_numpy(rng.uniform(0, 1, G) < 0.5),
            torch.from_numpy(rng.uniform(0, 1, D).astype(np.float32)))
    for m in (args[0], None):
        want = amd.tp_records(m, *args[1:], 5, num_thrs=T)
        got = amd.tp_records(None if m is None else m.cuda(), *[a.cuda() for a in args[1:]], 5, num_thrs=T)
        assert all(g.is_cuda and g.shape == (D,) and torch.equal(g.cpu(), w) for g, w in zip(got, want))
        out = tuple(torch.full((D + pad,), -1, dtype=dt, device='cuda') for dt in (torch.int32, torch.float32, torch.int32, torch.int32))
        amd.tp_records(None if m is None else m.cuda(), *[a.cuda() for a in args[1:]], 5, num_thrs=T, out=out, row=row)
        for c, w in zip(out, want):
            c = c.cpu()
            assert torch.equal(c[row:row + D], w) and (c[:row] == -1).all() and (c[row + D:] == -1).all()


def test_tp_records_on_the_device_equal_the_twin(amd):
    rng = np.random.default_rng(4)
    D, G, T = 1000, 37, 32
    matched = rng.integers(-1, G, (T, D)).astype(np.int32)
    matched[rng.uniform(0, 1, (T, D)) < 0.1] = G + 3
    args = (torch.from_numpy(matched), torch.from_numpy(rng.uniform(0, 1, D) < 0.6), torch.from_numpy(rng.uniform(0, 1, G) < 0.5),
            torch.from_numpy(rng.uniform(0, 1, D).astype(np.float32)))
    for m in (args[0], None):
        want = amd.tp_records(m, *args[1:], 5, num_thrs=T)
        got = amd.tp_records(None if m is None else m.cuda(), *[a.cuda() for a in args[1:]], 5, num_thrs=T)
        assert all(g.is_cuda and torch.equal(g.cpu(), w) for g, w in zip(got, want))


def test_evaluator_on_device_tensors_against_the_golden_fixture(amd):
    cpu.check_golden('cuda')


def test_evaluator_on_device_tensors_equals_its_run_on_cpu_tensors(amd):
    """Integers exact, fp64 bit-equal — the affinities, the matcher and the accumulation all replay on the host."""
    det, anno = cpu.safe_dataset('iou3d', [0.5, 0.7])
    for affinity, thrs in (('iou3d', [0.5, 0.7]), ('trans', [0.5, 2.0])):
        runs = []
        for device in ('cuda', 'cpu'):
            fse = amd.FlexibleStatisticsEval(cpu.CLASSES, thrs, [dict(type='RangeBreakdown', ranges=cpu.RANGES)],
                                             dict(type=cpu.AFFINITY_TYPES[affinity]), dict(type='MatcherCoCo'), [], 0)
            runs.append(fse.statistics_eval(cpu.as_tensors(det, device), anno))
        assert len(runs[0]) == len(runs[1]) > 0
        for (gk, gv), (ck, cv) in zip(*runs):
            assert gk == ck and gv['num_det'] == cv['num_det'] and gv['num_gt'] == cv['num_gt']
            assert np.float64(gv['recall']).view(np.int64) == np.float64(cv['recall']).view(np.int64)
            assert np.float32(gv['mAP']).view(np.int32) == np.float32(cv['mAP']).view(np.int32)
    # numpy detections move to the GPU: the same numbers again
    fse = amd.FlexibleStatisticsEval(cpu.CLASSES, [0.5, 2.0], [dict(type='RangeBreakdown', ranges=cpu.RANGES)], dict(type='LidarCenterTransBEV'),
                                     dict(type='MatcherCoCo'), [], 0)
    again = fse.statistics_eval(det, anno)
    assert [(k, v['num_det'], float(v['mAP'])) for k, v in again] == [(k, v['num_det'], float(v['mAP'])) for k, v in runs[0]]
