"""The SimOTA BEV assigner on the MI355X (csrc/simota.hip): the cases of tests/simota_ref.py on cuda:0.  Every output of
`simota_assign` EQUAL to the numpy restatement and to the `_cpu` twin in the list, stacked and shared-prior forms, and equal on a
second run; device counts past the rows; the C entry on sentinel-filled outputs with a guard row either side — every element
written, nothing beyond, the workspace's guards included; hostile values, the twin's bits; and the call captured in a graph with a
gather through `pos_inds` behind it, replayed on new data with other candidate and conflict counts."""
import numpy as np
import pytest
import torch

import mmdet3d_gaussian_amd as amd
import simota_ref as ref
from mmdet3d_gaussian_amd import _lib
from test_cpu_simota import KEYS, call_forms, same, t

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.mark.parametrize('name', sorted(ref.CASES))
def test_device_equals_the_restatement_and_the_twin(name):
    dev, twin, again = call_forms(name, DEV), call_forms(name, 'cpu'), call_forms(name, DEV)
    for (form, got, g_cap), (_, tw, _), (_, ag, _) in zip(dev, twin, again):
        same(got, ref.expected(name, g_cap), (name, form, 'restatement'))
        same(got, tw, (name, form, 'twin'))
        same(got, ag, (name, form, 'second run'))


def test_device_counts_past_the_rows_are_clamped():
    case = ref.CASES['empties']
    sc, bx, pr, gt, lb, pcnt, gcnt = ref.stacked(case)
    for pc, gc in (([100, 50, 10 ** 6, 5], [3, -2, 10 ** 6, 1]), ([40, 40], [2, 2]), ([10 ** 9], [10 ** 9])):
        pc, gc = np.array(pc, np.int32), np.array(gc, np.int32)
        got = amd.simota_assign(t(sc, DEV), t(bx, DEV), t(pr, DEV), t(gt, DEV), t(lb, DEV), prior_batch_cnt=t(pc, DEV), gt_batch_cnt=t(gc, DEV))
        want = ref.assign_batch(sc, bx, pr, gt, lb, pc, gc, min(len(gt), 1024))
        same({k: v.cpu().numpy() for k, v in got.items()}, want, list(pc))


# several samples with empty ones between; 1025 priors on 257 gts at candidate_topk 32; conflicts; the shared grid
@pytest.mark.parametrize('name', ['empties', 'sizes_topk32', 'crowd', 'shared_grid', 'hostile'])
def test_every_output_element_is_written_and_nothing_beyond(name):
    """the C entry point on sentinel-filled outputs with a guard row either side, the workspace between two guard blocks: every
    output element is written, no guard is touched"""
    case = ref.CASES[name]
    p = case['params']
    sc, bx, pr, gt, lb, pcnt, gcnt = ref.stacked(case)
    P, G, B, C, K = len(sc), len(gt), len(pcnt), sc.shape[1], p['topk']
    g_cap = int(gcnt.max())
    L = g_cap * K
    S = -77

    def buf(rows, cols=None, dtype=torch.int64):
        return torch.full((rows + 2,) if cols is None else (rows + 2, cols), S, dtype=dtype, device=DEV)
    out = dict(gt_inds=buf(P), labels=buf(P), max_overlaps=buf(P, dtype=torch.float32), pos_cnt=buf(B, dtype=torch.int32),
               pos_inds=buf(B, L), pos_gt_inds=buf(B, L))
    lib = _lib.load()
    ws_bytes = lib.gd3d_simota_workspace_bytes(P, B, g_cap, K)
    guard = 4096
    ws = torch.full((ws_bytes + 2 * guard,), 0xA5, dtype=torch.uint8, device=DEV)
    d = [t(a, DEV) for a in (sc, bx, pr, gt, lb, pcnt, gcnt)]
    ptr = lambda x: x.data_ptr() if x.numel() else None   # noqa: E731
    rc = lib.gd3d_simota_assign(ptr(d[0]), ptr(d[1]), ptr(d[2]), len(pr), pr.shape[1], int(case['shared']), d[5].data_ptr(), P, ptr(d[3]), ptr(d[4]),
                                d[6].data_ptr(), G, B, C, g_cap, p.get('radius', 0.5), K, 3.0, 1.0, p.get('match_init', 2.0),
                                *(out[k][1:].data_ptr() for k in KEYS), ws[guard:].data_ptr(), ws_bytes, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, 'gd3d_simota_assign')
    torch.cuda.synchronize()
    want = ref.expected(name, g_cap)
    for k, v in out.items():
        assert (v[0] == S).all() and (v[-1] == S).all(), k
        got = v[1:-1].cpu().numpy()
        a, b = (got.view(np.uint32), want[k].view(np.uint32)) if k == 'max_overlaps' else (got, want[k])
        assert np.array_equal(a, b), (name, k)
    assert (ws[:guard] == 0xA5).all() and (ws[guard + ws_bytes:] == 0xA5).all()


def test_hostile_values_give_the_twins_bits_and_stay_in_bounds():
    (_, got, _), (_, tw, _) = call_forms('hostile', DEV)[0], call_forms('hostile', 'cpu')[0]
    same(got, tw, 'hostile')
    P = len(got['gt_inds'])
    n = int(got['pos_cnt'][0])
    assert ((got['gt_inds'] >= 0) & (got['gt_inds'] <= 9)).all() and not np.isnan(got['max_overlaps']).any()
    assert ((got['pos_inds'][0, :n] >= 0) & (got['pos_inds'][0, :n] < P)).all() and (got['pos_inds'][0, n:] == -1).all()


def _batch(seed, trained, P=1500, G=12):
    rng = np.random.default_rng(seed)
    s = [ref.sample(rng, P, G, span=10.0, trained=trained) for _ in range(2)]
    return [torch.from_numpy(np.concatenate([x[k] for x in s])).to(DEV) for k in ('scores', 'boxes', 'priors', 'gts', 'labels')]


def test_captured_with_a_gather_through_pos_inds_and_replayed_on_new_data():
    """simota_assign and a gather of the positives' boxes and gts captured in one graph; replayed on other data — other candidate
    counts, other conflict counts — it equals the eager call on that data"""
    cnt = dict(prior_batch_cnt=torch.tensor([1500, 1500], dtype=torch.int32, device=DEV), gt_batch_cnt=torch.tensor([12, 12], dtype=torch.int32, device=DEV))
    static = _batch(1, True)

    def step():
        o = amd.simota_assign(*static, **cnt)
        idx, gidx = o['pos_inds'].clamp(min=0), o['pos_gt_inds'].clamp(min=0)
        live = (o['pos_inds'] >= 0).unsqueeze(-1)
        o['pos_boxes'] = static[1][idx] * live
        o['pos_gts'] = static[3][gidx] * live
        return o
    step()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = step()
    counts = []
    for seed, trained in ((2, False), (3, True), (4, False)):
        for dst, src in zip(static, _batch(seed, trained)):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        got = {k: v.clone() for k, v in held.items()}
        want = step()
        torch.cuda.synchronize()
        for k in want:
            assert torch.equal(got[k], want[k]), (seed, k)
        twin = amd.simota_assign(*(x.cpu() for x in static), **{k: v.cpu() for k, v in cnt.items()})
        for k in KEYS:
            assert torch.equal(got[k].cpu(), twin[k]), (seed, k)
        counts.append(tuple(got['pos_cnt'].tolist()))
    assert len(set(counts)) == 3 and all(min(c) > 0 for c in counts), counts
