"""Hard voxelization, dynamic voxelization and the mean voxel encoder on the MI355X (csrc/hard_voxel.hip): the cases of
tests/hard_voxel_ref.py on cuda:0, through the helpers of tests/test_cpu_hard_voxel.py.  Every output — voxels, mean, coors, num_points,
voxel_batch_cnt, num — bit-identical to the numpy restatement of the sequential walk and to the `_cpu` twin, and from run to run; the
mean without the voxel tensor; bands around every output and around the workspace untouched; tail rows; a 70 000-point batch; the
static form recorded and replayed in one graph on fresh inputs; the device guard.  Exact equality everywhere: no tolerance."""
import numpy as np
import pytest
import torch

import hard_voxel_ref as ref
import mmdet3d_gaussian_amd as amd
from mmdet3d_gaussian_amd import _lib, voxelize
from test_cpu_hard_voxel import (OUTPUTS, case_of, check_case, check_dynamic, check_irregular_counts, check_mean_without_voxels, check_public_forms, check_pvrcnn_voxelize,
                                 check_voxel_mean, check_voxelization_module, run_static, stacked)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
S = -77.0           # the sentinel of the guard test


@pytest.mark.parametrize('name', sorted(ref.CASES))
def test_hard_voxelize_on_the_device(name):
    got = check_case(name, DEV)                                  # the restatement's bits, tail rows included
    twin, again = run_static(case_of(name), 'cpu'), run_static(case_of(name), DEV)
    for k in OUTPUTS:
        assert ref.same_bits(got[k], twin[k]), f'{name}: {k} differs from the twin'
        assert ref.same_bits(got[k], again[k]), f'{name}: {k} differs from run to run'
    check_mean_without_voxels(name, DEV)


@pytest.mark.parametrize('name', sorted(ref.CASES))
def test_dynamic_voxelize_and_the_encoder_alone_on_the_device(name):
    got = check_dynamic(name, DEV)
    assert torch.equal(got.cpu(), check_dynamic(name, 'cpu'))
    check_voxel_mean(name, DEV)


def test_sweep_of_70000_points():
    """3 samples of 30 001, 9 999 and 30 000 points, 274 workgroups per per-point kernel, the rows of 48 573 voxels (two samples cut at 20 000): against the
    restatement and with the 16-byte and the 4-byte row paths (a view one float into a wider buffer) giving the same bits"""
    got = check_case('sweep', DEV)
    check_mean_without_voxels('sweep', DEV)
    case = case_of('sweep')
    rows = torch.from_numpy(np.concatenate(case['samples'], 0)).to(DEV)
    wide = torch.zeros((rows.size(0), 5), device=DEV)
    wide[:, 1:] = rows
    shifted = wide[:, 1:]                                         # rows of stride 5 starting 4 bytes into the buffer: the scalar path
    cnt = torch.tensor([len(s) for s in case['samples']], dtype=torch.int32, device=DEV)
    assert shifted.data_ptr() % 16 == 4
    out = amd.hard_voxelize(shifted, case['voxel_size'], case['point_cloud_range'], case['P'], case['MV'], points_batch_cnt=cnt, with_mean=True,
                            static=True)
    for t, k in zip(out, ('voxels', 'coors', 'num_points', 'voxel_batch_cnt', 'mean')):
        assert ref.same_bits(t.cpu().numpy(), got[k]), k
    assert torch.equal(check_dynamic('sweep', DEV).cpu(), check_dynamic('sweep', 'cpu'))


@pytest.mark.parametrize('name', ['three_samples_middle_empty', 'voxel_cut_mv16', 'trailing_columns_c4', 'num_features_3_of_4', 'n0', 'every_point_dropped'])
def test_list_stacked_and_static_forms_agree(name):
    check_public_forms(name, DEV)


def test_pvrcnn_voxelize_equals_the_reference_loop():
    check_pvrcnn_voxelize(DEV)


def test_voxelization_module_mode_switch_and_dynamic_route():
    check_voxelization_module(DEV)


def test_counts_that_overrun_the_stack_and_negative_counts():
    check_irregular_counts(DEV)


@pytest.mark.parametrize('name', ['voxel_cut_mv16', 'slot_cut_p32', 'c7', 'trailing_columns_c4_stride8', 'every_point_dropped', 'n1', 'pillars_p32'])
def test_nothing_is_written_beyond_the_outputs_and_the_workspace(name):
    """the C entry points on sentinel-filled buffers with a guard band either side of every output and of the workspace: every row of
    every output is written (the tail rows -1 / 0 / 0), the bands stay untouched"""
    case, want = case_of(name), ref.expected(name)
    pts, cnt = voxelize._stacked(*stacked(case, DEV), 'test')
    N, C, B, P, MV, F = pts.size(0), case['C'], cnt.numel(), case['P'], case['MV'], case['F']
    R = min(N, B * MV)
    size, lo, grid = voxelize._geometry(tuple(float(v) for v in case['voxel_size']), tuple(float(v) for v in case['point_cloud_range']))
    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
    G = 64                                                        # guard elements either side
    bufs = dict(voxels=torch.full((R * P * C + 2 * G,), S, device=DEV), mean=torch.full((R * F + 2 * G,), S, device=DEV),
                coors=torch.full((R * 4 + 2 * G,), 77, dtype=torch.int32, device=DEV), num_points=torch.full((R + 2 * G,), 77, dtype=torch.int32, device=DEV),
                voxel_batch_cnt=torch.full((B + 2 * G,), 77, dtype=torch.int32, device=DEV), num=torch.full((2 + 2 * G,), 77, dtype=torch.int64, device=DEV),
                dynamic=torch.full((N * 4 + 2 * G,), 77, dtype=torch.int32, device=DEV))
    ws = lib.gd3d_hard_voxelize_workspace_bytes(N, B, MV)
    assert ws % 256 == 0
    band = 4096
    work = torch.full((ws + 2 * band,), 0x5a, dtype=torch.uint8, device=DEV)
    assert (work.data_ptr() + band) % 256 == 0
    at = lambda k: bufs[k][G:].data_ptr()
    _lib.check(lib.gd3d_hard_voxelize(pts.data_ptr(), N, pts.stride(0), C, cnt.data_ptr(), B, size, lo, grid, P, MV, F, work.data_ptr() + band,
                                      at('voxels'), at('mean'), at('coors'), at('num_points'), at('voxel_batch_cnt'), at('num'), stream),
               'gd3d_hard_voxelize')
    _lib.check(lib.gd3d_dynamic_voxelize(pts.data_ptr(), N, pts.stride(0), cnt.data_ptr(), B, size, lo, grid, at('dynamic'), stream),
               'gd3d_dynamic_voxelize')
    torch.cuda.synchronize()
    for k, t in bufs.items():
        guard = S if t.dtype == torch.float32 else 77
        assert (t[:G] == guard).all() and (t[-G:] == guard).all(), f'{k}: a guard band was written'
        assert ref.same_bits(t[G:-G].cpu().numpy().reshape(want[k].shape), want[k]), k
    assert (work[:band] == 0x5a).all() and (work[-band:] == 0x5a).all(), 'the workspace bands were written'
    mean = torch.full((R * F + 2 * G,), S, device=DEV)          # the encoder alone, on the voxels just written
    _lib.check(lib.gd3d_voxel_mean(at('voxels'), at('num_points'), R, P, C, F, mean[G:].data_ptr(), stream), 'gd3d_voxel_mean')
    assert (mean[:G] == S).all() and (mean[-G:] == S).all() and ref.same_bits(mean[G:-G].cpu().numpy().reshape(want['mean'].shape), want['mean'])


def test_static_form_under_graph_capture():
    """hard_voxelize(static=True) with its mean, voxel_centers on its coors and the encoder alone on its voxels, for 3 samples of ~100
    points: recorded on a single stream in ONE graph, replayed twice — the second time on new points AND new per-sample counts in the
    static buffers — and compared with the eager run bit for bit"""
    geom = ref.SMALL
    rng = np.random.default_rng(11)
    first = torch.from_numpy(ref._inside(rng, 300, geom, margin=0.05))
    second = torch.from_numpy(ref._inside(rng, 300, geom, margin=0.05))
    pts, cnt = first.to(DEV), torch.tensor([120, 80, 100], dtype=torch.int32, device=DEV)

    def step():
        voxels, coors, num_points, vbc, mean = amd.hard_voxelize(pts, geom['voxel_size'], geom['point_cloud_range'], 3, 40, points_batch_cnt=cnt,
                                                                 with_mean=True, static=True)
        xyz, per_sample = amd.voxel_centers(coors, geom['voxel_size'], geom['point_cloud_range'], 1, 'half', 3)
        return [voxels, coors, num_points, vbc, mean, xyz, per_sample, amd.voxel_mean(voxels, num_points)]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        warm = [t.clone() for t in step()]                        # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    assert warm[3].tolist() == [40, 40, 40] and torch.equal(warm[6], warm[3]) and torch.equal(warm[7], warm[4])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(captured, warm):
        assert torch.equal(got, want)
    pts.copy_(second.to(DEV))
    cnt.copy_(torch.tensor([10, 0, 290], dtype=torch.int32))
    graph.replay()
    torch.cuda.synchronize()
    eager = step()
    assert eager[3].tolist()[1:] == [0, 40] and 0 < eager[3].tolist()[0] <= 10 and not torch.equal(eager[1], warm[1])
    for got, want in zip(captured, eager):
        assert torch.equal(got, want)
    want = ref.hard_voxelize_ref([second.numpy()[:10], second.numpy()[10:10], second.numpy()[10:]], geom['voxel_size'], geom['point_cloud_range'], 3, 40, 4, 4)
    assert ref.same_bits(captured[0].cpu().numpy(), want['voxels']) and ref.same_bits(captured[4].cpu().numpy(), want['mean'])


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason='needs two visible devices')
def test_a_call_on_another_devices_tensors_leaves_the_callers_device_current():
    torch.cuda.set_device(0)
    got = run_static(case_of('voxel_cut_mv16'), 'cuda:1')
    assert torch.cuda.current_device() == 0
    for k in OUTPUTS:
        assert ref.same_bits(got[k], ref.expected('voxel_cut_mv16')[k]), k
    assert torch.equal(check_dynamic('voxel_cut_mv16', 'cuda:1').cpu(), check_dynamic('voxel_cut_mv16', 'cpu'))
