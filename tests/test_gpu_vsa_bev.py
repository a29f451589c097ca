"""The keypoint BEV interpolation, the voxel centres and the keypoint gather on the MI355X (csrc/vsa_bev.hip): the cases of
tests/test_cpu_vsa_bev.py on cuda:0.  The interpolated features and the map's gradient within the same bounds against the fp64
restatement (computed on the CPU, once per case), in both layouts; the forward bit-identical to the `_cpu` twin, between the layouts and
from run to run; the voxel centres and counts bit-identical to the twin and to the fp32 torch statements; the integer-exact backward; the
16-byte and the 4-byte access paths bit-identical; every output element written and nothing beyond; the robustness inputs; and the chain
voxel_centers -> sample_keypoints -> bev_interpolate -> QueryAndGroup, forward and backward, captured in one graph.

Figures: every case passes on gfx950; the largest |ours - fp64| / bound per tensor is in DESIGN.md §3.13's table."""
import pytest
import torch

import mmdet3d_gaussian_amd as amd
import vsa_bev_ref as ref
from mmdet3d_gaussian_amd import _lib, vsa_bev
from test_cpu_vsa_bev import (LAYOUTS, check_centre_sweep, check_centres, check_centres_many_ids, check_interp_case,
                              check_interp_single_misaligned_operand, check_robustness, check_sample_keypoints, check_sweep_exact,
                              check_sweep_forward, geometry, in_layout, run_interp)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
S = -77.0           # the sentinel of the guard tests


@pytest.mark.parametrize('name', sorted(ref.INTERP_CASES))
def test_bev_interpolate_on_the_device(name):
    case = ref.interp_reference(name)[0]
    got = {layout: run_interp(case, layout, dev=DEV) for layout in LAYOUTS}
    for layout in LAYOUTS:
        check_interp_case(got[layout], name, f'gfx950 {layout}')          # the shared-cell case: grad_bev equal to fp64 exactly
    twin = run_interp(case, 'nchw', dev='cpu')
    assert torch.equal(got['nchw']['out'], twin['out']), 'the forward is the twin\'s bits'
    assert torch.equal(got['nchw']['out'], got['channels_last']['out']), 'the forward is the same bits in both layouts'
    for layout in LAYOUTS:                                                # run to run (the gradient is summed atomically: not compared)
        assert torch.equal(run_interp(case, layout, dev=DEV)['out'], got[layout]['out'])


def test_bev_interpolate_misaligned_base_equals_the_aligned_case():
    """C = 64, channels last, with the map viewed one float into a larger buffer: the 4-byte path gives the 16-byte path's bits; and
    the same for NCHW"""
    case = ref.interp_reference(ref.MISALIGNED_OF)[0]
    for layout in LAYOUTS:
        shift = (lambda t: ref.offset_view(t.permute(0, 2, 3, 1)).permute(0, 3, 1, 2) if t.dim() == 4 else ref.offset_view(t)) \
            if layout == 'channels_last' else ref.offset_view
        aligned, shifted = run_interp(case, layout, dev=DEV), run_interp(case, layout, dev=DEV, view=shift)
        assert torch.equal(aligned['out'], shifted['out']), layout
        check_interp_case(shifted, ref.MISALIGNED_OF, f'gfx950 {layout} offset view')


@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('name', ['m63_c3_5x7_half_s8', 'm130_c260_5x7_halfmin_s8', 'outside_far_c64', 'm1_c1_2x2_half_s8'])
def test_every_interp_output_element_is_written(name, layout):
    """the C entry points on sentinel-filled outputs with a guard row either side: every element of `out` (zero rows included) and of
    `grad_bev` (the zeros of untouched cells included) is written, and nothing beyond the arrays"""
    case = ref.interp_reference(name)[0]
    kp = case['keypoints'].to(DEV)
    bev = in_layout(case['bev'].to(DEV), layout)
    g = case['grad_out'].to(DEV).contiguous()
    B, C, H, W = bev.shape
    M = kp.size(1)
    flag = int(layout == 'channels_last')
    dense = bev.permute(0, 2, 3, 1) if flag else bev                 # the map as it lies in memory
    assert dense.is_contiguous()
    corners = vsa_bev._corners(case['voxel_size'][:2], case['point_cloud_range'][:2], case['point_cloud_range'][3:5], case['scale'], case['align'])
    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
    out = torch.full((B * M + 2, C), S, device=DEV)
    guard = C * W                                                     # floats either side of grad_bev
    grad = torch.full((bev.numel() + 2 * guard,), S, device=DEV)
    _lib.check(lib.gd3d_vsa_bev_interp(kp.data_ptr(), kp.stride(0), kp.stride(1), dense.data_ptr(), flag, B, M, C, H, W, *corners,
                                       out[1:].data_ptr(), stream), 'gd3d_vsa_bev_interp')
    _lib.check(lib.gd3d_vsa_bev_interp_backward(g.data_ptr(), kp.data_ptr(), kp.stride(0), kp.stride(1), flag, B, M, C, H, W, *corners,
                                                grad[guard:].data_ptr(), stream), 'gd3d_vsa_bev_interp_backward')
    assert (out[0] == S).all() and (out[-1] == S).all() and not (out[1:-1] == S).any()
    assert (grad[:guard] == S).all() and (grad[-guard:] == S).all() and not (grad[guard:-guard] == S).any()
    body = grad[guard:-guard].view(dense.shape)
    got = dict(out=out[1:-1].view(B, M, C).cpu(), grad_bev=(body.permute(0, 3, 1, 2) if flag else body).cpu().contiguous())
    check_interp_case(got, name, f'gfx950 {layout} C entry')
    assert torch.equal(got['out'], run_interp(case, layout, dev=DEV)['out'])


@pytest.mark.parametrize('name', sorted(ref.SWEEP_CASES))
def test_bev_interpolate_sweep_forward(name):
    """B * M = 2 x 32771 = 65542 keypoints > 16384 workgroups x 4 keypoints (L = 64 lanes each): six keypoints fall to the second trip of
    interp_kernel<false> (C = 64, NCHW) and of interp_kernel<true> (C = 256, channels last)"""
    check_sweep_forward(name, DEV)


def test_bev_interpolate_sweep_backward_is_exact():
    """the same 65542 keypoints, C = 64 (L = 64, 4 keypoints per workgroup), through interp_backward_kernel in both layouts: the second
    trip's six rows add into the map exactly once"""
    check_sweep_exact(DEV)


@pytest.mark.parametrize('shift', ['bev', 'out'])
def test_bev_interpolate_single_misaligned_operand_equals_the_aligned_run(shift):
    check_interp_single_misaligned_operand(shift, DEV)


@pytest.mark.parametrize('dtype', [torch.int32, torch.int64])
def test_voxel_centers_sweep(dtype):
    """N = 1 048 641 > 4096 workgroups x 256 rows: voxel_centers_kernel's second trip, its last wave one row wide"""
    xyz, cnt = check_centre_sweep(dtype, DEV)
    twin_xyz, twin_cnt = check_centre_sweep(dtype, 'cpu')
    assert torch.equal(xyz, twin_xyz) and torch.equal(cnt, twin_cnt)


@pytest.mark.parametrize('dtype', [torch.int32, torch.int64])
def test_voxel_centers_many_distinct_ids_in_a_wave(dtype):
    assert torch.equal(check_centres_many_ids(dtype, DEV), check_centres_many_ids(dtype, 'cpu'))


def test_non_finite_and_huge_coordinates_give_zero_rows():
    check_robustness(DEV)


@pytest.mark.parametrize('n', ref.CENTRE_N)
@pytest.mark.parametrize('dtype', [torch.int32, torch.int64])
def test_voxel_centers_on_the_device(n, dtype):
    for i, (align, scale) in enumerate(ref.CENTRE_GEOMETRY):
        coors = ref.make_coors(n, 3, 10 * n + i, dtype)
        xyz, cnt = check_centres(coors, align, scale, dev=DEV)            # the fp32 torch statements' bits
        twin_xyz, twin_cnt = amd.voxel_centers(coors, ref.VOXEL_SIZE, ref.point_cloud_range(1600, 1408, 1), scale, align, 3)
        assert torch.equal(xyz.cpu(), twin_xyz) and torch.equal(cnt.cpu(), twin_cnt)
    mixed = ref.make_coors(2049, 3, 4, dtype)                             # batch ids interleaved inside every wave: several adds per wave
    mixed[:, 0] = torch.arange(2049) % 5 - 1                              # -1, 0, 1, 2, 3 (= B): the first and the last are counted nowhere
    _, cnt = check_centres(mixed, 'half', 8, dev=DEV)
    assert cnt.tolist() == [410, 410, 410]


@pytest.mark.parametrize('dtype', [torch.int32, torch.int64])
def test_every_centre_output_element_is_written(dtype):
    coors = ref.make_coors(2049, 3, 21, dtype).to(DEV)
    rng = ref.point_cloud_range(1600, 1408, 1)
    want_xyz, want_cnt = amd.voxel_centers(coors, ref.VOXEL_SIZE, rng, 8, 'half', 3)
    size, lo, add = vsa_bev._centre_terms(ref.VOXEL_SIZE, rng[:3], 8, 'half')
    xyz = torch.full((2049 + 2, 3), S, device=DEV)
    cnt = torch.full((3 + 2,), -5, dtype=torch.int32, device=DEV)
    _lib.check(_lib.load().gd3d_vsa_voxel_centers(coors.data_ptr(), int(dtype == torch.int64), 2049, size, 8.0, lo, add, 3, xyz[1:].data_ptr(),
                                                  cnt[1:].data_ptr(), torch.cuda.current_stream().cuda_stream), 'gd3d_vsa_voxel_centers')
    assert (xyz[0] == S).all() and (xyz[-1] == S).all() and not (xyz[1:-1] == S).any()
    assert cnt[0] == -5 and cnt[-1] == -5
    assert torch.equal(xyz[1:-1], want_xyz) and torch.equal(cnt[1:-1], want_cnt) and int(cnt[2]) == 0     # the empty sample's zero is written


def test_sample_keypoints_on_the_device():
    want = check_sample_keypoints(DEV)
    assert torch.equal(want.cpu(), check_sample_keypoints('cpu'))


def test_vsa_stage_under_graph_capture():
    """voxel_centers -> sample_keypoints -> bev_interpolate -> QueryAndGroup and the gradients of the map and of the voxel features, for 2
    samples of ~300 voxels, 24 keypoints each: recorded on a single stream in ONE graph, replayed twice — the second time on new values
    AND new per-sample counts in the static buffers — and compared with the eager run bit for bit.  The voxel centres sit on sixteenths
    of a BEV cell and the upstream gradients are small integers, so the atomically summed gradients are exact in any order."""
    B, K, C, CB, H, W = 2, 24, 8, 16, 5, 7
    rng = ref.point_cloud_range(H, W, 8)
    g = torch.Generator().manual_seed(5)
    n = 600
    coors = torch.stack([torch.zeros(n, dtype=torch.int64), torch.randint(0, 32, (n,), generator=g), torch.randint(0, 8 * H, (n,), generator=g),
                         torch.randint(0, 8 * W, (n,), generator=g)], dim=1).int()
    coors[310:, 0] = 1
    coors = coors.to(DEV)
    feats = torch.randint(-4, 5, (n, C), generator=g).float().to(DEV).requires_grad_(True)
    bev = torch.randint(-4, 5, (B, CB, H, W), generator=g).float().to(DEV).requires_grad_(True)
    w_bev = torch.randint(-3, 4, (B, K, CB), generator=g).float().to(DEV)
    w_grp = torch.randint(-3, 4, (B * K, 3 + C, 8), generator=g).float().to(DEV)
    new_cnt = torch.full((B,), K, dtype=torch.int32, device=DEV)
    group = amd.QueryAndGroup(2.0, 8)

    def step():
        xyz, cnt = amd.voxel_centers(coors, ref.VOXEL_SIZE, rng, 1, 'half', B)
        kp = amd.sample_keypoints(xyz, cnt, K)
        bev_feats = amd.bev_interpolate(kp, bev, ref.VOXEL_SIZE, rng, 8, 'half')
        grouped, idx = group(xyz, cnt, kp.reshape(-1, 3), new_cnt, feats)
        g_bev, g_feats = torch.autograd.grad([bev_feats, grouped], [bev, feats], grad_outputs=[w_bev, w_grp])
        return [xyz, cnt, kp, bev_feats, grouped, idx, g_bev, g_feats]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        first = [t.detach().clone() for t in step()]      # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    assert first[1].tolist() == [310, 290] and first[6].any() and first[7].any() and first[3].any()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(captured, first):
        assert torch.equal(got.detach(), want)
    with torch.no_grad():                                 # new values and new counts in the static buffers
        bev.add_(1.0)
        coors[310:330, 0] = 0
        coors[:, 3] = (coors[:, 3] + 3) % (8 * W)
    graph.replay()
    torch.cuda.synchronize()
    eager = step()
    assert eager[1].tolist() == [330, 270] and not torch.equal(eager[2], first[2]) and not torch.equal(eager[6], first[6])
    for got, want in zip(captured, eager):
        assert torch.equal(got.detach(), want.detach())
