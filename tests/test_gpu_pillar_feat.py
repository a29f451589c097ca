"""The pillar encoders' point decoration on the MI355X (csrc/pillar_feat.hip): the cases of tests/pillar_feat_cases.py on cuda:0,
through the helpers of tests/test_cpu_pillar_feat.py.  Every output bit-identical to the numpy restatement and to the `_cpu` twin; the
fused stats bit-identical to the reference's statements written out over this package's own `Scatter` on the device; the chains from
voxelization; bands around every output, around the table and in the untouched columns of an `out=` tensor; both entries recorded and
replayed in one graph; the device guard.  Exact equality everywhere but `f_cluster` against torch's own sum (the bound of
test_cpu_pillar_feat.py)."""
import numpy as np
import pytest
import torch

import pillar_feat_cases as cases
import pillar_feat_ref as ref
import mmdet3d_gaussian_amd as amd
from mmdet3d_gaussian_amd import _lib, pillar_feat
from test_cpu_pillar_feat import (DECO_FLAGS, FLAG_SETS, check_deco, check_decoration_against_statements, check_modules, check_stats,
                                  check_views_and_forms, f_cluster_bound, index_of, run_deco, run_stats)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
S = -77.0           # the sentinel of the guard tests


@pytest.mark.parametrize('name', sorted(cases.STATS))
def test_stats_cases_on_the_device(name):
    got = check_stats(name, DEV)                                  # the restatement's bits
    assert ref.same_bits(got.cpu().numpy(), run_stats(cases.STATS[name], 'cpu').numpy()), f'{name}: differs from the twin'
    assert ref.same_bits(got.cpu().numpy(), run_stats(cases.STATS[name], DEV).cpu().numpy()), f'{name}: differs from run to run'
    kitti_dv = dict(with_cluster_center=False, with_covariance=False, with_voxel_center=False, with_voxel_point_count=False)
    check_stats(name, DEV, cols=4, append=True, **kitti_dv)      # 10 columns: the 4-byte store path and the one-launch-less-table path
    check_stats(name, DEV, with_covariance=False)                 # 16 columns: whole 16-byte rows


def test_stats_all_64_flag_sets_on_the_device():
    case = cases.STATS['sizes_1_to_9']
    for flags in FLAG_SETS:
        got = check_stats('sizes_1_to_9', DEV, **flags)
        assert ref.same_bits(got.cpu().numpy(), run_stats(case, 'cpu', **flags).numpy()), flags


def test_views_appended_columns_int64_rows_and_out():
    check_views_and_forms(DEV)


def test_modules():
    check_modules(DEV)


@pytest.mark.parametrize('name', sorted(cases.STATS))
def test_fused_stats_equal_the_statements_over_our_own_scatter(name):
    """PointVoxelStatsCalculator.forward written out over mmdet3d_gaussian_amd.Scatter on the device (reduce_mapback, mapback, torch
    elementwise ops): bit-identical, all 25 channels — the mean kernels share the summation order"""
    case = cases.STATS[name]
    if len(case['points']) == 0:
        assert run_stats(case, DEV).shape == (0, 25)
        return
    xyz = torch.from_numpy(case['points']).to(DEV)[:, :3].contiguous()
    sc = amd.Scatter(torch.from_numpy(case['coors']).to(DEV))
    want = ref.stats_statements(xyz, sc, case['voxel_size'], case['point_cloud_range'])
    got = amd.point_voxel_stats(xyz, sc, case['voxel_size'], case['point_cloud_range'])
    assert want.dtype == torch.float32 and ref.same_bits(got.cpu().numpy(), want.cpu().numpy()), name


def test_chain_from_dynamic_voxelization():
    """dynamic_voxelize -> Scatter -> point_voxel_stats(append_features=True) equals DynamicPillarFeatureNet.forward:214-216 written
    out (the KITTI dv config's flags), for three samples of 4-column points, some outside the range"""
    rng = np.random.default_rng(5)
    geom = cases.KITTI
    lo, hi = np.array(geom['point_cloud_range'][:3], np.float32), np.array(geom['point_cloud_range'][3:], np.float32)
    pts = (lo + rng.random((700, 3), dtype=np.float32) * np.array([4.0, 3.0, 4.0], np.float32)).astype(np.float32)
    pts[::23] += hi                                                # beyond the range: dropped
    feats = torch.from_numpy(np.concatenate([pts, rng.random((700, 1), dtype=np.float32)], 1)).to(DEV)
    cnt = torch.tensor([300, 150, 250], dtype=torch.int32, device=DEV)
    coors = amd.dynamic_voxelize(feats, geom['voxel_size'], geom['point_cloud_range'], cnt)
    sc = amd.Scatter(coors)
    assert int((sc.pts_voxel_maps < 0).sum()) >= 30 and sc.voxel_coors.size(0) > 70
    flags = dict(with_cluster_center=False, with_covariance=False, with_voxel_center=False, with_voxel_point_count=False)
    want = torch.cat([ref.stats_statements(feats[:, :3], sc, geom['voxel_size'], geom['point_cloud_range'], **flags), feats[:, 3:]], dim=-1)
    got = amd.point_voxel_stats(feats, sc, geom['voxel_size'], geom['point_cloud_range'], append_features=True, **flags)
    assert got.shape == (700, 10) and ref.same_bits(got.cpu().numpy(), want.cpu().numpy())


def test_chain_from_hard_voxelization():
    """hard_voxelize -> pillar_decorate equals the decoration of PillarFeatureNet.forward written out in torch (fp32 and float64 on the
    device): exact but for f_cluster, whose torch sum has no fixed order ((P + 2) * 2^-24 * max|x|), and the distance (3 ulp)"""
    rng = np.random.default_rng(6)
    geom = cases.KITTI
    lo = np.array(geom['point_cloud_range'][:3], np.float32)
    pts = np.concatenate([lo + rng.random((2000, 3), dtype=np.float32) * np.array([3.0, 2.5, 4.0], np.float32), rng.random((2000, 1), dtype=np.float32)], 1)
    voxels, coors, num, _ = amd.hard_voxelize(torch.from_numpy(pts.astype(np.float32)).to(DEV), geom['voxel_size'], geom['point_cloud_range'], 8, 400,
                                              points_batch_cnt=torch.tensor([1200, 800], dtype=torch.int32, device=DEV))
    assert voxels.size(0) > 100 and int(num.max()) == 8 and int(num.min()) >= 1
    got = amd.pillar_decorate(voxels, num, coors, geom['voxel_size'], geom['point_cloud_range'], True, True, True)
    want32 = ref.decorate_statements(voxels, num, coors, geom['voxel_size'], geom['point_cloud_range'], True, True, True)
    want64 = ref.decorate_statements(voxels.double(), num, coors, geom['voxel_size'], geom['point_cloud_range'], True, True, True)
    check_decoration_against_statements(got.cpu().numpy(), want32.cpu().numpy(), want64.cpu().numpy(), voxels.cpu().numpy(), num.cpu().numpy(), 4)
    twin = amd.pillar_decorate(voxels.cpu(), num.cpu(), coors.cpu(), geom['voxel_size'], geom['point_cloud_range'], True, True, True)
    assert ref.same_bits(got.cpu().numpy(), twin.numpy())


@pytest.mark.parametrize('shape', cases.DECO_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_decoration_cases_on_the_device(shape):
    check_deco(shape, DEV)
    case = cases.make_deco(*shape)
    for flags in DECO_FLAGS:
        assert ref.same_bits(run_deco(case, DEV, flags).cpu().numpy(), run_deco(case, 'cpu', flags).numpy()), (shape, flags)


def test_decoration_ignores_what_lies_in_padded_slots():
    for shape in ((300, 5, 4), (37, 33, 5), (300, 20, 5)):
        clean = check_deco(shape, DEV)
        for garbage in ('finite', 'nan'):
            got = check_deco(shape, DEV, garbage=garbage)
            assert torch.equal(got, clean) and not torch.isnan(got).any()
    case = cases.make_deco(300, 5, 4, garbage='finite')
    t = {k: torch.from_numpy(case[k]).to(DEV) for k in ('features', 'num_points', 'coors')}
    n = t['num_points'].clamp(max=5)
    want = ref.decorate_statements(t['features'], n, t['coors'], case['voxel_size'], case['point_cloud_range'], False, True, True)
    got = run_deco(case, DEV, (False, True, True))
    valid = torch.arange(5, device=DEV)[None, :] < n[:, None]
    assert (got[~valid] == 0).all() and (want[~valid] == 0).all()               # value-equal to the torch statements: zeros
    assert ref.same_bits(got[..., :7][valid].cpu().numpy(), want[..., :7][valid].cpu().numpy())


@pytest.mark.parametrize('name,flags,cols', [('v75_unbatched', 127, 5), ('three_samples_dropped', 2 | 16 | 64, 4), ('sizes_1_to_9', 1 | 2 | 8 | 32, 3),
                                             ('one_voxel_300', 31, 3), ('every_point_dropped', 127, 5), ('n1', 127, 3), ('near_1e4', 8, 3)])
def test_nothing_is_written_beyond_the_stats_output_and_the_table(name, flags, cols):
    """the C entry point on sentinel-filled buffers: a band either side of the table, a band either side of an `out` that is wider than
    the op's columns (the op writes columns [col, col + width) of every row and nothing else), and no element left unwritten"""
    case = cases.STATS[name]
    pts = torch.from_numpy(case['points']).to(DEV)[:, :cols].contiguous()
    sc = amd.Scatter(torch.from_numpy(case['coors']).to(DEV))
    N, C, V = pts.size(0), (cols if flags & 64 else 3), sc.voxel_pts_counts.numel()
    W = pillar_feat.stats_width(flags, C)
    size, off = pillar_feat._geom(case['voxel_size'], case['point_cloud_range'])
    G = 64
    ts = 12 if flags & 4 else 3
    order, seg = sc._grouping
    coors = sc.pts_coors.contiguous()
    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
    want = ref.stats_ref(case['points'][:, :cols], case['coors'], case['voxel_size'], case['point_cloud_range'], append_features=bool(flags & 64),
                         **dict(zip(ref.FLAG_NAMES, (bool(flags & 1), bool(flags & 2), bool(flags & 4), bool(flags & 8), bool(flags & 32), bool(flags & 16)))))
    # a wider tensor at an odd column (4-byte stores), the contiguous output (16-byte stores across rows), rows of whole vectors in a wider tensor
    for total, col in ((W + 9, 5), (W, 0), ((W + 3) // 4 * 4 + 8, 4)):
        buf = torch.full((N * total + 2 * G,), S, device=DEV)
        table = torch.full((V * ts + 2 * G,), S, device=DEV)
        _lib.check(lib.gd3d_point_voxel_stats(pts.data_ptr(), N, pts.stride(0), C, coors.data_ptr(), 0, coors.size(1), sc.pts_voxel_maps.data_ptr(),
                                              sc.voxel_pts_counts.data_ptr() if V else None, order.data_ptr(), seg.data_ptr(), V, size, off, flags,
                                              table[G:].data_ptr(), buf[G + col:].data_ptr(), total, stream), 'gd3d_point_voxel_stats')
        torch.cuda.synchronize()
        assert (buf[:G] == S).all() and (buf[-G:] == S).all() and (table[:G] == S).all() and (table[-G:] == S).all(), 'a guard band was written'
        rows = buf[G:-G].view(N, total)
        assert (rows[:, :col] == S).all() and (rows[:, col + W:] == S).all(), 'columns outside the op\'s were written'
        assert ref.same_bits(rows[:, col:col + W].cpu().numpy(), want), (total, col)
        if flags & 7 and V:
            assert not (table[G:-G] == S).any(), 'a table element was left unwritten'


@pytest.mark.parametrize('shape', [(1, 1, 3), (300, 5, 4), (37, 33, 5), (9, 100, 5), (300, 32, 4)], ids=lambda s: 'x'.join(map(str, s)))
def test_nothing_is_written_beyond_the_decoration(shape):
    case = cases.make_deco(*shape, garbage='nan')
    V, P, C = shape
    t = {k: torch.from_numpy(case[k]).to(DEV) for k in ('features', 'num_points', 'coors')}
    size, off = pillar_feat._geom(case['voxel_size'], case['point_cloud_range'])
    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
    for flags in (7, 3, 4, 0):
        W = C + 3 * bool(flags & 1) + 3 * bool(flags & 2) + bool(flags & 4)
        for G in (64, 63):                                        # 63: the output starts 4 bytes off a 16-byte boundary — the 4-byte store path
            buf = torch.full((V * P * W + 2 * G,), S, device=DEV)
            _lib.check(lib.gd3d_pillar_decorate(t['features'].data_ptr(), t['num_points'].data_ptr(), t['coors'].data_ptr(), V, P, C, size, off,
                                                flags, buf[G:].data_ptr(), stream), 'gd3d_pillar_decorate')
            torch.cuda.synchronize()
            assert (buf[:G] == S).all() and (buf[-G:] == S).all(), 'a guard band was written'
            want = ref.decorate_ref(case['features'], case['num_points'], case['coors'], case['voxel_size'], case['point_cloud_range'],
                                    bool(flags & 1), bool(flags & 2), bool(flags & 4))
            assert ref.same_bits(buf[G:G + V * P * W].cpu().numpy().reshape(want.shape), want), (shape, flags, G)


def test_both_entries_under_graph_capture():
    """point_voxel_stats (its Scatter built before the capture) and pillar_decorate recorded on a single stream in ONE graph; replayed
    on refilled inputs — new coordinates in the same cells, new slot contents and counts — and compared with the eager run bit for bit"""
    case = cases.STATS['three_samples_dropped']
    pts = torch.from_numpy(case['points']).to(DEV)
    sc = amd.Scatter(torch.from_numpy(case['coors']).to(DEV))
    first, second = cases.make_deco(300, 20, 5), cases.make_deco(300, 20, 5, seed=1)
    d = {k: torch.from_numpy(first[k]).to(DEV) for k in ('features', 'num_points', 'coors')}
    wide = torch.zeros((pts.size(0), 27), device=DEV)

    def step():
        stats = amd.point_voxel_stats(pts, sc, case['voxel_size'], case['point_cloud_range'], append_features=True, out=(wide, 0))
        return [stats, amd.pillar_decorate(d['features'], d['num_points'], d['coors'], first['voxel_size'], first['point_cloud_range'], True, True, True)]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        warm = [t.clone() for t in step()]                        # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(captured, warm):
        assert torch.equal(got, want)
    pts.mul_(torch.tensor([1.0, 1.0, 1.0, 0.5, 2.0], device=DEV)).add_(torch.tensor([0.001, -0.002, 0.01, 0.0, 0.0], device=DEV))
    for k in d:
        d[k].copy_(torch.from_numpy(second[k]))
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in captured]
    eager = step()
    assert not torch.equal(replayed[0], warm[0]) and not torch.equal(replayed[1], warm[1])
    for got, want in zip(replayed, eager):
        assert ref.same_bits(got.cpu().numpy(), want.cpu().numpy())
    assert ref.same_bits(replayed[0].cpu().numpy(), ref.stats_ref(pts.cpu().numpy(), case['coors'], case['voxel_size'], case['point_cloud_range'],
                                                                   append_features=True))


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason='needs two visible devices')
def test_a_call_on_another_devices_tensors_leaves_the_callers_device_current():
    torch.cuda.set_device(0)
    check_stats('three_samples_dropped', 'cuda:1')
    check_deco((37, 33, 5), 'cuda:1')
    assert torch.cuda.current_device() == 0
