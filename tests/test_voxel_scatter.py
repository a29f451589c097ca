"""§8f-4 dynamic scatter-reduce: oracle self-checks on CPU; GPU kernels vs the oracle.  The oracle itself is pinned to the
reference's own kernels (scatter_points_cuda.cu compiled for the device, oracle/_ref/ref_vox.so) by
tests/test_gpu_ref_kernels.py; see oracle/voxel_oracle.py."""
import numpy as np
import pytest
import torch

from oracle import voxel_oracle as vo


def _cloud(n, seed, grid=(40, 40, 2), c=9, neg_frac=0.03, dup=True):
    rng = np.random.default_rng(seed)
    coors = np.stack([rng.integers(0, g, n) for g in grid], -1).astype(np.int32)
    coors[rng.random(n) < neg_frac, rng.integers(0, 3)] = -1          # out-of-range points
    feats = rng.normal(0, 1, (n, c)).astype(np.float32)
    if dup and n > 10:
        feats[n // 2] = feats[n // 3]                                     # ties for max
        coors[n // 2] = coors[n // 3]
    return coors, feats


def test_oracle_index_and_reduce_properties():
    coors, feats = _cloud(3000, 0)
    uniq, pmap, cnt = vo.scatter_index(coors)
    assert (uniq >= 0).all() and cnt.sum() == (pmap >= 0).sum() and (np.diff(uniq.view([('', uniq.dtype)] * 3).ravel().argsort()) == 1).all()
    assert ((coors < 0).any(-1) == (pmap < 0)).all()
    np.testing.assert_array_equal(uniq[pmap[pmap >= 0]], coors[pmap >= 0])
    for red in ('sum', 'mean', 'max'):
        out, _ = vo.scatter_reduce(feats, pmap, cnt, red)
        v = 17
        rows = feats[pmap == v].astype(np.float64)
        want = {'sum': rows.sum(0), 'mean': rows.mean(0), 'max': rows.max(0)}[red]
        np.testing.assert_allclose(out[v], want, rtol=1e-12)
        # backward == autograd of a torch restatement
        gv = np.random.default_rng(1).normal(0, 1, out.shape)
        g = vo.scatter_backward(gv, feats, pmap, cnt, red)
        tf = torch.from_numpy(feats).double().requires_grad_(True)
        idx = torch.from_numpy(pmap[pmap >= 0].astype(np.int64))
        src = tf[torch.from_numpy(np.nonzero(pmap >= 0)[0])]
        if red == 'max':
            tout = torch.full(out.shape, -np.inf, dtype=torch.float64).scatter_reduce(0, idx[:, None].expand(-1, feats.shape[1]), src, 'amax')
            # torch splits ties evenly; compare only where the max is unique
            continue
        tout = torch.zeros(out.shape, dtype=torch.float64).index_add(0, idx, src)
        if red == 'mean':
            tout = tout / torch.from_numpy(cnt).double()[:, None]
        (tout * torch.from_numpy(gv)).sum().backward()
        np.testing.assert_allclose(g, tf.grad.numpy(), rtol=1e-12, atol=1e-14)


def test_host_scatter_index_matches_oracle_cpu():
    """The ATen statement of the index (what the product runs on the DEVICE beyond the kernels' limits, and what the GPU
    test compares vox_index_build with) against the numpy oracle, on CPU tensors; the public entry has no CPU path."""
    from mmdet3d_gaussian_amd.scatter import _index_and_grouping_torch, group_points, scatter_index
    coors, _ = _cloud(2000, 3)
    with pytest.raises(RuntimeError):
        scatter_index(torch.from_numpy(coors))
    u, m, c = _index_and_grouping_torch(torch.from_numpy(coors))[:3]
    uo, mo, co = vo.scatter_index(coors)
    np.testing.assert_array_equal(u.numpy(), uo); np.testing.assert_array_equal(m.numpy(), mo); np.testing.assert_array_equal(c.numpy(), co)
    assert m.dtype == torch.int32 and c.dtype == torch.int32
    order, seg = group_points(m, c)
    o = order.numpy(); s = seg.numpy()
    assert s[0] == (mo < 0).sum() and s[-1] == len(mo)
    for v in (0, 5, len(co) - 1):
        pts = o[s[v]:s[v + 1]]
        assert (mo[pts] == v).all() and (np.diff(pts) > 0).all()          # grouped, ascending point id
    e = scatter_index(torch.zeros(0, 3, dtype=torch.int32))
    assert e[0].shape == (0, 3) and e[1].numel() == 0


@pytest.mark.gpu
@pytest.mark.parametrize('n,ndim,dtype', [(1, 3, torch.int32), (255, 3, torch.int32), (70_001, 4, torch.int32), (2_000_000, 4, torch.int32),
                                          (5000, 4, torch.int64), (3000, 2, torch.int32), (4096, 8, torch.int32)])
def test_gpu_index_build_equals_the_aten_statement_and_the_oracle(n, ndim, dtype):
    """vox_index_build (round 3: one library call instead of ~20 ATen launches) against the ATen statement on the same
    device tensors — every output, bit for bit, incl. the grouping — and against the numpy oracle; dropped points
    (negative coordinates), an all-dropped batch, a single voxel and a batch column."""
    from mmdet3d_gaussian_amd.scatter import _index_and_grouping, _index_and_grouping_torch, scatter_index
    rng = np.random.default_rng(n + ndim)
    hi = [4, 6, 60, 70, 3, 3, 3, 3][:ndim] if ndim >= 4 else [40, 50, 30][:ndim]
    coors = np.stack([rng.integers(-1 if d == ndim - 1 else 0, h, n) for d, h in enumerate(hi)], -1)
    cases = [coors]
    if n >= 255:
        allneg = coors.copy(); allneg[:, 0] = -1
        one = np.zeros_like(coors); one[:, -1] = 7
        cases += [allneg, one]
    for cc in cases:
        t = torch.from_numpy(cc).to(dtype).cuda()
        got = _index_and_grouping(t)
        want = _index_and_grouping_torch(t)
        assert got[0].dtype == t.dtype and got[1].dtype == torch.int32 and got[2].dtype == torch.int32
        for a, b in zip(got[:3], want[:3]):
            assert torch.equal(a, b)
        assert torch.equal(got[3][0], want[3][0]) and torch.equal(got[3][1], want[3][1])
        if n <= 70_001:
            uo, mo, co = vo.scatter_index(cc)
            np.testing.assert_array_equal(got[0].cpu().numpy(), uo)
            np.testing.assert_array_equal(got[1].cpu().numpy(), mo)
            np.testing.assert_array_equal(got[2].cpu().numpy(), co)
    t0 = torch.from_numpy(coors).to(dtype).cuda()
    u, m, c = scatter_index(t0)
    w0 = _index_and_grouping_torch(t0)
    assert torch.equal(u, w0[0]) and torch.equal(m, w0[1]) and torch.equal(c, w0[2])


@pytest.mark.gpu
@pytest.mark.parametrize('n,c', [(1, 4), (257, 9), (5000, 10), (20000, 64), (3000, 130), (9000, 16), (7000, 128), (4000, 12), (60000, 3), (30000, 33),
                                 (5000, 127), (2000, 129), (1, 3)])
@pytest.mark.parametrize('red', ['sum', 'mean', 'max'])
def test_gpu_scatter_reduce_forward_backward(host_glue, n, c, red):
    import mmdet3d_gaussian_amd as amd  # noqa: F401
    from mmdet3d_gaussian_amd.scatter import Scatter
    coors, feats = _cloud(n, n + c, c=c)
    uo, mo, co = vo.scatter_index(coors)
    sc = Scatter(torch.from_numpy(coors).cuda())
    np.testing.assert_array_equal(sc.voxel_coors.cpu().numpy(), uo)
    np.testing.assert_array_equal(sc.pts_voxel_maps.cpu().numpy(), mo)
    np.testing.assert_array_equal(sc.voxel_pts_counts.cpu().numpy(), co)
    f = torch.from_numpy(feats).cuda().requires_grad_(True)
    out, vc = sc.reduce(f, red)
    want, _ = vo.scatter_reduce(feats, mo, co, red)
    if len(co) == 0:
        assert out.shape[0] == 0
        return
    if red == 'max':
        np.testing.assert_array_equal(out.detach().cpu().numpy(), want.astype(np.float32))     # max is exact
    else:
        np.testing.assert_allclose(out.detach().cpu().numpy(), want, rtol=2e-6, atol=2e-6)
    gv = np.random.default_rng(7).normal(0, 1, want.shape).astype(np.float32)
    out.backward(torch.from_numpy(gv).cuda())
    gw = vo.scatter_backward(gv, feats, mo, co, red)
    np.testing.assert_allclose(f.grad.cpu().numpy(), gw, rtol=2e-6, atol=1e-7)
    # mapback / reduce_mapback as the pillar encoders use them (voxel_encoders/utils.py:56)
    back = sc.reduce_mapback(f.detach(), red, default_feat=0)
    ref_back = np.where((mo >= 0)[:, None], want[np.clip(mo, 0, None)], 0)
    np.testing.assert_allclose(back.cpu().numpy(), ref_back, rtol=2e-6, atol=2e-6)


@pytest.mark.gpu
def test_gpu_scatter_batched_coors_and_determinism(host_glue):
    from mmdet3d_gaussian_amd.scatter import Scatter
    rng = np.random.default_rng(0)
    n = 8000
    coors3, feats = _cloud(n, 11, c=16)
    b = rng.integers(0, 3, n).astype(np.int32)
    coors4 = np.concatenate([b[:, None], coors3], 1)
    sc = Scatter(torch.from_numpy(coors4).cuda())
    assert sc.batch_size == 3 and sc.voxel_coors.shape[1] == 4
    f = torch.from_numpy(feats).cuda()
    o1, _ = sc.reduce(f, 'sum'); o2, _ = sc.reduce(f, 'sum')
    assert torch.equal(o1, o2)                                     # fixed summation order
    # per-sample voxels: every voxel row equals the sum over its batch-restricted points
    vc = sc.voxel_coors.cpu().numpy(); m = sc.pts_voxel_maps.cpu().numpy()
    for v in (0, len(vc) // 2, len(vc) - 1):
        sel = (m == v)
        assert (coors4[sel] == vc[v]).all()
        np.testing.assert_allclose(o1[v].cpu().numpy(), feats[sel].astype(np.float64).sum(0), rtol=1e-5, atol=1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize('c', [3, 4, 9, 10, 16, 33, 64, 100, 127])
@pytest.mark.parametrize('red', [0, 1, 2])
def test_gpu_backward_voxel_order_equals_map_order(c, red):
    """vox_scatter_backward_grouped (each voxel row read once, streamed to its points) must produce the same bits as the
    map-ordered gather, incl. zero rows for the points outside every voxel (3 % of the cloud) and untouched arg-max ties."""
    import mmdet3d_gaussian_amd as amd
    from mmdet3d_gaussian_amd.scatter import Scatter, group_points
    lib = amd.load_library()
    n = 30000
    coors, feats = _cloud(n, 100 + c, c=c, neg_frac=0.03)
    sc = Scatter(torch.from_numpy(coors).cuda())
    order, seg = group_points(sc.pts_voxel_maps, sc.voxel_pts_counts)
    assert int(seg[0]) > 0                                  # there ARE invalid points in this cloud
    v = sc.voxel_coors.shape[0]
    f = torch.from_numpy(feats).cuda()
    out = torch.empty(v, c, device='cuda'); arg = torch.empty(v, c, dtype=torch.int32, device='cuda')
    assert lib.vox_scatter_reduce(f.data_ptr(), order.data_ptr(), seg.data_ptr(), n, c, v, red, out.data_ptr(),
                                  arg.data_ptr() if red == 2 else None, None) == 0
    gv = torch.randn(v, c, device='cuda')
    a = torch.full((n, c), float('nan'), device='cuda'); b = torch.full((n, c), float('nan'), device='cuda')
    am = arg.data_ptr() if red == 2 else None
    assert lib.vox_scatter_backward(gv.data_ptr(), sc.pts_voxel_maps.data_ptr(), sc.voxel_pts_counts.data_ptr(), am, n, c, v,
                                    red, a.data_ptr(), None) == 0
    assert lib.vox_scatter_backward_grouped(gv.data_ptr(), order.data_ptr(), seg.data_ptr(), am, n, c, v, red, b.data_ptr(),
                                            None) == 0
    torch.cuda.synchronize()
    assert not torch.isnan(b).any() and torch.equal(a, b)
    assert (b[sc.pts_voxel_maps < 0] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize('red', ['sum', 'max'])
def test_gpu_scatter_feature_offsets_beyond_2_31(red):
    """36 M points x 64 channels = 2.3e9 floats: element offsets beyond int32 in the point-feature array.  The 64-channel
    result equals the two 32-channel halves reduced on their own (every channel is summed in ascending point order whatever
    the channel count), forward and backward, and the rows of the LAST points carry the right voxel's gradient."""
    from mmdet3d_gaussian_amd.scatter import Scatter
    n, c = 36_000_000, 64
    free, _ = torch.cuda.mem_get_info()
    if free < (48 << 30):
        pytest.skip('needs 48 GB of free HBM')
    dev = torch.device('cuda')
    g = torch.Generator(device=dev).manual_seed(3)
    coors = torch.stack([torch.randint(0, 10, (n,), generator=g, device=dev), torch.randint(0, 400, (n,), generator=g, device=dev),
                         torch.randint(0, 400, (n,), generator=g, device=dev)], 1).int()
    coors[::97, 1] = -1                                     # points outside every voxel
    feats = torch.empty(n, c, device=dev)
    for s in range(0, n, 4_000_000):
        feats[s:s + 4_000_000] = torch.randn(4_000_000, c, generator=g, device=dev)
    assert feats.numel() > 2 ** 31
    sc = Scatter(coors)
    f = feats.requires_grad_(True)
    out, _ = sc.reduce(f, red)
    halves = [sc.reduce(feats.detach()[:, k:k + 32].contiguous(), red)[0] for k in (0, 32)]
    assert torch.equal(out.detach()[:, :32], halves[0]) and torch.equal(out.detach()[:, 32:], halves[1])
    gv = torch.randn(out.shape, generator=g, device=dev)
    out.backward(gv)
    m = sc.pts_voxel_maps
    tail = slice(n - 1000, n)                               # rows whose offsets are beyond 2^31
    mt = m[tail].long()
    if red == 'sum':
        want = torch.where((mt >= 0)[:, None], gv[mt.clamp(min=0)], torch.zeros((), device=dev))
        assert torch.equal(f.grad[tail], want)
    else:
        hit = out.detach()[mt.clamp(min=0)] == feats.detach()[tail]
        got = f.grad[tail]
        assert bool(((got != 0) <= (hit & (mt >= 0)[:, None])).all())          # gradient only where the point IS the max
        assert torch.equal(got[got != 0], gv[mt.clamp(min=0)][got != 0])
    del f, feats, out, gv
    torch.cuda.empty_cache()


@pytest.mark.gpu
def test_gpu_scatter_all_points_outside_and_single_voxel(host_glue):
    """Edge clouds: every point invalid (no voxel at all), and every point in ONE voxel (the longest possible segment)."""
    from mmdet3d_gaussian_amd.scatter import Scatter
    n, c = 5000, 16
    feats = torch.randn(n, c, device='cuda', requires_grad=True)
    none = Scatter(torch.full((n, 3), -1, dtype=torch.int32, device='cuda'))
    assert none.voxel_coors.shape[0] == 0 and bool((none.pts_voxel_maps == -1).all())
    out, vc = none.reduce(feats, 'max')
    assert out.shape == (0, c) and vc.shape[0] == 0
    back = none.reduce_mapback(feats.detach(), 'mean', default_feat=7.0)
    assert back.shape == (n, c) and bool((back == 7.0).all())
    one = Scatter(torch.tensor([[3, 2, 1]], dtype=torch.int32, device='cuda').expand(n, 3).contiguous())
    assert one.voxel_coors.tolist() == [[3, 2, 1]] and one.voxel_pts_counts.tolist() == [n]
    for red in ('sum', 'mean', 'max'):
        feats.grad = None
        o, _ = one.reduce(feats, red)
        f64 = feats.detach().double()
        want = {'sum': f64.sum(0), 'mean': f64.mean(0), 'max': f64.max(0).values}[red]
        # 5000 fp32 terms added in ascending point order: |error| <~ n * eps * max|partial sum| ~ 2e-3 on the sum
        atol = {'sum': 2e-3, 'mean': 2e-3 / n, 'max': 0.0}[red]
        assert torch.allclose(o[0].double(), want, rtol=1e-6, atol=atol)
        o.sum().backward()
        if red == 'max':
            assert int((feats.grad != 0).sum()) == c                  # exactly one winner per channel
        else:
            assert torch.allclose(feats.grad, torch.full_like(feats, 1.0 if red == 'sum' else 1.0 / n))


@pytest.mark.gpu
@pytest.mark.parametrize('c', [3, 10, 16])
@pytest.mark.parametrize('red', ['sum', 'mean', 'max'])
def test_gpu_narrow_rows_long_runs_and_same_bits_as_the_vector_kernels(host_glue, c, red):
    """Rows that are not whole 16-byte vectors, and narrow rows, on a skewed cloud: three voxels hold 40 % of the points (runs of
    thousands of points), the rest are singletons and small voxels.  The backward here is the node's choice for c < 32, the
    map-ordered gather (max: the fill and max_grad_kernel), NOT the voxel-ordered LDS kernel: its tiles are the business of
    test_gpu_spread_lds_tiles_and_workgroup_sizes.  Every kernel visits a voxel's points in ascending point id: the c channels embedded in the first columns of a
    64-channel array (which takes the 16-byte vector kernels) give bit-identical sums / means / maxima."""
    from mmdet3d_gaussian_amd.scatter import Scatter
    rng = np.random.default_rng(c)
    n = 50_000
    coors = np.stack([rng.integers(0, 60, n), rng.integers(0, 60, n), rng.integers(0, 2, n)], -1).astype(np.int32)
    big = rng.random(n) < 0.4
    coors[big] = np.array([[5, 5, 0], [30, 31, 1], [59, 59, 1]], np.int32)[rng.integers(0, 3, big.sum())]
    coors[rng.random(n) < 0.02, 1] = -1
    feats = rng.normal(0, 1, (n, c)).astype(np.float32)
    wide = np.zeros((n, 64), np.float32); wide[:, :c] = feats
    sc = Scatter(torch.from_numpy(coors).cuda())
    assert int(sc.voxel_pts_counts.max()) > 4000
    f = torch.from_numpy(feats).cuda().requires_grad_(True)
    out, _ = sc.reduce(f, red)
    ref, _ = sc.reduce(torch.from_numpy(wide).cuda(), red)
    assert torch.equal(out.detach(), ref[:, :c].contiguous())
    uo, mo, co = vo.scatter_index(coors)
    want, _ = vo.scatter_reduce(feats, mo, co, red)
    np.testing.assert_allclose(out.detach().cpu().numpy(), want, rtol=1e-4, atol=1e-3)   # fp32 running sums over up to 7 000 points
    gv = torch.randn(out.shape, device='cuda')
    out.backward(gv)
    gw = vo.scatter_backward(gv.cpu().numpy(), feats, mo, co, red)
    np.testing.assert_allclose(f.grad.cpu().numpy(), gw, rtol=2e-6, atol=1e-7)
    assert (f.grad[sc.pts_voxel_maps < 0] == 0).all()


@pytest.mark.gpu
def test_gpu_index_reports_key_overflow_and_out_of_range_coordinates():
    """extents whose product passes 2^63 used to wrap the mixed-radix key (merged voxels, fake dropped points); an
    int64 coordinate beyond int32 used to wrap in the cast.  Both are errors now; a large negative int64 is a dropped point."""
    from mmdet3d_gaussian_amd.scatter import scatter_index
    big = torch.tensor([[2 ** 30, 2 ** 30, 2 ** 30, 5], [1, 2, 3, 4]], dtype=torch.int32, device='cuda')   # product ~ 2^90 x 6
    with pytest.raises(RuntimeError, match='63-bit'):
        scatter_index(big)
    ok = torch.tensor([[2 ** 20, 2 ** 20, 2 ** 20], [1, 2, 3], [1, 2, 3]], dtype=torch.int32, device='cuda')        # 2^60: fits
    vc, pm, cnt = scatter_index(ok)
    assert vc.shape[0] == 2 and pm.tolist() == [1, 0, 0] and cnt.tolist() == [2, 1]
    wide = torch.tensor([[1, 2, 3], [2 ** 40, 0, 0]], dtype=torch.int64, device='cuda')
    with pytest.raises(RuntimeError, match='int32'):
        scatter_index(wide)
    neg = torch.tensor([[1, 2, 3], [-2 ** 40, 0, 0], [1, 2, 3]], dtype=torch.int64, device='cuda')
    vc, pm, cnt = scatter_index(neg)
    assert pm.tolist() == [0, -1, 0] and vc.dtype == torch.int64


@pytest.mark.gpu
def test_gpu_backward_with_its_zero_fill_replays_in_a_hipgraph(host_glue):
    """The arg-max backward at narrow rows clears grad_feats and then routes the voxel gradients: the clear is a KERNEL of the
    library, not a hipMemsetAsync — a memset node of a captured graph was found not to be reliably ordered against the kernels
    around it on this ROCm (round 4, rotated NMS).  Five replays on a poisoned output buffer must equal the eager result; the
    degenerate calls whose whole effect is a clear (no voxels; an empty loss call) are captured alongside."""
    import ctypes
    import mmdet3d_gaussian_amd as amd
    from mmdet3d_gaussian_amd.scatter import Scatter, group_points
    lib = amd.load_library()
    n, c, red = 30000, 10, 2
    coors, feats = _cloud(n, 321, c=c, neg_frac=0.03)
    sc = Scatter(torch.from_numpy(coors).cuda())
    order, seg = group_points(sc.pts_voxel_maps, sc.voxel_pts_counts)
    v = sc.voxel_coors.shape[0]
    f = torch.from_numpy(feats).cuda()
    out = torch.empty(v, c, device='cuda'); arg = torch.empty(v, c, dtype=torch.int32, device='cuda')
    assert lib.vox_scatter_reduce(f.data_ptr(), order.data_ptr(), seg.data_ptr(), n, c, v, red, out.data_ptr(), arg.data_ptr(), None) == 0
    gv = torch.randn(v, c, device='cuda')
    want = torch.full((n, c), float('nan'), device='cuda')
    assert lib.vox_scatter_backward(gv.data_ptr(), sc.pts_voxel_maps.data_ptr(), sc.voxel_pts_counts.data_ptr(), arg.data_ptr(), n, c, v,
                                    red, want.data_ptr(), None) == 0
    got = torch.full((n, c), float('nan'), device='cuda')
    none = torch.full((64, c), float('nan'), device='cuda')          # a call with v == 0: its whole effect is the clear
    lsum = torch.full((1,), float('nan'), device='cuda')             # gd3d_loss_reduce with n == 0: writes 0
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        s = ctypes.c_void_p(side.cuda_stream)
        with torch.cuda.graph(graph, stream=side):
            assert lib.vox_scatter_backward(gv.data_ptr(), sc.pts_voxel_maps.data_ptr(), sc.voxel_pts_counts.data_ptr(), arg.data_ptr(),
                                            n, c, v, red, got.data_ptr(), s) == 0
            assert lib.vox_scatter_backward(gv.data_ptr(), sc.pts_voxel_maps.data_ptr(), sc.voxel_pts_counts.data_ptr(), None,
                                            64, c, 0, 0, none.data_ptr(), s) == 0
            assert lib.gd3d_loss_reduce(None, 0, lsum.data_ptr(), s) == 0
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(5):
        got.fill_(float('nan')); none.fill_(float('nan')); lsum.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(got, want)
        assert (none == 0).all() and lsum.item() == 0.0


# ---- the dispatch paths of csrc/voxel_scatter.hip, case by case (tests/voxel_scatter_cases.py) ------------------------------------------

import voxel_scatter_cases as vc  # noqa: E402

_ID = lambda k: k.id if isinstance(k, vc.Case) else None
RED = vc.REDS.index
F_GUARD, I_GUARD, BAND = -77.0, -7, 64        # sentinels no result can equal (arg max >= -1), guard elements either side


@pytest.mark.parametrize('case', vc.ALL_CASES, ids=_ID)
def test_case_table_reaches_the_paths_it_names(case):
    """every case's predicate, from its own sizes and the oracle's index: the kernel, the index form, the voxels per workgroup and the
    tile starts it is in the table for; dropped points and a voxel of several points in every cloud, a run beyond one tile in the long ones"""
    assert vc.reaches(case) == []


def test_case_table_notices_a_size_that_misses_its_path(monkeypatch):
    """the same predicates on sizes one step off: n = 4103 takes the multiply-high, n = 4106 is no longer the first division, 67 000
    voxels of 31 channels fit one sweep, a cloud of short runs has one tile per workgroup"""
    monkeypatch.setitem(vc.CLOUDS, 'off_4103', lambda: vc._uniform(1, 4103, 300))
    monkeypatch.setitem(vc.CLOUDS, 'off_4106', lambda: vc._uniform(1, 4106, 300))
    for case in vc.DIV_CASES:
        assert vc.reaches(case._replace(cloud='off_4103')) and vc.reaches(case._replace(cloud='off_4106'))
    assert vc.reaches(vc.SWEEP_CASE._replace(c=30)) and vc.reaches(vc.SWEEP_CASE._replace(c=32))
    assert vc.reaches(vc.LDS_CASES[0]._replace(cloud='wide')) and vc.reaches(vc.LDS_CASES[0]._replace(c=4))
    assert vc.reaches(vc.WIDE_CASES[0]._replace(c=128)) and vc.reaches(vc.WIDE_CASES[3]._replace(c=256))
    assert vc.reaches(vc.MISALIGNED_CASE._replace(c=66)) and vc.reaches(vc.GUARD_CASES[0]._replace(cloud='lds_c'))


def test_nonfinite_plants_as_the_oracle_sees_them():
    """what the non-finite cloud holds, by the oracle alone: a voxel-channel of NaN reduces to -inf and routes no gradient; one of -inf
    (also behind a leading NaN) gives its gradient to its smallest -inf point (the reference's trace-back is an equality test); +inf
    ties go to the first +inf; a NaN among finite values changes nothing"""
    for case in vc.NONFINITE_CASES:
        c = case.c
        _, _, mo, co = vc.cloud(case.cloud)
        feats, want, where = vc.inputs(case.cloud, c), vc.expected(case.cloud, c, 'max'), vc.plants(c)
        pts = lambda v: np.flatnonzero(mo == v)
        v, ch = where['all_nan']
        assert np.isnan(feats[pts(v), ch]).all() and want['out'][v, ch] == -np.inf and (want['grad'][pts(v), ch] == 0).all()
        v, ch = where['all_ninf']
        assert (feats[pts(v), ch] == -np.inf).all() and want['out'][v, ch] == -np.inf
        assert want['grad'][pts(v)[0], ch] == want['gv'][v, ch] != 0 and (want['grad'][pts(v)[1:], ch] == 0).all()
        v, ch = where['nan_then_ninf']
        assert np.isnan(feats[pts(v)[0], ch]) and want['grad'][pts(v)[0], ch] == 0 and want['grad'][pts(v)[1], ch] == want['gv'][v, ch]
        v, ch = where['inf_ties']
        assert want['out'][v, ch] == np.inf and want['grad'][pts(v)[1], ch] == want['gv'][v, ch] and (want['grad'][pts(v)[2:], ch] == 0).all()
        assert np.isnan(feats[:, 4:]).sum() > 100 and not np.isnan(want['out']).any() and np.isfinite(want['grad']).all()


_DEVICE = {}


def _gpu(a):
    """a frozen array of the case table as a device tensor of its own"""
    return torch.tensor(a, device='cuda')


def _on_gpu(name):
    """the cloud's Scatter (its index checked against the oracle's once) and the grouping the C entry points take"""
    if name not in _DEVICE:
        from mmdet3d_gaussian_amd.scatter import Scatter
        coors, uo, mo, co = vc.cloud(name)
        sc = Scatter(_gpu(coors))
        np.testing.assert_array_equal(sc.voxel_coors.cpu().numpy(), uo)
        np.testing.assert_array_equal(sc.pts_voxel_maps.cpu().numpy(), mo)
        np.testing.assert_array_equal(sc.voxel_pts_counts.cpu().numpy(), co)
        _DEVICE[name] = (sc,) + tuple(sc._grouping)
    return _DEVICE[name]


def _shifted(t):
    """the same values in a contiguous view that starts 4 bytes past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    view = buf[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_forward(got, want, red, what):
    """max: the oracle's bits.  sum / mean: the sequential-summation bound of the case (voxel_scatter_cases.expected), per element;
    the largest error / bound ratio is printed, the bound itself is derived and not tuned"""
    got = got.detach().cpu().numpy()
    if red == 'max':
        np.testing.assert_array_equal(_bits(got), _bits(want['out']), err_msg=what)
        return
    err = np.abs(got.astype(np.float64) - want['out'])
    pos = want['bound'] > 0
    print(f'SUMBOUND {what} {red}: largest error / bound = {(err[pos] / want["bound"][pos]).max():.4f}')
    assert (err <= want['bound']).all(), (what, float((err - want['bound']).max()))


def _check_backward(got, want, red, what):
    """sum and max: copies of grad_vox rows or zeros, the oracle's bits.  mean: one fp32 division against fp64"""
    if red == 'mean':
        np.testing.assert_allclose(got.detach().cpu().numpy(), want['grad'], rtol=2e-6, atol=1e-7, err_msg=what)
    else:
        np.testing.assert_array_equal(_bits(got), _bits(want['grad']), err_msg=what)


def _through_the_node(case, red, shift=False):
    sc = _on_gpu(case.cloud)[0]
    want = vc.expected(case.cloud, case.c, red)
    f = _gpu(vc.inputs(case.cloud, case.c))
    f = (_shifted(f) if shift else f).requires_grad_(True)
    out, _ = sc.reduce(f, red)
    _check_forward(out, want, red, case.id)
    out.backward(_gpu(want['gv']))
    _check_backward(f.grad, want, red, case.id)
    return sc, f, out.detach(), want


def _forward(case, red, out=None, arg=None, feats=None):
    """vox_scatter_reduce on the case's cloud -> (out, arg max | None)"""
    import mmdet3d_gaussian_amd as amd
    lib = amd.load_library()
    sc, order, seg = _on_gpu(case.cloud)
    n, c, v = sc.pts_voxel_maps.numel(), case.c, sc.voxel_coors.shape[0]
    f = _gpu(vc.inputs(case.cloud, c)) if feats is None else feats
    out = torch.full((v, c), float('nan'), device='cuda') if out is None else out
    if red == 'max' and arg is None:
        arg = torch.full((v, c), I_GUARD, dtype=torch.int32, device='cuda')
    assert lib.vox_scatter_reduce(f.data_ptr(), order.data_ptr(), seg.data_ptr(), n, c, v, RED(red), out.data_ptr(),
                                  arg.data_ptr() if red == 'max' else None, None) == 0
    return out, (arg if red == 'max' else None)


def _backward(case, red, gv, arg, grouped, gf=None):
    """vox_scatter_backward | vox_scatter_backward_grouped into a NaN-poisoned (or the given) buffer -> (return code, grad_feats)"""
    import mmdet3d_gaussian_amd as amd
    lib = amd.load_library()
    sc, order, seg = _on_gpu(case.cloud)
    n, c, v = sc.pts_voxel_maps.numel(), case.c, sc.voxel_coors.shape[0]
    gf = torch.full((n, c), float('nan'), device='cuda') if gf is None else gf
    am = arg.data_ptr() if red == 'max' else None
    if grouped:
        rc = lib.vox_scatter_backward_grouped(gv.data_ptr(), order.data_ptr(), seg.data_ptr(), am, n, c, v, RED(red), gf.data_ptr(), None)
    else:
        rc = lib.vox_scatter_backward(gv.data_ptr(), sc.pts_voxel_maps.data_ptr(), sc.voxel_pts_counts.data_ptr(), am, n, c, v, RED(red),
                                      gf.data_ptr(), None)
    torch.cuda.synchronize()
    return rc, gf


def _banded(shape, dtype):
    """a sentinel-filled buffer and the view of `shape` inside it, BAND elements from either end (16-byte aligned, as the buffer is)"""
    numel = int(np.prod(shape))
    buf = torch.full((numel + 2 * BAND,), F_GUARD if dtype == torch.float32 else I_GUARD, dtype=dtype, device='cuda')
    inner = buf[BAND:BAND + numel].view(shape)
    assert inner.data_ptr() % 16 == 0
    return buf, inner


def _bands_intact_and_inside_written(buf, what):
    guard = F_GUARD if buf.dtype == torch.float32 else I_GUARD
    assert (buf[:BAND] == guard).all() and (buf[-BAND:] == guard).all(), f'{what}: a guard band was written'
    assert (buf[BAND:-BAND] != guard).all(), f'{what}: an element inside was not written'


@pytest.mark.gpu
@pytest.mark.parametrize('red', vc.REDS)
@pytest.mark.parametrize('case', vc.DIV_CASES, ids=_ID)
def test_gpu_gather_index_by_division_and_by_the_last_exact_multiply_high(host_glue, case, red):
    """gather_grad_kernel turns a flat index into (point, lane) with a shift, ONE multiply-high, or — from n * cv >= floor(2^32 / cv) on —
    a 64-bit division.  cv = 1023 lanes a row, scalar (c = 1023) and vector (c = 4092): n = 4105 is the first size that divides,
    n = 4104 the last that multiplies, so its last rows are the hardest indices of that form.  Forward (the scalar multi-pass kernel)
    and backward through the node against the fp64 oracle."""
    _through_the_node(case, red)


@pytest.mark.gpu
def test_gpu_max_backward_beyond_one_sweep_of_its_capped_grid(host_glue):
    """max_grad_kernel's grid stops at 8192 workgroups: with 68 000 voxels of 31 channels the grid-stride loop goes round again, and
    the voxels of the second sweep get their gradient only there.  72 000 points with exact ties for the max and dropped points;
    forward and backward are exact."""
    _through_the_node(vc.SWEEP_CASE, 'max')


@pytest.mark.gpu
@pytest.mark.parametrize('red', vc.REDS)
@pytest.mark.parametrize('case', vc.LDS_CASES, ids=_ID)
def test_gpu_spread_lds_tiles_and_workgroup_sizes(case, red):
    """spread_lds_kernel called directly (the node never picks it): workgroups shrunk by lds_plan's run-length term, by 512 / c, to ONE
    voxel and at the cap of 128; runs of several 1024-point tiles whose boundaries fall inside a voxel and exactly between two.  The same
    bits as the map-ordered backward on NaN-poisoned buffers, zero rows for the dropped points, and the fp64 oracle's gradient."""
    want = vc.expected(case.cloud, case.c, red)
    _, arg = _forward(case, red)
    gv = _gpu(want['gv'])
    rc_a, a = _backward(case, red, gv, arg, grouped=False)
    rc_b, b = _backward(case, red, gv if case.aligned else _shifted(gv), arg, grouped=True)
    assert rc_a == 0 and rc_b == 0
    assert not torch.isnan(b).any() and torch.equal(a, b)
    assert (b[_on_gpu(case.cloud)[0].pts_voxel_maps < 0] == 0).all()
    _check_backward(b, want, red, case.id)


@pytest.mark.gpu
@pytest.mark.parametrize('red', vc.REDS)
@pytest.mark.parametrize('case', vc.WIDE_CASES, ids=_ID)
def test_gpu_rows_wider_than_128_channels_through_the_node(host_glue, case, red):
    """128 < c <= 256 with c % 4 == 0: one voxel per wave in reduce_v4_kernel and spread_grad_v4_kernel, the lanes beyond c / 4 idle;
    c = 260: the scalar multi-pass forward and the vector gather at 65 lanes a row.  Against the oracle, and — every kernel visits a
    voxel's points in ascending id — the same bits as the same channels in a (c + 1)-wide array on the scalar path."""
    sc, f, out, _ = _through_the_node(case, red)
    if case.c <= vc.VEC_C_MAX:
        wide = torch.zeros((f.shape[0], case.c + 1), device='cuda')
        wide[:, :case.c] = f.detach()
        ref, _ = sc.reduce(wide, red)
        assert torch.equal(out, ref[:, :case.c].contiguous())


@pytest.mark.gpu
@pytest.mark.parametrize('red', vc.REDS)
@pytest.mark.parametrize('case', vc.WIDE_CASES, ids=_ID)
def test_gpu_rows_wider_than_128_channels_both_backward_entries(case, red):
    """the two backward entry points on the wide rows: the vector gather at 33 .. 65 lanes a row against the oracle; the voxel-ordered
    form bit-equal to it where it accepts the shape (c <= 256), GD3D_E_BADARG and nothing written at c = 260"""
    want = vc.expected(case.cloud, case.c, red)
    out, arg = _forward(case, red)
    _check_forward(out, want, red, case.id)
    gv = _gpu(want['gv'])
    rc_a, a = _backward(case, red, gv, arg, grouped=False)
    rc_b, b = _backward(case, red, gv, arg, grouped=True)
    assert rc_a == 0
    _check_backward(a, want, red, case.id)
    if case.c <= vc.VEC_C_MAX:
        assert rc_b == 0 and torch.equal(a, b)
    else:
        assert rc_b == vc.BADARG and torch.isnan(b).all()


@pytest.mark.gpu
@pytest.mark.parametrize('red', vc.REDS)
def test_gpu_features_four_bytes_off_alignment_through_the_node(host_glue, red):
    """a contiguous (n, 64) view that starts 4 bytes into its buffer: the forward must leave the 16-byte kernels for the scalar one
    (same visiting order, same bits as the aligned run), and the gradient comes back the same"""
    case = vc.MISALIGNED_CASE
    _, f0, out0, _ = _through_the_node(case, red)
    _, f1, out1, _ = _through_the_node(case, red, shift=True)
    assert f1.data_ptr() % 16 == 4 and f0.data_ptr() % 16 == 0
    assert torch.equal(out0, out1) and torch.equal(f0.grad, f1.grad)


@pytest.mark.gpu
@pytest.mark.parametrize('red', vc.REDS)
def test_gpu_gradient_four_bytes_off_alignment_at_the_entry_points(red):
    """a misaligned grad_vox, which the node's own copy never produces: the map-ordered backward falls back to the dword gather, the
    voxel-ordered one to spread_lds_kernel at c = 64 — both with the aligned run's bits — and returns GD3D_E_BADARG at c = 132, where
    it has no dword form, without writing anything; a misaligned grad_feats takes the same fallbacks"""
    case = vc.MISALIGNED_CASE
    want = vc.expected(case.cloud, case.c, red)
    _, arg = _forward(case, red)
    gv = _gpu(want['gv'])
    rc, aligned = _backward(case, red, gv, arg, grouped=False)
    assert rc == 0
    _check_backward(aligned, want, red, case.id)
    for grouped in (False, True):
        rc, got = _backward(case, red, _shifted(gv), arg, grouped)
        assert rc == 0 and torch.equal(got, aligned), grouped
        rc, got = _backward(case, red, gv, arg, grouped, gf=_shifted(torch.full_like(aligned, float('nan'))))
        assert rc == 0 and torch.equal(got, aligned), grouped
    bad = vc.MISALIGNED_BADARG
    want = vc.expected(bad.cloud, bad.c, red)
    _, arg = _forward(bad, red)
    gv = _gpu(want['gv'])
    rc, got = _backward(bad, red, _shifted(gv), arg, grouped=True)
    assert rc == vc.BADARG and torch.isnan(got).all()
    rc, got = _backward(bad, red, _shifted(gv), arg, grouped=False)
    assert rc == 0
    _check_backward(got, want, red, bad.id)


@pytest.mark.gpu
@pytest.mark.parametrize('red', vc.REDS)
@pytest.mark.parametrize('case', vc.GUARD_CASES, ids=_ID)
def test_gpu_nothing_is_written_beyond_out_argmax_and_grad_feats(case, red):
    """the three C entry points on sentinel-filled buffers with a guard band either side of out, argmax and grad_feats, at v = 1237 and
    n = 4999 (no multiple of any per-wave or per-workgroup count): float4 / int4 and nontemporal stores at computed row offsets, the
    fill + max_grad_kernel route (max, c = 10) and spread_lds_kernel (grouped, c = 10) among them.  Every element inside is written,
    no guard is touched, and the values are the oracle's."""
    want = vc.expected(case.cloud, case.c, red)
    v, n = want['out'].shape[0], want['grad'].shape[0]
    obuf, out = _banded((v, case.c), torch.float32)
    abuf, arg = _banded((v, case.c), torch.int32)
    _forward(case, red, out=out, arg=arg)
    torch.cuda.synchronize()
    _bands_intact_and_inside_written(obuf, 'out')
    if red == 'max':
        _bands_intact_and_inside_written(abuf, 'argmax')
    else:
        assert (abuf == I_GUARD).all()
    _check_forward(out, want, red, case.id)
    gv = _gpu(want['gv'])
    for grouped in (False, True):
        gbuf, gf = _banded((n, case.c), torch.float32)
        rc, _ = _backward(case, red, gv, arg, grouped, gf=gf)
        assert rc == 0
        _bands_intact_and_inside_written(gbuf, f'grad_feats, grouped={grouped}')
        _check_backward(gf, want, red, case.id)


@pytest.mark.gpu
@pytest.mark.parametrize('case', vc.NONFINITE_CASES, ids=_ID)
def test_gpu_max_of_nan_and_infinite_features(case):
    """NaN among finite values, a voxel-channel of NaN (reduces to -inf, arg max -1, no gradient: the rows a missing guard would store
    at point -1, into the band in front of grad_feats), a voxel-channel of -inf (the reference's equality trace-back gives the gradient
    to its smallest point id, and so does the tie rule of the reduce kernels), +inf ties: the oracle's bits forward, and backward on
    every route — fill + max_grad_kernel, the voxel-ordered vector kernel (c = 16) or LDS kernel (c = 10), and the LDS kernel by way
    of a misaligned gradient — inside guard bands"""
    want = vc.expected(case.cloud, case.c, 'max')
    v, n = want['out'].shape[0], want['grad'].shape[0]
    obuf, out = _banded((v, case.c), torch.float32)
    abuf, arg = _banded((v, case.c), torch.int32)
    _forward(case, 'max', out=out, arg=arg)
    torch.cuda.synchronize()
    _bands_intact_and_inside_written(obuf, 'out')
    _bands_intact_and_inside_written(abuf, 'argmax')
    _check_forward(out, want, 'max', case.id)
    where = vc.plants(case.c)
    at = lambda k: int(arg[int(where[k][0]), where[k][1]])
    assert at('all_nan') == -1 and at('all_ninf') >= 0 and at('nan_then_ninf') >= 0
    gv = _gpu(want['gv'])
    for grouped, g in ((False, gv), (True, gv), (True, _shifted(gv))):
        gbuf, gf = _banded((n, case.c), torch.float32)
        rc, _ = _backward(case, 'max', g, arg, grouped, gf=gf)
        assert rc == 0
        _bands_intact_and_inside_written(gbuf, f'grad_feats, grouped={grouped}')
        _check_backward(gf, want, 'max', case.id)


@pytest.mark.gpu
@pytest.mark.parametrize('case', vc.NONFINITE_CASES, ids=_ID)
def test_gpu_max_of_nan_and_infinite_features_through_the_node(host_glue, case):
    _through_the_node(case, 'max')
