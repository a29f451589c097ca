"""The voxel-set-abstraction ops without a GPU: the `_cpu` twins of csrc/vsa_cpu.cpp (what CPU tensors take) against the numpy
oracle tests/vsa_ref.py with EXACT equality on idx, cnt, the empty-ball mask, the FPS picks and the grouped output; autograd of
`grouping` and `QueryAndGroup` against an fp64 index-select restatement; the argument errors."""
import numpy as np
import pytest
import torch

import mmdet3d_gaussian_amd as amd
import vsa_cases as cases
import vsa_ref


def _t(*arrays):
    return [torch.from_numpy(np.array(a)) for a in arrays]


def _forward(xyz, pc, new_xyz, qc, feats, radius, nsample, c, use_xyz):
    f = None if c == 0 else feats[:, :c].contiguous()
    out, idx = amd.QueryAndGroup(radius, nsample, use_xyz=use_xyz)(xyz, pc, new_xyz, qc, f)
    bidx, mask, cnt = amd.ball_query(radius, nsample, xyz, pc, new_xyz, qc, return_cnt=True)
    assert torch.equal(idx, bidx)          # the fused launch and the stand-alone query are one scan
    return out, idx, cnt, mask


def _check_forward(kind, name, radius, nsample, c, use_xyz):
    xyz, pc, new_xyz, qc, feats = _t(*cases.inputs(kind, name))
    out, idx, cnt, mask = _forward(xyz, pc, new_xyz, qc, feats, radius, nsample, c, use_xyz)
    r_out, r_idx, r_cnt, r_mask = cases.reference(kind, name, radius, nsample, c, use_xyz)
    assert idx.dtype == torch.int32 and mask.dtype == torch.bool and cnt.dtype == torch.int32 and out.dtype == torch.float32
    assert np.array_equal(idx.numpy(), r_idx) and np.array_equal(cnt.numpy(), r_cnt) and np.array_equal(mask.numpy(), r_mask)
    assert out.shape == r_out.shape and np.array_equal(out.numpy(), r_out)
    if c:   # the stand-alone grouping is the same gather; in a sample WITHOUT points no index is in range: it writes zeros
        g = amd.grouping(feats[:, :c].contiguous(), pc, idx, qc).numpy()
        has_points = (pc.numpy() > 0)[vsa_ref.sample_of_rows(qc.numpy())]
        ref = vsa_ref.grouping(np.concatenate([feats[:, :c].numpy(), np.zeros((1, c), np.float32)]), pc.numpy(), r_idx, qc.numpy())
        assert np.array_equal(g[has_points], ref[has_points]) and not g[~has_points].any()
    return r_cnt


@pytest.mark.parametrize('nsample', [1, 5, 16, 32])
@pytest.mark.parametrize('name', sorted(cases.STACKS))
def test_twin_matches_oracle_on_stacked_batches(name, nsample):
    """dense balls (radius 0.9: more members than nsample -> the early stop) and sparse ones (0.25: padded tails), empty balls, a
    sample without points, one without queries"""
    dense = _check_forward('stack', name, 0.9, nsample, 3, True)
    sparse = _check_forward('stack', name, 0.25, nsample, 3, True)
    assert (dense == 0).any() and (name.startswith('small') or (dense == nsample).any())
    if nsample >= 5:
        assert ((sparse > 0) & (sparse < nsample)).any()


@pytest.mark.parametrize('c,use_xyz', [(0, True)] + [(c, u) for c in (1, 3, 16, 17, 64, 67) for u in (True, False)])
def test_twin_matches_oracle_over_channel_counts(c, use_xyz):
    """c = 0: features=None (which needs use_xyz=True)"""
    _check_forward('stack', 'tile+1_nopoints_64', 0.6, 16, c, use_xyz)


@pytest.mark.parametrize('nsample', [1, 5, 16, 32])
@pytest.mark.parametrize('members', [4, 5, 6, 16, 32, 33, 40])
def test_exactly_nsample_members_and_boundary_straddlers(members, nsample):
    """balls with fewer members than nsample, exactly nsample, and more, the members lying either side of the 64-point step and of
    the tile boundary: stopping early must not change idx, cnt or the tail"""
    cnt = _check_forward('crafted', '', cases.crafted_radius(members), nsample, 16, True)
    assert cnt[0] == min(members, nsample) and cnt[-1] == 0


@pytest.mark.parametrize('nsample', cases.WIDE_NSAMPLE)
def test_twin_matches_oracle_above_one_wave_of_slots(nsample):
    """nsample 33 to 1024 (vsa_cases.WIDE_NSAMPLE) on 2300, 700 and 0 points: balls that fill two tiles after their first member,
    padded tails of 1 to 990 slots, empty balls"""
    for radius in (cases.R_ALL, cases.R_MID):
        want = cases.wide_conditions(radius, nsample)
        assert np.array_equal(_check_forward('wide', '', radius, nsample, 3, True), want)


@pytest.mark.parametrize('c,use_xyz', [(0, True)] + [(c, u) for c in (1, 17, 67) for u in (True, False)])
@pytest.mark.parametrize('nsample', [64, 128, 1024])
def test_twin_matches_oracle_over_channel_counts_at_large_nsample(nsample, c, use_xyz):
    for radius in (cases.R_ALL, cases.R_MID):
        cases.wide_conditions(radius, nsample)
        _check_forward('wide', '', radius, nsample, c, use_xyz)


def test_point_at_exactly_the_radius_is_excluded():
    xyz, pc, new_xyz, qc = _t(*cases.exact_radius())
    idx, mask, cnt = amd.ball_query(5.0, 8, xyz, pc, new_xyz, qc, return_cnt=True)
    assert idx[0].tolist() == [1, 2, 1, 1, 1, 1, 1, 1] and cnt.tolist() == [2, 0] and mask.tolist() == [False, True]
    r_idx, r_cnt, r_mask = vsa_ref.ball_query(5.0, 8, xyz.numpy(), pc.numpy(), new_xyz.numpy(), qc.numpy())
    assert np.array_equal(idx.numpy(), r_idx) and np.array_equal(cnt.numpy(), r_cnt)
    # d2 == radius2 exactly for rows 0, 3, 4, 5 of the sample: the contract's strict <
    assert (vsa_ref.dist2(new_xyz[0].numpy(), xyz.numpy())[[0, 3, 4, 5]] == np.float32(25)).all()


def _index_select_restatement(xyz, pc, new_xyz, qc, feats, idx, mask, use_xyz):
    """QueryAndGroup from torch index ops in fp64, differentiable wrt feats"""
    start = torch.from_numpy(vsa_ref.starts(pc.numpy())[vsa_ref.sample_of_rows(qc.numpy())])
    rows = (start[:, None] + idx.long()).reshape(-1)
    m, ns = idx.shape
    g = feats.index_select(0, rows).reshape(m, ns, -1).permute(0, 2, 1)
    if use_xyz:
        gx = xyz.double().index_select(0, rows).reshape(m, ns, 3).permute(0, 2, 1) - new_xyz.double()[:, :, None]
        g = torch.cat([gx, g], 1)
    return g * (~mask)[:, None, None]


@pytest.mark.parametrize('use_xyz', [True, False])
def test_query_and_group_autograd_on_cpu(use_xyz):
    """integer upstream gradients: every sum is exact in fp32 in any order, so the gradient equals the fp64 restatement's bit for
    bit; many queries share one centre, tails are padded, empty balls pass nothing"""
    xyz, pc, new_xyz, qc = _t(*cases.duplication())
    rng = np.random.RandomState(0)
    feats = torch.from_numpy(rng.uniform(-1, 1, (xyz.shape[0], 5)).astype(np.float32)).requires_grad_()
    out, idx = amd.QueryAndGroup(0.5, 16, use_xyz=use_xyz)(xyz, pc, new_xyz, qc, feats)
    _, mask, cnt = amd.ball_query(0.5, 16, xyz, pc, new_xyz, qc, return_cnt=True)
    assert mask.sum() == 3 and ((cnt > 0) & (cnt < 16)).any() and not idx.requires_grad
    gout = torch.from_numpy(rng.randint(-8, 9, tuple(out.shape)).astype(np.float32))
    grad, = torch.autograd.grad(out, feats, gout)
    f64 = feats.detach().double().requires_grad_()
    ref = _index_select_restatement(xyz, pc, new_xyz, qc, f64, idx, mask, use_xyz)
    assert torch.equal(ref.detach().float(), out.detach())
    rgrad, = torch.autograd.grad(ref, f64, gout.double())
    assert torch.equal(grad.double(), rgrad)
    c_off = 3 if use_xyz else 0
    o_grad, _, _ = vsa_ref.grouping_backward(gout.numpy()[:, c_off:], idx.numpy(), qc.numpy(), pc.numpy(), xyz.shape[0], ~mask.numpy())
    assert np.array_equal(grad.numpy().astype(np.float64), o_grad)


def test_grouping_autograd_on_cpu():
    xyz, pc, new_xyz, qc, feats = _t(*cases.stack('63_tile-1_noqueries'))
    idx, _ = amd.ball_query(0.9, 5, xyz, pc, new_xyz, qc)
    f = feats[:, :17].clone().requires_grad_()
    out = amd.grouping(f, pc, idx, qc)
    gout = torch.from_numpy(np.random.RandomState(1).randint(-8, 9, tuple(out.shape)).astype(np.float32))
    grad, = torch.autograd.grad(out, f, gout)
    o_grad, _, _ = vsa_ref.grouping_backward(gout.numpy(), idx.numpy(), qc.numpy(), pc.numpy(), xyz.shape[0])
    assert np.array_equal(grad.numpy().astype(np.float64), o_grad)
    f64 = f.detach().double().requires_grad_()
    assert torch.autograd.gradcheck(lambda t: amd.grouping(t.float(), pc, idx, qc).double(), (f64,), eps=1e-2, atol=1e-3,
                                    nondet_tol=0.0, fast_mode=True)


@pytest.mark.parametrize('c', [1, 17])
@pytest.mark.parametrize('nsample', [65, 128, 701, 1024])
def test_backward_is_exact_on_integer_gradients_at_large_nsample(nsample, c):
    """every point of the sample a member: full balls of up to 1024 slots in sample 0, in sample 1 (700 points) a tail of 1 slot at
    nsample 701 and of 324 at 1024.  At most 12 * 1024 integers of magnitude <= 8 meet in one sum: exact in fp32 in any order."""
    want_cnt = cases.wide_conditions(cases.R_ALL, nsample)
    assert (want_cnt[7:10] == min(700, nsample)).all()
    xyz, pc, new_xyz, qc, feats = _t(*cases.wide())
    _, r_idx, _, r_mask = cases.reference('wide', '', cases.R_ALL, nsample, 0, True)
    gout = np.random.RandomState(1000 * c + nsample).randint(-8, 9, (new_xyz.shape[0], 3 + c, nsample)).astype(np.float32)
    f = feats[:, :c].contiguous().requires_grad_()
    out, idx = amd.QueryAndGroup(cases.R_ALL, nsample)(xyz, pc, new_xyz, qc, f)
    assert np.array_equal(idx.numpy(), r_idx)
    grad, = torch.autograd.grad(out, f, torch.from_numpy(gout))
    n = xyz.shape[0]
    want, _, _ = vsa_ref.grouping_backward(gout[:, 3:], r_idx, qc.numpy(), pc.numpy(), n, ~r_mask)
    assert np.abs(want).max() > 8 and np.array_equal(grad.numpy().astype(np.float64), want)
    f2 = f.detach().clone().requires_grad_()
    g2, = torch.autograd.grad(amd.grouping(f2, pc, idx, qc), f2, torch.from_numpy(gout[:, 3:].copy()))
    want2, _, _ = vsa_ref.grouping_backward(gout[:, 3:], r_idx, qc.numpy(), pc.numpy(), n)
    assert not np.array_equal(want2, want) and np.array_equal(g2.numpy().astype(np.float64), want2)


def test_backward_with_normal_gradients_stays_inside_the_rounding_bound_at_nsample_128():
    """An fp32 sum of k terms taken in any order differs from the exact sum by at most k * 2^-24 * sum|terms|; k and the sum come
    from the oracle, nothing is measured.  Full balls, and tails of 3 to 94 slots."""
    xyz, pc, new_xyz, qc, feats = _t(*cases.wide())
    for radius in (cases.R_MID, cases.R_ALL):
        cases.wide_conditions(radius, 128)
        _, r_idx, _, r_mask = cases.reference('wide', '', radius, 128, 0, True)
        gout = np.random.RandomState(17128).standard_normal((new_xyz.shape[0], 20, 128)).astype(np.float32)
        f = feats[:, :17].contiguous().requires_grad_()
        out, _ = amd.QueryAndGroup(radius, 128)(xyz, pc, new_xyz, qc, f)
        grad, = torch.autograd.grad(out, f, torch.from_numpy(gout))
        want, num, mag = vsa_ref.grouping_backward(gout[:, 3:], r_idx, qc.numpy(), pc.numpy(), xyz.shape[0], ~r_mask)
        err = np.abs(grad.numpy().astype(np.float64) - want)
        assert num.max() >= 6 and (err <= num[:, None] * 2.0 ** -24 * mag).all()
        assert (grad.numpy()[num == 0] == 0).all()


def test_nsample_above_the_limit_is_refused_by_the_twins():
    """GD3D_E_TOOLARGE from every `_cpu` entry point that takes nsample, as from its device twin"""
    from mmdet3d_gaussian_amd import _lib
    xyz, pc, new_xyz, qc, feats = _t(*cases.stack('small_1_64_65'))
    with pytest.raises(RuntimeError, match='nsample'):
        amd.QueryAndGroup(0.5, 1025)
    with pytest.raises(RuntimeError, match='nsample'):
        amd.ball_query(0.5, 1025, xyz, pc, new_xyz, qc)
    with pytest.raises(RuntimeError, match='nsample'):
        amd.grouping(feats, pc, torch.zeros((new_xyz.shape[0], 1025), dtype=torch.int32), qc)
    lib = _lib.load()
    n, m, c, ns, b = xyz.shape[0], new_xyz.shape[0], 2, 1025, 3
    f = feats[:, :c].contiguous()
    out, idx = torch.zeros((m, 3 + c, ns)), torch.zeros((m, ns), dtype=torch.int32)
    cnt, mask, grad = torch.zeros((m,), dtype=torch.int32), torch.zeros((m,), dtype=torch.bool), torch.zeros((n, c))
    p = lambda t: t.data_ptr()
    too_large = 10002
    assert lib.gd3d_vsa_query_and_group_cpu(p(xyz), p(pc), p(new_xyz), p(qc), p(f), b, n, m, c, 0.5, ns, 1, p(out), p(idx), p(cnt),
                                            p(mask), 0) == too_large
    assert lib.gd3d_vsa_ball_query_cpu(p(xyz), p(pc), p(new_xyz), p(qc), b, n, m, 0.5, ns, p(idx), p(cnt), p(mask), 0) == too_large
    assert lib.gd3d_vsa_group_cpu(p(f), p(pc), p(idx), p(qc), b, n, m, c, ns, p(out), 0) == too_large
    assert lib.gd3d_vsa_group_backward_cpu(p(out), p(idx), p(qc), p(pc), b, n, m, c, ns, p(grad)) == too_large
    assert lib.gd3d_vsa_query_and_group_backward_cpu(p(out), p(idx), p(cnt), p(qc), p(pc), b, n, m, c, ns, 3, p(grad)) == too_large
    assert not out.any() and not idx.any() and not grad.any()


def test_other_dtypes_are_evaluated_in_fp32_and_cast_back():
    xyz, pc, new_xyz, qc, feats = _t(*cases.stack('63_tile-1_noqueries'))
    f16 = feats[:, :3].half()
    out, idx = amd.QueryAndGroup(0.9, 5)(xyz.double(), pc.long(), new_xyz.double(), qc.long(), f16)
    ref, ridx = amd.QueryAndGroup(0.9, 5)(xyz, pc, new_xyz, qc, f16.float())
    assert out.dtype == torch.float16 and torch.equal(idx, ridx) and torch.equal(out, ref.half())


def test_fps_twin_matches_oracle():
    """sizes 1, 2, 63, 64, 65, 1024, 1025 and either side of the kernels' register capacity, an empty sample; npoint below and
    above the sample sizes in one call (wrap-around)"""
    xyz, cnt = _t(*cases.fps_cloud())
    for npoint in (1, 7):
        got = amd.furthest_point_sample_stacked(xyz, cnt, npoint)
        assert got.dtype == torch.int64 and np.array_equal(got.numpy(), cases.fps_reference(npoint))
    small = int(np.sum(cases.FPS_SIZES[:7]))      # the seven small samples with npoint = 2048: n picks, then cyclic
    got = amd.furthest_point_sample_stacked(xyz[:small], cnt[:7], 2048)
    ref = vsa_ref.fps_stacked(xyz[:small].numpy(), cnt[:7].numpy(), 2048)
    assert np.array_equal(got.numpy(), ref)
    assert got[3, :64].sort().values.tolist() == list(range(64)) and torch.equal(got[3, 64:128], got[3, :64])


def test_fps_lowest_index_wins_exact_ties():
    xyz, cnt = _t(*cases.fps_ties())
    got = amd.furthest_point_sample_stacked(xyz, cnt, 40)
    assert np.array_equal(got.numpy(), vsa_ref.fps_stacked(xyz.numpy(), cnt.numpy(), 40))
    # the batched form is the stacked form with equal counts, int32
    lat = xyz[:729].reshape(1, 729, 3).repeat(2, 1, 1).contiguous()
    b = amd.furthest_point_sample(lat, 40)
    assert b.dtype == torch.int32 and torch.equal(b[0].long(), got[0]) and torch.equal(b[1], b[0])


@pytest.mark.parametrize('npoint', cases.FPS_DEEP_NPOINT)
def test_fps_twin_matches_oracle_beyond_the_register_capacity(npoint):
    """the sizes at which the kernel's threads visit one and two points beyond their registers; npoint 19000 wraps around in four
    samples and not in the fifth"""
    xyz, cnt = _t(*cases.fps_deep())
    got = amd.furthest_point_sample_stacked(xyz, cnt, npoint)
    assert got.dtype == torch.int64 and np.array_equal(got.numpy(), cases.fps_deep_reference(npoint))


def test_fps_twin_ties_and_batched_form_on_large_samples():
    xyz, cnt = _t(*cases.fps_deep_ties())
    got = amd.furthest_point_sample_stacked(xyz, cnt, 800)
    want = cases.fps_deep_ties_reference(800)
    assert len(np.unique(want)) == 729 and want.max() < 729      # every later copy of the lattice ties with the first and loses
    assert np.array_equal(got.numpy(), want)
    x, want = cases.fps_batched()
    x = torch.from_numpy(np.array(x))
    b = amd.furthest_point_sample(x, cases.FPS_BATCHED_NPOINT)
    assert b.dtype == torch.int32 and np.array_equal(b.numpy(), want)
    s = amd.furthest_point_sample_stacked(x.reshape(-1, 3), torch.full((x.shape[0],), x.shape[1], dtype=torch.int32), cases.FPS_BATCHED_NPOINT)
    assert torch.equal(b.long(), s)


def test_argument_errors():
    xyz, pc, new_xyz, qc, feats = _t(*cases.stack('63_tile-1_noqueries'))
    with pytest.raises(RuntimeError, match='Cannot have not features and not use xyz'):
        amd.QueryAndGroup(0.5, 8, use_xyz=False)(xyz, pc, new_xyz, qc, None)
    with pytest.raises(RuntimeError, match='shape mismatch'):
        amd.QueryAndGroup(0.5, 8)(xyz[:, :2], pc, new_xyz, qc)
    with pytest.raises(RuntimeError, match='shape mismatch'):
        amd.QueryAndGroup(0.5, 8)(xyz, pc, new_xyz, qc, feats[:-1])            # one feature row per point
    with pytest.raises(RuntimeError, match='shape mismatch'):
        amd.QueryAndGroup(0.5, 8)(xyz, pc, new_xyz, qc[:-1])                   # sample counts disagree
    with pytest.raises(RuntimeError, match='shape mismatch'):
        amd.grouping(feats, pc, torch.zeros(13, dtype=torch.int32), qc)
    with pytest.raises(RuntimeError, match='nsample'):
        amd.ball_query(0.5, 0, xyz, pc, new_xyz, qc)
    with pytest.raises(RuntimeError, match='nsample'):
        amd.QueryAndGroup(0.5, 4096)
    with pytest.raises(RuntimeError, match='integer'):
        amd.ball_query(0.5, 4, xyz, pc.float(), new_xyz, qc)
    with pytest.raises(RuntimeError, match='shape mismatch'):
        amd.furthest_point_sample(xyz, 4)
    with pytest.raises(TypeError):
        amd.QueryAndGroup(0.5, 8, True, True)                                   # the reference's `debug` is not taken
