"""The voxel-set-abstraction kernels of csrc/vsa.hip on the MI355X: device against the `_cpu` twin and against the numpy oracle
(tests/vsa_ref.py), both with EXACT equality on idx, cnt, the empty-ball mask, the grouped output and the FPS picks, on the
smallest shapes at which each kernel can still go wrong (tests/vsa_cases.py); the atomic backward bit for bit on integer
gradients and inside the derived rounding bound on normal ones; graph capture."""
import numpy as np
import pytest
import torch

import mmdet3d_gaussian_amd as amd
import vsa_cases as cases
import vsa_ref

pytestmark = pytest.mark.gpu


def _t(*arrays):
    return [torch.from_numpy(np.array(a)) for a in arrays]


def _dev(*tensors):
    return [t.cuda() for t in tensors]


def _check_forward(kind, name, radius, nsample, c, use_xyz):
    """device == oracle == twin for the fused launch, the stand-alone query and the stand-alone grouping"""
    host = _t(*cases.inputs(kind, name))
    xyz, pc, new_xyz, qc, feats = _dev(*host)
    f = None if c == 0 else feats[:, :c].contiguous()
    out, idx = amd.QueryAndGroup(radius, nsample, use_xyz=use_xyz)(xyz, pc, new_xyz, qc, f)
    bidx, mask, cnt = amd.ball_query(radius, nsample, xyz, pc, new_xyz, qc, return_cnt=True)
    r_out, r_idx, r_cnt, r_mask = cases.reference(kind, name, radius, nsample, c, use_xyz)
    assert idx.dtype == torch.int32 and mask.dtype == torch.bool and cnt.dtype == torch.int32
    assert np.array_equal(idx.cpu().numpy(), r_idx) and np.array_equal(bidx.cpu().numpy(), r_idx)
    assert np.array_equal(cnt.cpu().numpy(), r_cnt) and np.array_equal(mask.cpu().numpy(), r_mask)
    assert out.shape == r_out.shape and np.array_equal(out.cpu().numpy(), r_out)
    hf = None if c == 0 else host[4][:, :c].contiguous()
    t_out, t_idx = amd.QueryAndGroup(radius, nsample, use_xyz=use_xyz)(host[0], host[1], host[2], host[3], hf)
    assert torch.equal(out.cpu(), t_out) and torch.equal(idx.cpu(), t_idx)
    if c:
        g = amd.grouping(f, pc, idx, qc)
        assert torch.equal(g.cpu(), amd.grouping(hf, host[1], t_idx, host[3]))
    return r_cnt


@pytest.mark.parametrize('nsample', [1, 5, 16, 32])
@pytest.mark.parametrize('name', sorted(cases.STACKS))
def test_device_matches_oracle_and_twin_on_stacked_batches(name, nsample):
    """B = 3 with unequal counts, a sample without points and one without queries, M no multiple of the 8 queries of a workgroup,
    samples of 1, 63, 64, 65 points and one tile - 1, exact, + 1; dense balls (early stop), sparse balls (padded tails), empty ones"""
    dense = _check_forward('stack', name, 0.9, nsample, 3, True)
    sparse = _check_forward('stack', name, 0.25, nsample, 3, True)
    assert (dense == 0).any() and (name.startswith('small') or (dense == nsample).any())
    if nsample >= 5:
        assert ((sparse > 0) & (sparse < nsample)).any()


@pytest.mark.parametrize('c,use_xyz', [(0, True)] + [(c, u) for c in (1, 3, 16, 17, 64, 67) for u in (True, False)])
def test_device_matches_oracle_over_channel_counts(c, use_xyz):
    """rows shorter than a wave, a whole wave, longer; more channels than one pass through the transpose buffer holds (67 x 17 floats)"""
    _check_forward('stack', 'tile+1_nopoints_64', 0.6, 16, c, use_xyz)
    if c in (0, 67):
        _check_forward('stack', '1_tile_2tiles+', 0.9, 32, c, use_xyz)


@pytest.mark.parametrize('nsample', [1, 5, 16, 32])
@pytest.mark.parametrize('members', [4, 5, 6, 16, 32, 33, 40])
def test_exactly_nsample_members_and_boundary_straddlers(members, nsample):
    """fewer members than nsample, exactly nsample, more — lying either side of the 64-point step (63 | 64) and of the tile
    boundary (1023 | 1024): the early stop must not change idx, cnt or the tail"""
    cnt = _check_forward('crafted', '', cases.crafted_radius(members), nsample, 16, True)
    assert cnt[0] == min(members, nsample) and cnt[-1] == 0


@pytest.mark.parametrize('nsample', cases.WIDE_NSAMPLE)
def test_device_matches_oracle_and_twin_above_one_wave_of_slots(nsample):
    """nsample 33 to 1024 (vsa_cases.WIDE_NSAMPLE: either side of one wave of slots, of one channel per pass and of the 64 KiB of
    dynamic LDS of the fused and of the stand-alone grouping launch) on 2300, 700 and 0 points: balls that fill two tiles after
    their first member, padded tails of 1 to 990 slots, empty balls"""
    for radius in (cases.R_ALL, cases.R_MID):
        want = cases.wide_conditions(radius, nsample)
        assert np.array_equal(_check_forward('wide', '', radius, nsample, 3, True), want)


@pytest.mark.parametrize('c,use_xyz', [(0, True)] + [(c, u) for c in (1, 17, 67) for u in (True, False)])
@pytest.mark.parametrize('nsample', [64, 128, 1024])
def test_device_matches_oracle_over_channel_counts_at_large_nsample(nsample, c, use_xyz):
    """16, 8 and ONE channel per pass through the transpose buffer: 17 and 67 channels end in a shorter pass (67 at 8 per pass:
    three channels, 21 rows per wave instruction and an idle lane), at 1024 every channel is a pass of its own"""
    for radius in (cases.R_ALL, cases.R_MID):
        cases.wide_conditions(radius, nsample)
        _check_forward('wide', '', radius, nsample, c, use_xyz)


def test_point_at_exactly_the_radius_is_excluded():
    xyz, pc, new_xyz, qc = _dev(*_t(*cases.exact_radius()))
    idx, mask, cnt = amd.ball_query(5.0, 8, xyz, pc, new_xyz, qc, return_cnt=True)
    assert idx[0].tolist() == [1, 2, 1, 1, 1, 1, 1, 1] and cnt.tolist() == [2, 0] and mask.tolist() == [False, True]


def _backward_inputs(c, nsample, radius, integer, seed):
    xyz, pc, new_xyz, qc = _t(*cases.duplication())
    rng = np.random.RandomState(seed)
    feats = torch.from_numpy(rng.uniform(-1, 1, (xyz.shape[0], c)).astype(np.float32))
    r_idx, r_cnt, r_mask = vsa_ref.ball_query(radius, nsample, xyz.numpy(), pc.numpy(), new_xyz.numpy(), qc.numpy())
    shape = (new_xyz.shape[0], 3 + c, nsample)
    gout = rng.randint(-8, 9, shape).astype(np.float32) if integer else rng.standard_normal(shape).astype(np.float32)
    return (xyz, pc, new_xyz, qc, feats), (r_idx, r_cnt, r_mask), gout


@pytest.mark.parametrize('c', [1, 16, 17, 67])
def test_backward_is_exact_on_integer_gradients(c):
    """grad_out drawn from the integers in [-8, 8]: every sum is exact in fp32 in ANY order, so the atomic backward must equal
    the oracle bit for bit — 40 queries at one centre (heavy duplication), padded tails (folded before one add), empty balls"""
    nsample = 16
    host, (r_idx, r_cnt, r_mask), gout = _backward_inputs(c, nsample, 0.9, True, c)
    assert r_mask.sum() == 3 and ((r_cnt > 0) & (r_cnt < nsample)).any() and (r_cnt == nsample).any()
    xyz, pc, new_xyz, qc, feats = _dev(*host)
    n = xyz.shape[0]
    feats.requires_grad_()
    out, idx = amd.QueryAndGroup(0.9, nsample)(xyz, pc, new_xyz, qc, feats)
    assert np.array_equal(idx.cpu().numpy(), r_idx)
    grad, = torch.autograd.grad(out, feats, torch.from_numpy(gout).cuda())
    want, _, _ = vsa_ref.grouping_backward(gout[:, 3:], r_idx, qc.cpu().numpy(), pc.cpu().numpy(), n, ~r_mask)
    assert np.array_equal(grad.cpu().numpy().astype(np.float64), want)
    # the stand-alone grouping backward: every slot a contribution of its own, the empty balls' zero indices included
    f2 = feats.detach().clone().requires_grad_()
    g2, = torch.autograd.grad(amd.grouping(f2, pc, idx, qc), f2, torch.from_numpy(gout[:, 3:].copy()).cuda())
    want2, _, _ = vsa_ref.grouping_backward(gout[:, 3:], r_idx, qc.cpu().numpy(), pc.cpu().numpy(), n)
    assert np.array_equal(g2.cpu().numpy().astype(np.float64), want2)
    # and the twin
    hf = host[4].clone().requires_grad_()
    h_out, _ = amd.QueryAndGroup(0.9, nsample)(host[0], host[1], host[2], host[3], hf)
    h_grad, = torch.autograd.grad(h_out, hf, torch.from_numpy(gout))
    assert torch.equal(grad.cpu(), h_grad)


def test_backward_with_normal_gradients_stays_inside_the_rounding_bound():
    """An fp32 sum of k terms taken in any order differs from the exact sum by at most k * 2^-24 * sum|terms| (k - 1 additions, each
    rounding a partial sum no larger than sum|terms|; second-order terms are covered by the k-th unit).  Per element, k and
    sum|terms| come from the oracle; nothing here is measured."""
    c, nsample = 32, 16
    host, (r_idx, r_cnt, r_mask), gout = _backward_inputs(c, nsample, 0.9, False, 99)
    xyz, pc, new_xyz, qc, feats = _dev(*host)
    feats.requires_grad_()
    out, _ = amd.QueryAndGroup(0.9, nsample)(xyz, pc, new_xyz, qc, feats)
    grad, = torch.autograd.grad(out, feats, torch.from_numpy(gout).cuda())
    want, num, mag = vsa_ref.grouping_backward(gout[:, 3:], r_idx, qc.cpu().numpy(), pc.cpu().numpy(), xyz.shape[0], ~r_mask)
    assert num.max() >= 40
    err = np.abs(grad.cpu().numpy().astype(np.float64) - want)
    bound = num[:, None] * 2.0 ** -24 * mag
    print('max err / bound:', float((err / np.maximum(bound, 1e-300)).max()), 'max contributions', int(num.max()))
    assert (err <= bound).all()
    assert (grad.cpu().numpy()[num == 0] == 0).all()


def _wide_backward(c, nsample, radius, integer):
    """-> the fused backward's and the stand-alone grouping backward's gradient on `wide` (device), the twin's fused one, the
    oracle's idx and mask, the upstream gradient"""
    host = _t(*cases.wide())
    xyz, pc, new_xyz, qc, feats = _dev(*host)
    _, r_idx, _, r_mask = cases.reference('wide', '', radius, nsample, 0, True)
    rng = np.random.RandomState(1000 * c + nsample)
    shape = (new_xyz.shape[0], 3 + c, nsample)
    gout = rng.randint(-8, 9, shape).astype(np.float32) if integer else rng.standard_normal(shape).astype(np.float32)
    f = feats[:, :c].contiguous().requires_grad_()
    out, idx = amd.QueryAndGroup(radius, nsample)(xyz, pc, new_xyz, qc, f)
    assert np.array_equal(idx.cpu().numpy(), r_idx)
    grad, = torch.autograd.grad(out, f, torch.from_numpy(gout).cuda())
    f2 = f.detach().clone().requires_grad_()
    g2, = torch.autograd.grad(amd.grouping(f2, pc, idx, qc), f2, torch.from_numpy(gout[:, 3:].copy()).cuda())
    hf = host[4][:, :c].contiguous().requires_grad_()
    h_out, _ = amd.QueryAndGroup(radius, nsample)(host[0], host[1], host[2], host[3], hf)
    h_grad, = torch.autograd.grad(h_out, hf, torch.from_numpy(gout))
    return grad.cpu(), g2.cpu(), h_grad, r_idx, r_mask, gout


@pytest.mark.parametrize('c', [1, 17])
@pytest.mark.parametrize('nsample', [65, 128, 701, 1024])
def test_backward_is_exact_on_integer_gradients_at_large_nsample(nsample, c):
    """every point of the sample a member: full balls of up to 1024 slots in sample 0, in sample 1 (700 points) a folded tail of 1
    slot at nsample 701 and of 324 at 1024.  At most 12 * 1024 integers of magnitude <= 8 meet in one sum: exact in fp32 (< 2^24)
    in any order, so the atomic backward equals the oracle bit for bit."""
    want_cnt = cases.wide_conditions(cases.R_ALL, nsample)
    assert (want_cnt[7:10] == min(700, nsample)).all()
    grad, g2, h_grad, r_idx, r_mask, gout = _wide_backward(c, nsample, cases.R_ALL, True)
    _, pc, _, qc, _ = cases.wide()
    n = int(pc.sum())
    want, _, _ = vsa_ref.grouping_backward(gout[:, 3:], r_idx, qc, pc, n, ~r_mask)
    assert np.abs(want).max() > 8 and np.array_equal(grad.numpy().astype(np.float64), want)
    # the stand-alone grouping backward: every slot a contribution of its own, the zero indices of the empty balls included
    want2, _, _ = vsa_ref.grouping_backward(gout[:, 3:], r_idx, qc, pc, n)
    assert not np.array_equal(want2, want) and np.array_equal(g2.numpy().astype(np.float64), want2)
    assert torch.equal(grad, h_grad)


def test_backward_with_normal_gradients_stays_inside_the_rounding_bound_at_nsample_128():
    """the bound of test_backward_with_normal_gradients_stays_inside_the_rounding_bound (k * 2^-24 * sum|terms|, k and the sum from
    the oracle, nothing measured) where the slot loops take two passes: full balls, and tails of 3 to 94 slots folded in fp32"""
    for radius in (cases.R_MID, cases.R_ALL):
        cases.wide_conditions(radius, 128)
        grad, _, _, r_idx, r_mask, gout = _wide_backward(17, 128, radius, False)
        _, pc, _, qc, _ = cases.wide()
        want, num, mag = vsa_ref.grouping_backward(gout[:, 3:], r_idx, qc, pc, int(pc.sum()), ~r_mask)
        err = np.abs(grad.numpy().astype(np.float64) - want)
        bound = num[:, None] * 2.0 ** -24 * mag
        print('radius', radius, 'max err / bound:', float((err / np.maximum(bound, 1e-300)).max()), 'max contributions', int(num.max()))
        assert num.max() >= 6 and (err <= bound).all()
        assert (grad.numpy()[num == 0] == 0).all()


def test_nsample_above_the_limit_is_refused():
    """the wrappers refuse nsample 1025, and so does every C entry point that stages idx rows in LDS (GD3D_E_TOOLARGE, no launch)"""
    from mmdet3d_gaussian_amd import _lib
    xyz, pc, new_xyz, qc, feats = _dev(*_t(*cases.stack('small_1_64_65')))
    with pytest.raises(RuntimeError, match='nsample'):
        amd.QueryAndGroup(0.5, 1025)
    with pytest.raises(RuntimeError, match='nsample'):
        amd.ball_query(0.5, 1025, xyz, pc, new_xyz, qc)
    lib = _lib.load()
    n, m, c, ns, b = xyz.shape[0], new_xyz.shape[0], 2, 1025, 3
    f = feats[:, :c].contiguous()
    out = torch.zeros((m, 3 + c, ns), device='cuda')
    idx = torch.zeros((m, ns), dtype=torch.int32, device='cuda')
    cnt = torch.zeros((m,), dtype=torch.int32, device='cuda')
    mask = torch.zeros((m,), dtype=torch.bool, device='cuda')
    grad = torch.zeros((n, c), device='cuda')
    p = lambda t: t.data_ptr()
    too_large = 10002
    assert lib.gd3d_vsa_query_and_group(p(xyz), p(pc), p(new_xyz), p(qc), p(f), b, n, m, c, 0.5, ns, 1, p(out), p(idx), p(cnt), p(mask),
                                        None) == too_large
    assert lib.gd3d_vsa_ball_query(p(xyz), p(pc), p(new_xyz), p(qc), b, n, m, 0.5, ns, p(idx), p(cnt), p(mask), None) == too_large
    assert lib.gd3d_vsa_group(p(f), p(pc), p(idx), p(qc), b, n, m, c, ns, p(out), None) == too_large
    assert lib.gd3d_vsa_group_backward(p(out), p(idx), p(qc), p(pc), b, n, m, c, ns, p(grad), None) == too_large
    assert lib.gd3d_vsa_query_and_group_backward(p(out), p(idx), p(cnt), p(qc), p(pc), b, n, m, c, ns, 3, p(grad), None) == too_large
    torch.cuda.synchronize()
    assert not out.any() and not idx.any() and not grad.any()      # nothing ran


def test_fps_sizes_capacity_and_wraparound_in_one_launch():
    """samples of 1, 2, 63, 64, 65, 1024, 1025 points, the register capacity - 1, exact and + 1 (the last takes the workspace path)
    and an empty one, in ONE launch per npoint; npoint 1, 7 and 2048 lie below and above the sample sizes (wrap-around)"""
    xyz, cnt = _t(*cases.fps_cloud())
    dx, dc = _dev(xyz, cnt)
    for npoint in (1, 7, 2048):
        got = amd.furthest_point_sample_stacked(dx, dc, npoint)
        assert got.dtype == torch.int64 and got.shape == (len(cases.FPS_SIZES), npoint)
        assert np.array_equal(got.cpu().numpy(), cases.fps_reference(npoint))
    assert torch.equal(amd.furthest_point_sample_stacked(dx, dc, 7).cpu(), amd.furthest_point_sample_stacked(xyz, cnt, 7))


def test_fps_lowest_index_wins_exact_ties():
    """a lattice (many exactly equal distances), a cloud whose points are each present three times, and the lattice repeated
    beyond the register capacity: the lowest index wins on the device as in the oracle and the twin"""
    xyz, cnt = _t(*cases.fps_ties())
    got = amd.furthest_point_sample_stacked(xyz.cuda(), cnt.cuda(), 800).cpu()
    assert np.array_equal(got.numpy(), vsa_ref.fps_stacked(xyz.numpy(), cnt.numpy(), 800))
    assert torch.equal(got, amd.furthest_point_sample_stacked(xyz, cnt, 800))


def test_fps_batched_form_equals_stacked_form():
    rng = np.random.RandomState(8)
    x = torch.from_numpy(rng.uniform(-3, 3, (3, 200, 3)).astype(np.float32)).cuda()
    for npoint in (64, 333):     # below and above N
        b = amd.furthest_point_sample(x, npoint)
        s = amd.furthest_point_sample_stacked(x.reshape(-1, 3), torch.full((3,), 200, dtype=torch.int32, device='cuda'), npoint)
        assert b.dtype == torch.int32 and torch.equal(b.long(), s)
        assert np.array_equal(b[1].cpu().numpy(), vsa_ref.fps(x[1].cpu().numpy(), npoint))


@pytest.mark.parametrize('npoint', cases.FPS_DEEP_NPOINT)
def test_fps_beyond_one_extra_stride_with_workspace_samples_side_by_side(npoint):
    """17408 points (every thread visits ONE point beyond the registers), 17409 (thread 0 a second one), 20000 and 18500, with a
    register-only sample between them: four workspace segments in one launch; npoint 19000 wraps around in four samples and not
    in the fifth"""
    xyz, cnt = _t(*cases.fps_deep())
    got = amd.furthest_point_sample_stacked(xyz.cuda(), cnt.cuda(), npoint)
    assert got.dtype == torch.int64 and got.shape == (len(cases.FPS_DEEP_SIZES), npoint)
    assert np.array_equal(got.cpu().numpy(), cases.fps_deep_reference(npoint))
    assert torch.equal(got.cpu(), amd.furthest_point_sample_stacked(xyz, cnt, npoint))


def test_fps_lowest_index_wins_exact_ties_across_the_workspace_strides():
    """26 copies of the lattice: equal distances between the register part, the first and the second visit beyond it"""
    xyz, cnt = _t(*cases.fps_deep_ties())
    assert cnt.item() == 18954 > cases.FPS_CAP + 2048
    got = amd.furthest_point_sample_stacked(xyz.cuda(), cnt.cuda(), 800).cpu()
    want = cases.fps_deep_ties_reference(800)
    assert len(np.unique(want)) == 729 and want.max() < 729      # every later copy ties with the first and loses
    assert np.array_equal(got.numpy(), want)
    assert torch.equal(got, amd.furthest_point_sample_stacked(xyz, cnt, 800))


def test_fps_batched_form_beyond_the_registers():
    """the batched entry point (sample b starts at b * n) with two samples that both use the workspace"""
    x, want = cases.fps_batched()
    x = torch.from_numpy(np.array(x))
    b, n, _ = x.shape
    got = amd.furthest_point_sample(x.cuda(), cases.FPS_BATCHED_NPOINT)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(got.cpu(), amd.furthest_point_sample(x, cases.FPS_BATCHED_NPOINT))
    s = amd.furthest_point_sample_stacked(x.cuda().reshape(-1, 3), torch.full((b,), n, dtype=torch.int32, device='cuda'),
                                          cases.FPS_BATCHED_NPOINT)
    assert torch.equal(got.long(), s)


def test_ops_are_capturable_in_one_graph():
    """QueryAndGroup forward and backward plus the stacked FPS captured in one torch.cuda.graph and replayed on new input values:
    no wrapper synchronises with the host"""
    host, ref, gout = _backward_inputs(16, 16, 0.5, True, 4)
    xyz, pc, new_xyz, qc, feats = _dev(*host)
    feats.requires_grad_()
    gout = torch.from_numpy(gout).cuda()
    mod = amd.QueryAndGroup(0.5, 16)

    def step():
        out, idx = mod(xyz, pc, new_xyz, qc, feats)
        grad, = torch.autograd.grad(out, feats, gout)
        return out, idx, grad, amd.furthest_point_sample_stacked(xyz, pc, 50)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    with torch.no_grad():
        new_xyz.add_(0.3)                        # new values in the static buffers: other balls
        xyz[:40].mul_(1.1)
    graph.replay()
    torch.cuda.synchronize()
    eager = step()
    assert not torch.equal(eager[1], torch.from_numpy(ref[0]).cuda())      # the inputs did change the result
    for got, want in zip(captured, eager):
        assert torch.equal(got, want)


def test_query_and_group_at_the_nsample_limit_is_capturable():
    """QueryAndGroup(., 1024) asks for more than 64 KiB of dynamic LDS: the limit is raised by the first launch (the warm-up), so
    the captured launch is a launch and nothing else; replay on new input values equals eager"""
    radius, nsample = 2.5, 1024
    xyz, pc, new_xyz, qc, feats = _dev(*_t(*cases.wide()))
    _, r_idx, r_cnt, _ = cases.reference('wide', '', radius, nsample, 0, True)
    assert (r_cnt == nsample).any() and ((r_cnt > 0) & (r_cnt < nsample)).any() and (r_cnt == 0).any()
    f = feats[:, :17].contiguous().requires_grad_()
    gout = torch.from_numpy(np.random.RandomState(6).randint(-8, 9, (new_xyz.shape[0], 20, nsample)).astype(np.float32)).cuda()
    mod = amd.QueryAndGroup(radius, nsample)

    def step():
        out, idx = mod(xyz, pc, new_xyz, qc, f)
        grad, = torch.autograd.grad(out, f, gout)
        return out, idx, grad

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        warm = step()                            # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    assert np.array_equal(warm[1].cpu().numpy(), r_idx)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    with torch.no_grad():
        new_xyz.add_(0.3)                        # new values in the static buffers: other balls
    graph.replay()
    torch.cuda.synchronize()
    eager = step()
    assert not torch.equal(eager[1], warm[1])    # the inputs did change the result
    for got, want in zip(captured, eager):
        assert torch.equal(got, want)
