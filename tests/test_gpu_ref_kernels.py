"""The REFERENCE's own device kernels against everything that claims to restate them.

oracle/_ref/ref_vsa.so (ball_query.cu, group_points.cu, sampling.cu, voxel_query_gpu.cu) and oracle/_ref/ref_vox.so
(scatter_points_cuda.cu) are the reference sources compiled for this GPU from where they lie (oracle/Makefile); oracle/ref_kernels.py
validates every argument on the host and launches them.  Each case (tests/ref_kernel_cases.py, asserted on the CPU at import to hold
what it names) compares the reference kernel's output with
  * the numpy restatement the other suites trust (tests/vsa_ref.py, tests/voxel_query_ref.py, oracle/voxel_oracle.py),
  * the product on the device, and
  * the product's `_cpu` twin (the scatter has none).
Decisions — indices, masks, picks, copies, maxima — compare EXACTLY; atomic fp32 sums compare exactly where the sum is exact
(small integers) and inside `k * 2^-24 * sum|terms|` of the fp64 sum otherwise.  Where the product deviates on purpose
(INTEGRATION.md §"Voxel-set-abstraction ops", "Voxel query") the deviation is a named case on the inputs it covers, nothing wider.

A test here skips only with the reason 'oracle/_ref/<file> absent or not loadable'.
"""
import numpy as np
import pytest
import torch

import mmdet3d_gaussian_amd as amd
from oracle import ref_kernels as rk
from oracle import voxel_oracle as vo

import ref_kernel_cases as cases
import vsa_ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                                                       # unit roundoff of fp32
CPU = torch.device('cpu')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda', torch.cuda.current_device())


@pytest.fixture(scope='module')
def vsa():
    if rk.load_vsa() is None:
        pytest.skip('oracle/_ref/ref_vsa.so absent or not loadable')


@pytest.fixture(scope='module')
def vox():
    if rk.load_vox() is None:
        pytest.skip('oracle/_ref/ref_vox.so absent or not loadable')


def t(a, d, dtype=None):
    x = torch.from_numpy(np.array(a))
    return (x if dtype is None else x.to(dtype)).to(d).contiguous()


def n(x):
    return x.detach().cpu().numpy()


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f'{what}: shape {got.shape} != {want.shape}'
    assert np.array_equal(got, want), f'{what}: {(got != want).sum()} of {got.size} differ'


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, f'{what}: shape {got.shape} != {want.shape}'
    assert got.tobytes() == want.tobytes(), f'{what}: {(got.view(np.int32) != want.view(np.int32)).sum()} of {got.size} differ in bits'


def fixup(raw, what):
    """What the kernels leave of an empty query, then the reference's Python fix-up (group_points.py:30-32): -> (idx, mask) numpy.
    The kernel writes ONLY slot 0 of an empty row (-1); the other slots keep the caller's zeros."""
    raw = n(raw)
    empty = raw[:, 0] == -1
    assert (raw[empty, 1:] == 0).all(), f'{what}: an empty row was written past slot 0'
    assert (raw[~empty] >= 0).all(), f'{what}: -1 outside slot 0'
    idx, mask = rk.ball_query_fixup(torch.from_numpy(raw))
    return idx.numpy(), mask.numpy()


# ------------------------------------------------------------------------------------------------ ball query

def _ball_query_everywhere(radius, nsample, xyz, pc, new_xyz, qc, dev, want):
    w_idx, w_cnt, w_mask = want
    raw = rk.ball_query(radius, nsample, t(xyz, dev), t(pc, dev), t(new_xyz, dev), t(qc, dev))
    r_idx, r_mask = fixup(raw, 'reference ball_query')
    same(r_idx, w_idx, 'reference idx vs restatement')
    same(r_mask, w_mask, 'reference mask vs restatement')
    for d in (dev, CPU):
        idx, mask, cnt = amd.ball_query(radius, nsample, t(xyz, d), t(pc, d), t(new_xyz, d), t(qc, d), return_cnt=True)
        same(n(idx), r_idx, f'product idx on {d.type} vs reference')
        same(n(mask), r_mask, f'product mask on {d.type} vs reference')
        same(n(cnt), w_cnt, f'product cnt on {d.type} vs restatement')
    return r_idx, r_mask


@pytest.mark.parametrize('nsample', cases.BQ_NSAMPLE)
def test_ball_query(nsample, vsa, dev):
    """points (700, 0, 65), queries (130, 7, 33); at this radius query 0 has exactly nsample members, others more, others none"""
    xyz, new_xyz = cases.bq_cloud()
    _ball_query_everywhere(cases.bq_radius(nsample), nsample, xyz, cases.BQ_POINTS, new_xyz, cases.BQ_QUERIES, dev,
                           cases.bq_reference(nsample))


def test_ball_query_excludes_the_sphere(vsa, dev):
    """integer lattice, radius 3: the points at d2 == 9 exactly are NOT members (d2 < radius2), in the reference as in ours"""
    xyz, pc, new_xyz, qc = cases.bq_lattice()
    want = vsa_ref.ball_query(cases.LATTICE_RADIUS, cases.LATTICE_NSAMPLE, xyz, pc, new_xyz, qc)
    r_idx, r_mask = _ball_query_everywhere(cases.LATTICE_RADIUS, cases.LATTICE_NSAMPLE, xyz, pc, new_xyz, qc, dev, want)
    assert not r_mask.any()
    for q, row in zip(new_xyz, r_idx):
        assert (vsa_ref.dist2(q, xyz[row]) < 9.0).all()
    same(np.sort(r_idx[0, :64]), np.sort(np.flatnonzero(vsa_ref.dist2(new_xyz[0], xyz) < 9.0)[:64]), 'interior query: first 64 of 93 inside')


# ------------------------------------------------------------------------------------------------ grouping

def _group_operands(nsample, dev):
    """idx as the reference's `BallQuery.forward` returns it (restatement, pinned to the kernel by test_ball_query), and the rows /
    counts the reference's grouping may be given: the queries of the sample WITHOUT points name a row that does not exist."""
    idx = cases.bq_reference(nsample)[0]
    has = cases.group_rows()
    return idx, has, t(idx[has], dev), t(cases.group_counts_for_reference(), dev)


@pytest.mark.parametrize('c', cases.GROUP_C)
def test_grouping_forward(c, vsa, dev):
    """out[m, c, s] = features[start_b + idx[m, s], c], bit for bit.  NAMED DEVIATION, on the 7 queries of the point-less sample only:
    the reference would read row 0 of the NEXT sample (or past the array); ours gives zeros."""
    feats = cases.group_features(c)
    for nsample in cases.BQ_NSAMPLE:
        idx, has, idx_ref, cnt_ref = _group_operands(nsample, dev)
        ref = n(rk.group_points(t(feats, dev), t(cases.BQ_POINTS, dev), idx_ref, cnt_ref))
        want = vsa_ref.grouping(feats, cases.BQ_POINTS, idx, cases.BQ_QUERIES)
        same_bits(ref, want[has], f'reference vs restatement, nsample {nsample}')
        for d in (dev, CPU):
            out = n(amd.grouping(t(feats, d), t(cases.BQ_POINTS, d), t(idx, d), t(cases.BQ_QUERIES, d)))
            same_bits(out[has], ref, f'product on {d.type} vs reference, nsample {nsample}')
            assert (~has).sum() == 7 and (out[~has] == 0).all()


def _grouping_backward(nsample, c, integer, dev):
    """-> (reference grad, product grad on the device, product grad on the CPU, restatement (fp64 grad, k, sum|terms|))"""
    idx, has, idx_ref, cnt_ref = _group_operands(nsample, dev)
    gout = cases.group_grad_out(nsample, c, integer)
    rows = int(cases.BQ_POINTS.sum())
    ref = n(rk.group_points_grad(t(gout[has], dev), idx_ref, cnt_ref, t(cases.BQ_POINTS, dev), rows))
    ours = []
    for d in (dev, CPU):
        f = t(cases.group_features(c), d).requires_grad_(True)
        out = amd.grouping(f, t(cases.BQ_POINTS, d), t(idx, d), t(cases.BQ_QUERIES, d))
        ours.append(n(torch.autograd.grad(out, f, t(gout, d))[0]))
    return ref, ours[0], ours[1], vsa_ref.grouping_backward(gout, idx, cases.BQ_QUERIES, cases.BQ_POINTS, rows)


@pytest.mark.parametrize('c', cases.GROUP_C)
def test_grouping_backward_on_integer_gradients(c, vsa, dev):
    """|g| <= 4 and at most a few thousand terms per element: every partial sum is an integer below 2^24, exact in any order"""
    ref, ours, twin, (want, num, _) = _grouping_backward(33, c, True, dev)
    assert num.max() >= 40 and (num == 0).any()
    same_bits(ref, want, 'reference vs restatement')
    same_bits(ours, ref, 'product on the device vs reference')
    same_bits(twin, ref, 'product twin vs reference')


def test_grouping_backward_on_random_gradients(vsa, dev):
    """an fp32 sum of k terms in any order lies within k * 2^-24 * sum|terms| of the exact sum"""
    ref, ours, twin, (want, num, mag) = _grouping_backward(32, 16, False, dev)
    bound = num[:, None] * U * mag
    assert num.max() >= 40
    for got, what in ((ref, 'reference'), (ours, 'product on the device'), (twin, 'product twin')):
        err = np.abs(got.astype(np.float64) - want)
        print(f'{what}: worst error / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}')
        assert (err <= bound).all(), what


@pytest.mark.parametrize('use_xyz', [True, False])
@pytest.mark.parametrize('nsample', [16, 33])
def test_query_and_group(nsample, use_xyz, vsa, dev):
    """ours (one launch) against `QueryAndGroup.forward` (group_points.py:131-183) made of the two reference kernels: ball query and
    fix-up, grouping of xyz, ONE fp32 subtraction of the centre, zeroing of the empty balls, grouping of the features, zeroing, cat.
    The queries of the point-less sample are empty balls: zero in the reference too, whatever it grouped for them."""
    xyz, new_xyz = cases.bq_cloud()
    pc, qc, c = cases.BQ_POINTS, cases.BQ_QUERIES, 5
    feats = cases.group_features(c)
    radius = cases.bq_radius(nsample)
    idx, mask = fixup(rk.ball_query(radius, nsample, t(xyz, dev), t(pc, dev), t(new_xyz, dev), t(qc, dev)), 'reference ball_query')
    has = cases.group_rows()
    assert mask[~has].all()
    idx_ref, cnt_ref = t(idx[has], dev), t(cases.group_counts_for_reference(), dev)
    m = len(new_xyz)
    grouped_xyz = np.zeros((m, 3, nsample), np.float32)
    grouped_xyz[has] = n(rk.group_points(t(xyz, dev), t(pc, dev), idx_ref, cnt_ref))
    grouped_xyz -= new_xyz[:, :, None]
    grouped_xyz[mask] = 0
    grouped = np.zeros((m, c, nsample), np.float32)
    grouped[has] = n(rk.group_points(t(feats, dev), t(pc, dev), idx_ref, cnt_ref))
    grouped[mask] = 0
    want = np.concatenate([grouped_xyz, grouped], 1) if use_xyz else grouped
    assert (want[~mask] != 0).any() and mask.any()
    for d in (dev, CPU):
        out, o_idx = amd.QueryAndGroup(radius, nsample, use_xyz=use_xyz)(t(xyz, d), t(pc, d), t(new_xyz, d), t(qc, d), t(feats, d))
        same(n(o_idx), idx, f'idx on {d.type}')
        same_bits(n(out), want, f'new_features on {d.type}')


# ------------------------------------------------------------------------------------------------ furthest point sampling

@pytest.mark.parametrize('size', cases.FPS_SMALL + cases.FPS_LARGE)
def test_fps_on_tie_free_clouds(size, vsa, dev):
    """dense (2, n, 3), npoint <= n; the restatement saw ONE arg max at every pick (asserted at import), so the reference's
    block-size-dependent tie-break has nothing to decide: picks equal exactly.  The reference's block is 2^floor(log2 n) <= 1024."""
    xyz = cases.fps_cloud(size)
    want, _ = cases.fps_reference(size)
    assert rk.fps_block(size) == min(1 << (size.bit_length() - 1), 1024)
    for npoint in cases.fps_npoints(size):
        ref = n(rk.furthest_point_sampling(t(xyz, dev), npoint))
        same(ref, want[:, :npoint], f'reference vs restatement, npoint {npoint}')
        for d in (dev, CPU):
            got = amd.furthest_point_sample(t(xyz, d), npoint)
            assert got.dtype == torch.int32
            same(n(got), ref, f'product on {d.type} vs reference, npoint {npoint}')


def test_fps_on_exact_ties_names_the_deviation(vsa, dev):
    """NAMED DEVIATION (include/gd3d.h gd3d_vsa_fps): on exactly equal running minima ours takes the LOWEST index, the
    reference whichever its shared-memory tree keeps (the lower thread slot, so it depends on the block size).  Up to the first pick
    where they part the picks are equal; at that pick both are arg maxima of the same running minima and ours is the lowest."""
    xyz = cases.fps_tied()
    want, t_at = cases.fps_tied_reference()
    npoint = cases.FPS_TIED_NPOINT
    ref = n(rk.furthest_point_sampling(t(xyz, dev), npoint))[0]
    for d in (dev, CPU):
        same(n(amd.furthest_point_sample(t(xyz, d), npoint))[0], want, f'product on {d.type} vs restatement')
    differ = np.flatnonzero(ref != want)
    print(f'block {rk.fps_block(xyz.shape[1])}: reference and product part at pick {differ[0] if len(differ) else None} of {npoint}')
    if len(differ):
        p = int(differ[0])
        assert p >= 1
        top = t_at[p].max()
        assert t_at[p][ref[p]] == top and t_at[p][want[p]] == top, 'at the parting pick one of the two is no arg max'
        assert want[p] == np.flatnonzero(t_at[p] == top)[0] and ref[p] > want[p]


# ------------------------------------------------------------------------------------------------ voxel query

def _voxel_query_everywhere(scene, max_range, radius, nsample, want, dev):
    """the reference on the product's OWN dense table and query cells (both equal to the restatement's, and validated by the driver)"""
    B, shape = cases.VQ_B, cases.VQ_SHAPE
    coors, xyz, new_xyz = t(scene['coors'], dev, torch.int32), t(scene['xyz'], dev), t(scene['new_xyz'], dev)
    table = amd.voxel_point_indices(coors, shape, B)
    nc = amd.voxel_query_coords(new_xyz, t(scene['counts'], dev), cases.VQ_VOXEL_SIZE, cases.VQ_PC_RANGE, 1)
    same(n(table), scene['table'], 'dense table')
    same(n(nc), scene['new_coords'], 'query cells')
    raw = rk.voxel_query(max_range, radius, nsample, xyz, new_xyz, nc, table)
    r_idx, r_mask = fixup(raw, 'reference voxel query')
    same(r_idx, want['idx'], 'reference idx vs restatement')
    same(r_mask, want['mask'], 'reference mask vs restatement')
    for d in (dev, CPU):
        c = t(scene['coors'], d, torch.int32)
        for form, index in (('table', amd.voxel_point_indices(c, shape, B)), ('sorted keys', amd.voxel_query_index(c, shape, B))):
            idx, mask, cnt = amd.voxel_query(max_range, radius, nsample, t(scene['xyz'], d), t(scene['new_xyz'], d),
                                             t(scene['new_coords'], d), index, return_cnt=True)
            same(n(idx), r_idx, f'product idx ({form}, {d.type}) vs reference')
            same(n(mask), r_mask, f'product mask ({form}, {d.type}) vs reference')
            same(n(cnt), want['cnt'], f'product cnt ({form}, {d.type}) vs restatement')
    return r_idx, r_mask


@pytest.mark.parametrize('nsample', cases.VQ_NSAMPLE)
@pytest.mark.parametrize('max_range', cases.VQ_RANGES, ids=lambda r: 'r%d%d%d' % r)
def test_voxel_query(max_range, nsample, vsa, dev):
    """B = 2 on (5, 12, 10), 395 voxels, 301 queries with every corner and face of the grid"""
    _voxel_query_everywhere(cases.vq_scene(), max_range, cases.vq_radius(max_range, nsample), nsample,
                            cases.vq_reference(max_range, nsample), dev)


def test_voxel_query_includes_the_sphere(vsa, dev):
    """integer lattice, radius 3: rows at d2 == 9 exactly ARE members (the reference rejects with dist2 > radius2)"""
    scene = cases.vq_lattice()
    r_idx, r_mask = _voxel_query_everywhere(scene, cases.VQ_LATTICE_RANGE, cases.LATTICE_RADIUS, cases.VQ_LATTICE_NSAMPLE,
                                            cases.vq_lattice_reference(), dev)
    assert not r_mask.any()
    assert (vsa_ref.dist2(scene['new_xyz'][0], scene['xyz'][r_idx[0]]) == 9.0).any()


# ------------------------------------------------------------------------------------------------ dynamic scatter

@pytest.mark.parametrize('name', sorted(cases.SC_CLOUDS))
def test_scatter_index(name, vox, dev):
    """voxel_coors (order included: at::unique_dim's), point2voxel_map, voxel_points_count: reference == numpy oracle == product"""
    from mmdet3d_gaussian_amd.scatter import scatter_index
    coors = t(cases.sc_coors(name), dev)
    want = cases.sc_index(name)
    ref = rk.scatter_index(coors)
    got = scatter_index(coors)
    assert ref[1].dtype == torch.int32 and ref[2].dtype == torch.int32 and got[1].dtype == torch.int32 and got[2].dtype == torch.int32
    for r, g, w, what in zip(ref, got, want, ('voxel_coors', 'point2voxel_map', 'voxel_points_count')):
        same(n(r), w, f'reference {what} vs oracle')
        same(n(g), n(r), f'product {what} vs reference')


def _scatter_operands(name, c, integer, dev):
    _, pmap, cnt = cases.sc_index(name)
    feats = cases.sc_feats(name, c, integer)
    return feats, pmap, cnt, t(feats, dev), t(pmap, dev), t(cnt, dev)


@pytest.mark.parametrize('red', cases.SC_REDUCE)
@pytest.mark.parametrize('c', cases.SC_C)
@pytest.mark.parametrize('name', sorted(cases.SC_CLOUDS))
def test_scatter_reduce_on_integer_features(name, c, red, vox, dev):
    """|v| <= 8: every sum is exact, so sum, max AND mean are bit-equal — mean = sum / count in fp32, no reciprocal form"""
    from mmdet3d_gaussian_amd.scatter import scatter_reduce
    feats, pmap, cnt, f, pm, ct = _scatter_operands(name, c, True, dev)
    ref = n(rk.scatter_reduce(f, pm, ct, red))
    want, _ = vo.scatter_reduce(feats, pmap, cnt, red, dtype=np.float32)
    same_bits(ref, want, 'reference vs oracle')
    same_bits(n(scatter_reduce(f, pm, ct, red)), ref, 'product vs reference')


@pytest.mark.parametrize('red', cases.SC_REDUCE)
@pytest.mark.parametrize('c', cases.SC_C)
def test_scatter_reduce_on_random_features(c, red, vox, dev):
    """max is a selection: bit-equal.  sum: k terms in any order, within k * 2^-24 * sum|terms| of the fp64 sum; mean adds the one
    rounding of the division: (k + 1) * 2^-24 * sum|terms| / k."""
    from mmdet3d_gaussian_amd.scatter import scatter_reduce
    feats, pmap, cnt, f, pm, ct = _scatter_operands('n3000', c, False, dev)
    ref, got = n(rk.scatter_reduce(f, pm, ct, red)), n(scatter_reduce(f, pm, ct, red))
    want, _ = vo.scatter_reduce(feats, pmap, cnt, red)
    if red == 'max':
        same_bits(ref, want.astype(np.float32), 'reference vs oracle')
        same_bits(got, ref, 'product vs reference')
        return
    mag, _ = vo.scatter_reduce(np.abs(feats), pmap, cnt, 'sum')
    k = cnt[:, None].astype(np.float64)
    bound = k * U * mag if red == 'sum' else (k + 1) * U * mag / k
    for out, what in ((ref, 'reference'), (got, 'product')):
        err = np.abs(out.astype(np.float64) - want)
        print(f'{what} {red}: worst error / bound = {np.max(err / bound):.3f}')
        assert (err <= bound).all(), what


@pytest.mark.parametrize('red', cases.SC_REDUCE)
@pytest.mark.parametrize('c', cases.SC_C)
@pytest.mark.parametrize('name', sorted(cases.SC_CLOUDS))
def test_scatter_backward(name, c, red, vox, dev):
    """integer gradients: sum copies, mean divides once (grad / count in fp32), max sends the gradient to the LOWEST point index among
    the equal maxima the case plants (the reference's atomicMin) — all bit-equal"""
    from mmdet3d_gaussian_amd.scatter import scatter_reduce
    feats, pmap, cnt, f, pm, ct = _scatter_operands(name, c, True, dev)
    gvox = cases.sc_grad(name, c)
    reduced = rk.scatter_reduce(f, pm, ct, red)
    ref = n(rk.scatter_backward(t(gvox, dev), f, reduced, pm, ct, red))
    want = vo.scatter_backward(gvox, feats, pmap, cnt, red, dtype=np.float32)
    same_bits(ref, want, 'reference vs oracle')
    fg = f.clone().requires_grad_(True)
    got, = torch.autograd.grad(scatter_reduce(fg, pm, ct, red), fg, t(gvox, dev))
    same_bits(n(got), ref, 'product vs reference')
    assert (ref[pmap < 0] == 0).all()
