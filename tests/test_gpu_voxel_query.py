"""The voxel query kernels (csrc/voxel_query.hip) on the MI355X against the numpy restatement of tests/voxel_query_ref.py — the cases
of tests/voxel_query_cases.py that tests/test_cpu_voxel_query.py runs on the `_cpu` twins, with both look-up forms (the sorted index
and the dense table), every comparison an exact equality — and the graph capture of the whole chain."""
import numpy as np
import pytest
import torch

import mmdet3d_gaussian_amd as amd

import voxel_query_cases as cases

pytestmark = pytest.mark.gpu

CHANNELS = [(c, u) for c in (0, 1, 3, 16, 17, 64, 67) for u in (True, False) if c > 0 or u]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda', torch.cuda.current_device())


@pytest.mark.parametrize('coors_dtype', [torch.int32, torch.int64], ids=['i32', 'i64'])
@pytest.mark.parametrize('name', sorted(cases.CASES))
def test_query_matches_the_restatement(name, coors_dtype, dev):
    cases.check_query_case(amd, name, dev, coors_dtype)


@pytest.mark.parametrize('C,use_xyz', CHANNELS)
def test_grouped_block_matches_the_restatement(C, use_xyz, dev):
    cases.check_group_case(amd, 'w63', dev, C, use_xyz)


def test_grouped_block_at_nsample_1024(dev):
    cases.check_group_case(amd, 'ns1024', dev, 3, True)


def test_device_equals_the_cpu_twin(dev):
    """the fourth corner of the square: kernels and twins on the same tensors, both look-up forms"""
    scene, calls, _ = cases.case('rows65')
    rng_, radius, nsample = calls[0]
    t = cases.t
    feats = torch.randn(len(scene.xyz), 9)
    mod = amd.VoxelQueryAndGroup(rng_, radius, nsample)
    outs = []
    for d in (torch.device('cpu'), dev):
        coors = t(scene.coors, d, torch.int32)
        for index in (amd.voxel_query_index(coors, scene.shape, scene.B), amd.voxel_point_indices(coors, scene.shape, scene.B)):
            out, idx = mod(t(scene.xyz, d), t(scene.new_xyz, d), t(scene.new_coords, d), index, feats.to(d))
            outs.append((out.cpu().numpy(), idx.cpu().numpy()))
    for out, idx in outs[1:]:
        assert out.tobytes() == outs[0][0].tobytes() and idx.tobytes() == outs[0][1].tobytes()


def test_query_coords(dev):
    cases.check_coords(amd, dev)


def test_a_callers_table_with_garbage(dev):
    cases.check_garbage_table(amd, dev)


def test_member_sets_equal_ball_querys(dev):
    cases.check_against_ball_query(amd, dev)


def test_inclusive_where_ball_query_is_strict(dev):
    cases.check_inclusive_vs_ball_query(amd, dev)


def test_entries_write_every_element_and_nothing_else(dev):
    cases.check_entries_write_everything_and_nothing_else(amd, dev)


def test_backward(dev):
    cases.check_backward(amd, dev)


def test_empty_sizes(dev):
    cases.check_empty_sizes(amd, dev)


def test_argument_errors(dev):
    cases.check_argument_errors(amd, dev)


def test_graph_capture_of_the_whole_chain(dev):
    """voxel_query_index -> voxel_query_coords -> VoxelQueryAndGroup forward and backward, recorded once on one stream and replayed on
    fresh inputs of the same shapes: the replay equals the eager run."""
    scene, calls, _ = cases.case('w125')
    rng_, radius, nsample = calls[0]
    t = cases.t
    B, shape = scene.B, scene.shape
    N, M, C = len(scene.xyz), len(scene.new_xyz), 6
    gen = np.random.default_rng(99)
    counts = torch.tensor(scene.counts, dtype=torch.int32, device=dev)
    mod = amd.VoxelQueryAndGroup(rng_, radius, nsample)

    def chain(coors, xyz, q, feats, gout):
        index = amd.voxel_query_index(coors, shape, B)
        nc = amd.voxel_query_coords(q, counts, (1, 1, 1), (0, 0, 0, 14, 12, 5), 1)
        out, idx = mod(xyz, q, nc, index, feats)
        grad, = torch.autograd.grad(out, feats, gout)
        return nc, out, idx, grad

    def inputs(seed_perm):
        perm = gen.permutation(N) if seed_perm else np.arange(N)
        q = scene.new_xyz[gen.permutation(M)] if seed_perm else scene.new_xyz
        g = gen.integers(-4, 5, (M, 3 + C, nsample)).astype(np.float32)          # integer-valued: the atomic sums are exact in any order
        return (t(scene.coors[perm], dev, torch.int32), t(scene.xyz[perm], dev), t(q, dev),
                t(gen.standard_normal((N, C)).astype(np.float32), dev).requires_grad_(True), t(g, dev))

    static = inputs(False)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        chain(*static)                                                           # warm-up: library, workspace sizes
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        recorded = chain(*static)
    fresh = inputs(True)
    eager = [x.clone() for x in chain(*fresh)]
    with torch.no_grad():
        for s, f in zip(static, fresh):
            s.copy_(f)
    graph.replay()
    torch.cuda.synchronize(dev)
    assert (eager[1] != 0).any() and (eager[3] != 0).any()
    for got, want, what in zip(recorded, eager, ('new_coords', 'new_features', 'idx', 'grad_features')):
        assert torch.equal(got, want), what
