"""The multi-view pillar encoder's view ops on the MI355X (csrc/view_net.hip): the cases of tests/test_cpu_view_net.py on cuda:0.  The
transformed points and coors bit-identical to the `_cpu` twin and to the numpy restatement, within the bound of the fp64 statements, the
real reference's cells reproduced exactly; the canvas and its gathered gradient equal to the restated module in both layouts (the LDS
tile and the row kernels); the sampled features bit-identical to the twin, between the layouts and from run to run, with the map's
gradient within the bound; the order-free backward EQUAL to fp64 through the atomics, in channels last, in NCHW and through the
channels-last workspace and its transpose; every output element written and nothing beyond; the 4-byte paths equal to the 16-byte paths;
and the chain pillar_scatter -> network stand-in -> view_sample, forward and backward, captured in one graph.

No kernel here has a capped grid (a workgroup owns its rows; csrc/view_net.hip), so there is no grid-stride sweep to test: the cases
past one workgroup, one wave and one LDS tile (63, 65, 1025, 2049, 4099 rows) cover every launch shape.

Figures: every case passes on gfx950; DESIGN.md §3.16 holds the largest ratios to the bounds."""
import pytest
import torch

import mmdet3d_gaussian_amd as amd
import view_net_ref as ref
from test_cpu_view_net import (LAYOUTS, check_golden_sample, check_golden_transforms, check_sample_case, check_sample_entries, check_sample_exact,
                               check_sample_id_forms, check_scatter_case, check_scatter_entries, check_scatter_module, check_single_transforms,
                               check_transform_case, check_transform_faces, check_transform_robustness, geometry, run_sample)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.mark.parametrize('views', ref.VIEW_SETS, ids='+'.join)
@pytest.mark.parametrize('C', ref.TRANSFORM_C)
@pytest.mark.parametrize('n', ref.TRANSFORM_N)
def test_transforms_on_the_device(n, C, views):
    """against the numpy restatement bit for bit (as the twin is: tests/test_cpu_view_net.py), hence the twin's bits"""
    check_transform_case(n, C, views, DEV)
    pts = ref.transform_points(n, C)
    sizes, ranges = geometry(views)
    on_dev = amd.multi_view_voxelize([pts.to(DEV)], views, sizes, ranges)
    twin = amd.multi_view_voxelize([pts], views, sizes, ranges)
    for got, want in zip(on_dev[0] + on_dev[1], twin[0] + twin[1]):
        assert torch.equal(got.cpu(), want)


def test_single_transforms_faces_and_robustness_on_the_device():
    check_single_transforms(DEV)
    check_transform_faces(DEV)
    check_transform_robustness(DEV)


@pytest.mark.parametrize('name', ['cyl', 'cart'])
def test_the_real_references_recorded_runs_on_the_device(name):
    check_golden_transforms(name, DEV)
    check_golden_sample(name, DEV)


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('C', ref.SCATTER_C)
@pytest.mark.parametrize('V', ref.SCATTER_V)
def test_pillar_scatter_on_the_device(V, C, B):
    check_scatter_case(V, C, B, *ref.SCATTER_CANVAS, dev=DEV)


@pytest.mark.parametrize('shape', [(1, 1), (1, 9), (9, 1)])
def test_pillar_scatter_on_degenerate_canvases(shape):
    check_scatter_case(65, 3, 3, *shape, dev=DEV)


def test_pillar_scatter_entries_and_module_on_the_device():
    check_scatter_entries(DEV)
    check_scatter_module(DEV)


@pytest.mark.parametrize('name', sorted(ref.SAMPLE_CASES))
def test_view_sample_on_the_device(name):
    check_sample_case(name, DEV)
    case = ref.sample_reference(name)[0]
    twin = run_sample(case, 'nchw', 'cpu', backward=False)['out']
    for layout in LAYOUTS:
        assert torch.equal(run_sample(case, layout, DEV, backward=False)['out'], twin), f'{layout}: the forward is the twin\'s bits'


def test_view_sample_id_forms_exact_backward_and_entries_on_the_device():
    check_sample_id_forms(DEV)
    check_sample_exact(DEV)          # channels last, NCHW direct, NCHW through the workspace and its transpose
    check_sample_entries(DEV)


def test_view_stage_under_graph_capture():
    """pillar_scatter -> an elementwise stand-in for the view network -> view_sample, with the gradients of the voxel features and of the
    network's weight: recorded on a single stream in ONE graph (a host sync inside the capture would raise), replayed twice — the second
    time on new values in the static buffers — and compared with the eager run bit for bit.  The order-free case: points on sixteenths
    of a cell of a 4 x 8 map, small-integer features, weights and gradients, so the atomically summed gradient is exact in any order."""
    case, _ = ref.exact_reference()
    B, C, H, W = case['map'].shape
    g = torch.Generator().manual_seed(11)
    cells = torch.randperm(B * H * W, generator=g)[:70].sort().values
    coors = torch.stack([cells // (H * W), torch.zeros(70, dtype=torch.int64), (cells // W) % H, cells % W], 1).to(DEV)
    feats = torch.randint(-4, 5, (70, C), generator=g).float().to(DEV).requires_grad_(True)
    weight = torch.randint(-2, 3, (1, C, 1, 1), generator=g).float().to(DEV).requires_grad_(True)
    pts, ids, gout = case['pts'].to(DEV), case['ids'].to(DEV), case['grad_out'].to(DEV)

    def step(channels_last):
        canvas = amd.pillar_scatter(feats, coors, B, (H, W), channels_last=channels_last)
        out = amd.view_sample(canvas * weight + 1.0, pts[:, :3], ids, case['rng'])
        g_feats, g_weight = torch.autograd.grad(out, [feats, weight], gout)
        return [canvas, out, g_feats, g_weight]

    for channels_last in (False, True):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            first = [t.detach().clone() for t in step(channels_last)]      # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        assert first[1].any() and first[2].any() and first[3].any()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = step(channels_last)
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(captured, first):
            assert torch.equal(got.detach(), want)
        with torch.no_grad():                                               # new values in the static buffers
            feats.add_(1.0)
            ids.copy_((ids + 1).clamp(max=B))
        graph.replay()
        torch.cuda.synchronize()
        eager = step(channels_last)
        assert not torch.equal(eager[1], first[1]) and not torch.equal(eager[2], first[2])
        for got, want in zip(captured, eager):
            assert torch.equal(got.detach(), want.detach())
        with torch.no_grad():
            feats.sub_(1.0)
            ids.copy_(case['ids'].to(DEV))
