"""The multi-view pillar encoder's view ops through the `_cpu` twins (csrc/view_net_cpu.cpp): `multi_view_voxelize` / `to_cylindrical` /
`to_spherical`, `pillar_scatter` / `PointPillarsScatter` and `view_sample` on CPU tensors against the statement-by-statement torch
restatement of the reference and the numpy restatement of the library's fixed fp32 sequences (tests/view_net_ref.py), and against the
real reference's recorded runs (tests/golden/view_net.npz).

  * transforms: points and coors bit-identical to the numpy restatement in both input forms; every column within the larger of 4x the
    fp32 torch statements' own largest deviation from fp64 and one fp32 ulp of the column's largest magnitude; the recorded cells of the
    real reference reproduced EXACTLY (its points keep 1e-5 from every cell face); points on the faces against the numpy restatement;
  * the canvas and its gathered gradient `torch.equal` to the restated module in both layouts;
  * the sampled features bit-identical to the numpy restatement in both layouts and within the same bound rule of the fp64 loop, with
    the map's gradient; the order-free backward EQUAL to fp64;
and the autograd wiring, the dtype rule, the argument checks and the twins under sanitizers as a stand-alone program.  The `check_*`
helpers are shared with tests/test_gpu_view_net.py.

Figures (this file's printed output): over the transform cases the angle columns stay within 2.4e-7 rad of fp64 where the
fp32 torch statements stay within 2.2e-7; the largest ratio to the bound is 0.94, on a 64-point case whose bound is the one-ulp term
(2.5e-7 at pi) because torch's own deviation on those points is 5.7e-8.  view_sample's largest ratio to its bound is 0.42; on the real
reference's recorded runs every tensor sits at or below 0.25 of its bound (the fp32 run's own deviation)."""
import numpy as np
import pytest
import torch

import mmdet3d_gaussian_amd as amd
import view_net_ref as ref
from mmdet3d_gaussian_amd import _host, view_net

LAYOUTS = ('nchw', 'channels_last')
SENTINEL = -77.0


def in_layout(t, layout):
    return t.contiguous(memory_format=torch.channels_last) if layout == 'channels_last' else t.contiguous()


def geometry(views):
    return [ref.GEOMETRY[v][0] for v in views], [ref.GEOMETRY[v][1] for v in views]


def equal_bits(t, a):
    """a torch tensor against a numpy array: same shape, dtype and bits (NaN payloads aside)"""
    got = t.detach().cpu().numpy()
    return got.shape == a.shape and got.dtype == a.dtype and np.array_equal(got, a, equal_nan=True)


# ---- transforms --------------------------------------------------------------------------------------------------------------------

def check_transform_case(n, C, views, dev='cpu'):
    """both input forms against the numpy restatement, bit for bit; the list form against the fp64 statements -> the figures"""
    pts, r32, r64 = ref.transform_reference(n, C, views)
    sizes, ranges = geometry(views)
    counts = ref.split_counts(n)
    parts = [p.to(dev) for p in torch.split(pts, counts)]
    mp, mc = amd.multi_view_voxelize(parts, views, sizes, ranges)
    want_p, want_c = ref.np_multi_view(pts.numpy(), counts, views, sizes, ranges)
    got = {}
    for i, v in enumerate(views):
        assert mp[i].shape == (n, C) and mp[i].dtype == torch.float32 and mc[i].shape == (n, 4) and mc[i].dtype == torch.int32
        assert mp[i].device.type == torch.device(dev).type and mc[i].device.type == torch.device(dev).type
        assert equal_bits(mp[i], want_p[i]), f'{v}: points'
        assert equal_bits(mc[i], want_c[i]), f'{v}: coors'
        assert n == 0 or bool((mc[i][:, 0].cpu() == torch.repeat_interleave(torch.arange(3), torch.tensor(counts))).all()), 'the id is in every row'
        for j in range(C):
            got[f'v{i}.c{j}'] = mp[i][:, j].cpu()
    figures = ref.check_values(got, r32, r64, sorted(got), f'{dev} n={n} C={C} {"+".join(views)}')
    stacked = pts.to(dev)
    cnt = torch.tensor(ref.stacked_counts(n), dtype=torch.int32, device=dev)
    sp, sc = amd.multi_view_voxelize(stacked, views, sizes, ranges, cnt)
    want_p, want_c = ref.np_multi_view(pts.numpy(), ref.stacked_counts(n), views, sizes, ranges)
    for i, v in enumerate(views):
        assert equal_bits(sp[i], want_p[i]) and equal_bits(sc[i], want_c[i]), v
        if v == 'cartesian':
            assert sp[i].data_ptr() == stacked.data_ptr(), 'the stacked input itself, not a copy'
        if n >= 3:
            assert bool((sc[i][-2:] == -1).all()) and int(sc[i][n - 3, 0]) == 2, 'only a row of no sample is all -1'
    return figures


@pytest.mark.parametrize('views', ref.VIEW_SETS, ids='+'.join)
@pytest.mark.parametrize('C', ref.TRANSFORM_C)
@pytest.mark.parametrize('n', ref.TRANSFORM_N)
def test_transforms_twin_matches_the_restatements(n, C, views):
    check_transform_case(n, C, views)


def check_single_transforms(dev='cpu'):
    pts = ref.transform_points(65, 5)
    for fn, view in ((amd.to_cylindrical, 'cylindrical'), (amd.to_spherical, 'spherical')):
        out = fn(pts.to(dev))
        assert out.shape == pts.shape and equal_bits(out, ref.np_transform(view, pts.numpy()))
        assert equal_bits(fn(pts.double().to(dev)), ref.np_transform(view, pts.numpy())), 'other dtypes are evaluated in fp32'
        assert fn(pts[:0].to(dev)).shape == (0, 5)
    origin = amd.to_spherical(torch.zeros(1, 3, device=dev))
    assert not origin.any() and bool(torch.isnan(ref.to_spherical(torch.zeros(1, 3))[0, 1])), 'restated: 0 where the reference is NaN'


def test_to_cylindrical_and_to_spherical_go_through_the_same_sequence():
    check_single_transforms()


def check_transform_faces(dev='cpu'):
    """points on cell faces and one ulp either side: the numpy restatement's cells (the fp64 statements may differ there)"""
    pts = ref.face_points()
    sizes, ranges = geometry(('cartesian',))
    _, mc = amd.multi_view_voxelize([pts.to(dev)], ('cartesian',), sizes, ranges)
    _, want = ref.np_multi_view(pts.numpy(), [len(pts)], ('cartesian',), sizes, ranges)
    assert equal_bits(mc[0], want[0])
    c = mc[0].cpu()
    assert bool((c[0, 1:] == -1).all()) and int(c[1, 3]) == 0 and int(c[2, 3]) == 0, 'below, on and above the first x face'
    assert bool((c[:, 0] == 0).all()) and bool((c[:, 1:] == -1).all(dim=1).any()) and bool((c[:, 1:] >= 0).all(dim=1).any())


def test_transforms_on_cell_faces_follow_the_fixed_sequence():
    check_transform_faces()


def check_transform_robustness(dev='cpu'):
    """NaN, +-inf, +-1e30: dropped, the id column kept, the features copied; the origin and x = 0 are ordinary finite points"""
    pts, bad = ref.robustness_points()
    views = ('cartesian', 'cylindrical', 'spherical')
    ranges = [(-20.0, -20.0, -3.0, 20.0, 20.0, 1.0), (-3.2, -3.0, 0.0, 3.2, 1.0, 100.0), (-3.2, -1.6, 0.0, 3.2, 1.6, 100.0)]
    sizes = [(0.16, 0.16, 4.0), (0.0025, 0.04, 100.0), (0.0025, 0.005, 100.0)]
    n = len(pts)
    mp, mc = amd.multi_view_voxelize([pts[:6].to(dev), pts[6:].to(dev)], views, sizes, ranges)
    want_p, want_c = ref.np_multi_view(pts.numpy(), [6, n - 6], views, sizes, ranges)
    ids = torch.tensor([0] * 6 + [1] * (n - 6), dtype=torch.int32)
    for i, v in enumerate(views):
        c, p = mc[i].cpu(), mp[i].cpu()
        assert equal_bits(c, want_c[i]), v
        assert torch.equal(c[:, 0], ids) and bool((c[:bad, 1:] == -1).all()), f'{v}: dropped, the id kept'
        assert bool((c[bad:, 1:] >= 0).all()), f'{v}: the origin, x = 0 and the ordinary row are kept'
        assert torch.equal(p[:, 3:], pts[:, 3:]), f'{v}: the features are copied'
        assert equal_bits(p[bad:], want_p[i][bad:]) and bool(torch.isfinite(p[bad:]).all())
    half_pi = float(np.float32(1.5707963267948966))
    assert mp[1][bad:bad + 3, 0].tolist() == [0.0, half_pi, -half_pi] and mp[2][bad, 1].item() == 0.0


def test_transforms_drop_non_finite_rows_and_keep_their_ids():
    check_transform_robustness()


def golden_inputs(name, dev):
    g = ref.golden()
    views = [str(v) for v in g[f'{name}.views']]
    counts = g[f'{name}.counts'].tolist()
    parts = [p.to(dev) for p in torch.split(torch.from_numpy(g[f'{name}.points']), counts)]
    return g, views, parts, g[f'{name}.voxel_sizes'].tolist(), g[f'{name}.ranges'].tolist()


def check_golden_transforms(name, dev='cpu'):
    """the real reference's recorded run: the cells EXACTLY (no share of mismatches), the points within the bound of its fp64 run"""
    g, views, parts, sizes, ranges = golden_inputs(name, dev)
    mp, mc = amd.multi_view_voxelize(parts, views, sizes, ranges)
    got, r32, r64 = {}, {}, {}
    for i, v in enumerate(views):
        assert np.array_equal(mc[i].cpu().numpy(), g[f'{name}.view{i}.coors32']), f'{name} {v}: the reference\'s cells'
        for j in range(3):
            key = f'v{i}.c{j}'
            got[key] = mp[i][:, j].cpu()
            r32[key], r64[key] = torch.from_numpy(g[f'{name}.view{i}.points32'][:, j]), torch.from_numpy(g[f'{name}.view{i}.points64'][:, j])
        assert np.array_equal(mp[i][:, 3:].cpu().numpy(), g[f'{name}.view{i}.points32'][:, 3:])
    return ref.check_values(got, r32, r64, sorted(got), f'{dev} golden {name}')


@pytest.mark.parametrize('name', ['cyl', 'cart'])
def test_transforms_reproduce_the_real_references_cells(name):
    check_golden_transforms(name)


# ---- pillar_scatter ----------------------------------------------------------------------------------------------------------------

def run_scatter(case, layout, dev='cpu', dtype=torch.int64, cols=4, view=lambda t: t):
    f = view(case['feats'].to(dev).clone()).requires_grad_(True)
    coors = case['coors'].to(dev).to(dtype)
    canvas = amd.pillar_scatter(f, coors if cols == 4 else coors[:, 1:], case['B'], (case['ny'], case['nx']), channels_last=layout == 'channels_last')
    assert canvas.shape == (case['B'], f.size(1), case['ny'], case['nx']) and canvas.dtype == torch.float32
    assert canvas.is_contiguous(memory_format=torch.channels_last if layout == 'channels_last' else torch.contiguous_format)
    canvas.backward(in_layout(case['grad'].to(dev), layout))
    return dict(canvas=canvas.detach().cpu().contiguous(), grad=f.grad.cpu())


def check_scatter_case(V, C, B, ny, nx, dev='cpu'):
    case = ref.scatter_case(V, C, B, ny, nx)
    want_canvas, want_grad = ref.scatter_reference(case)
    for layout in LAYOUTS:
        for dtype in (torch.int32, torch.int64):
            got = run_scatter(case, layout, dev, dtype)
            assert torch.equal(got['canvas'], want_canvas), (layout, dtype)
            assert torch.equal(got['grad'], want_grad), (layout, dtype)
        if B == 1:                                  # (V, 3) coors carry no b: the rows of sample 0, those outside in y or x included
            rows = case['coors'][:, 0] == 0
            single = dict(case, feats=case['feats'][rows], coors=case['coors'][rows])
            got = run_scatter(single, layout, dev, cols=3)
            assert torch.equal(got['canvas'], want_canvas) and torch.equal(got['grad'], want_grad[rows]), f'{layout}: (V, 3) coors'
    if V >= 63:
        c = case['coors']
        outside = (c[:, 0] < 0) | (c[:, 0] >= B) | (c[:, 2] < 0) | (c[:, 2] >= ny) | (c[:, 3] < 0) | (c[:, 3] >= nx)
        assert int(outside.sum()) >= 6 and not want_grad[outside].any() and bool(want_grad[~outside].ne(0).any(dim=1).all())


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('C', ref.SCATTER_C)
@pytest.mark.parametrize('V', ref.SCATTER_V)
def test_pillar_scatter_twin_equals_the_restated_module(V, C, B):
    check_scatter_case(V, C, B, *ref.SCATTER_CANVAS)


@pytest.mark.parametrize('shape', [(1, 1), (1, 9), (9, 1)])
def test_pillar_scatter_on_degenerate_canvases(shape):
    check_scatter_case(65, 3, 3, *shape)


def scatter_entries(case, layout, dev='cpu', shift=False):
    """`gd3d_pillar_scatter` and `gd3d_pillar_scatter_backward` (or their twins) on sentinel-filled buffers with a guard band either
    side; `shift`: the features, the canvas and both gradients start one float into a larger buffer.  Asserts that every element is
    written and no guard is -> (canvas as it lies in memory, grad_features) on the CPU"""
    feats, coors = case['feats'].to(dev).contiguous(), case['coors'].to(dev).contiguous()
    V, C = feats.shape
    B, ny, nx = case['B'], case['ny'], case['nx']
    flag = int(layout == 'channels_last')
    g = in_layout(case['grad'].to(dev), layout)
    g = g.permute(0, 2, 3, 1) if flag else g
    assert g.is_contiguous()
    if shift:
        feats, g = ref.offset_view(feats), ref.offset_view(g)
    off, band, total = int(shift), 64, B * C * ny * nx
    buf = torch.full((total + 2 * band + 8,), SENTINEL, device=dev)
    canvas = buf[off + band:off + band + total]
    _host.call('gd3d_pillar_scatter', feats.device, (feats.data_ptr(), coors.data_ptr(), 1, 4, flag, V, C, B, ny, nx, canvas.data_ptr()))
    assert (buf[:off + band] == SENTINEL).all() and (buf[off + band + total:] == SENTINEL).all(), 'a guard was written'
    assert not (canvas == SENTINEL).any(), 'an element of the canvas was left unwritten'
    gbuf = torch.full((V * C + 2 * band + 8,), SENTINEL, device=dev)
    grad = gbuf[off + band:off + band + V * C]
    _host.call('gd3d_pillar_scatter_backward', feats.device, (g.data_ptr(), coors.data_ptr(), 1, 4, flag, V, C, B, ny, nx, grad.data_ptr()))
    assert (gbuf[:off + band] == SENTINEL).all() and (gbuf[off + band + V * C:] == SENTINEL).all(), 'a guard was written'
    assert not (grad == SENTINEL).any(), 'a gradient element was left unwritten'
    return canvas.cpu().clone(), grad.view(V, C).cpu().clone()


def check_scatter_entries(dev='cpu'):
    """through the C entries: every element written and nothing beyond; an offset-by-one-float base gives the aligned run's bits"""
    for C in (3, 64):
        case = ref.scatter_case(1025, C, 3, *ref.SCATTER_CANVAS)
        want_canvas, want_grad = ref.scatter_reference(case)
        for layout in LAYOUTS:
            canvas, grad = scatter_entries(case, layout, dev)
            lie = want_canvas.permute(0, 2, 3, 1) if layout == 'channels_last' else want_canvas
            assert torch.equal(canvas, lie.reshape(-1)) and torch.equal(grad, want_grad), (C, layout)
            canvas2, grad2 = scatter_entries(case, layout, dev, shift=True)
            assert torch.equal(canvas2, canvas) and torch.equal(grad2, grad), f'{C} {layout}: the 4-byte path'


def test_pillar_scatter_entries_write_every_element_and_nothing_beyond():
    check_scatter_entries()


def check_scatter_module(dev='cpu'):
    case = ref.scatter_case(63, 64, 3, *ref.SCATTER_CANVAS)
    want, _ = ref.scatter_reference(case)
    m = amd.PointPillarsScatter(64, ref.SCATTER_CANVAS)
    assert (m.ny, m.nx, m.in_channels) == (5, 7, 64)
    assert torch.equal(m(case['feats'].to(dev), case['coors'].to(dev), 3).cpu(), want)
    single = ref.scatter_case(63, 64, 1, *ref.SCATTER_CANVAS)
    want1, _ = ref.scatter_reference(single)
    rows = single['coors'][:, 0] == 0
    assert torch.equal(m(single['feats'][rows].to(dev), single['coors'][rows][:, 1:].to(dev)).cpu(), want1), 'forward_single'
    assert torch.equal(m(single['feats'][rows].to(dev), single['coors'][rows].to(dev)).cpu(), want1), 'forward_single ignores a batch column'
    last = amd.PointPillarsScatter(64, ref.SCATTER_CANVAS, channels_last=True)(case['feats'].to(dev), case['coors'].to(dev), 3)
    assert last.is_contiguous(memory_format=torch.channels_last) and torch.equal(last.cpu().contiguous(), want)
    half = amd.pillar_scatter(case['feats'].half().to(dev), case['coors'].to(dev), 3, ref.SCATTER_CANVAS)
    assert half.dtype == torch.float16 and torch.equal(half.cpu(), want.half())
    assert amd.pillar_scatter(case['feats'].to(dev), case['coors'].to(dev), 0, ref.SCATTER_CANVAS).shape == (0, 64, 5, 7)


def test_point_pillars_scatter_has_mmdet3ds_surface():
    check_scatter_module()


# ---- view_sample -------------------------------------------------------------------------------------------------------------------

def run_sample(case, layout, dev='cpu', view=lambda t: t, backward=True, ids='vector', id_dtype=torch.int64):
    """the package's features and map gradient of a case on `dev` -> dict on the CPU; the points go in as the [:, :3] view of (N, 5) rows"""
    m = view(in_layout(case['map'].to(dev), layout).clone()).requires_grad_(backward)
    pts = case['pts'].to(dev)
    assert pts.size(1) == 5
    i = case['ids'].to(dev).to(id_dtype)
    if ids == 'coors':
        i = torch.cat([i.unsqueeze(1), torch.full((len(i), 3), 5, dtype=id_dtype, device=dev)], 1)
    out = amd.view_sample(m, pts[:, :3], i, case['rng'])
    assert out.is_contiguous() and out.dtype == torch.float32 and out.shape == (pts.size(0), m.size(1))
    if not backward:
        return dict(out=out.detach().cpu())
    out.backward(view(case['grad_out'].to(dev)))
    assert m.grad.stride() == m.stride(), 'the gradient comes in the caller\'s layout'
    return dict(out=out.detach().cpu(), grad_map=m.grad.cpu().contiguous())


def numpy_sample(case):
    return ref.np_view_sample(case['map'].numpy(), case['pts'][:, :2].numpy(), case['ids'].numpy(), case['rng'])


def check_sample_case(name, dev='cpu'):
    """the assertions the CPU and the GPU file share -> the figures per layout"""
    case, r32, r64 = ref.sample_reference(name)
    want = numpy_sample(case)
    figures, got = {}, {}
    for layout in LAYOUTS:
        got[layout] = run_sample(case, layout, dev)
        if case['kind'] != 'huge':           # the reference's row for a non-finite coordinate is NaN: restated (a zero row), not matched
            figures[layout] = ref.check_values(got[layout], r32, r64, ref.SAMPLE_KEYS, f'{dev} {layout} {name}')
        assert equal_bits(got[layout]['out'], want), f'{layout}: the numpy restatement\'s bits'
        assert torch.equal(run_sample(case, layout, dev, backward=False)['out'], got[layout]['out']), f'{layout}: run to run'
    assert torch.equal(got['nchw']['out'], got['channels_last']['out']), 'the forward is the same bits in both layouts'
    out, grad = got['nchw']['out'], got['nchw']['grad_map']
    if case['kind'] in ('outside_far', 'huge'):
        assert not out.any() and not grad.any()
    if case['kind'] in ('outer_half', 'outside_near', 'inside'):
        assert bool(out.ne(0).any(dim=1).all())
    if case['kind'] == 'centres':
        ix, iy = ref.pixel64(case['pts'][:, :2], case['rng'], case['map'].size(2), case['map'].size(3))
        assert torch.equal(out, case['map'][case['ids'], :, iy.long(), ix.long()]), 'weights 1 and 0: the cell\'s value itself'
    if case['kind'] == 'bad_ids':
        bad = (case['ids'] < 0) | (case['ids'] >= ref.SAMPLE_B)
        assert bool(bad.any()) and not out[bad].any() and bool(out[~bad].ne(0).any(dim=1).all())
    if case['kind'] == 'empty_sample':
        assert not grad[1].any() and grad[0].any() and grad[2].any()
    return figures


@pytest.mark.parametrize('name', sorted(ref.SAMPLE_CASES))
def test_view_sample_twin_matches_the_restatements(name):
    check_sample_case(name)


def check_sample_id_forms(dev='cpu'):
    """int32 and int64 ids, as a vector and as column 0 of (N, 4) coors: one result"""
    case = ref.sample_reference('bad_ids_c64_5x7')[0]
    want = run_sample(case, 'nchw', dev)
    for form in ('vector', 'coors'):
        for dtype in (torch.int32, torch.int64):
            got = run_sample(case, 'channels_last', dev, ids=form, id_dtype=dtype)
            assert torch.equal(got['out'], want['out']), (form, dtype)


def test_view_sample_reads_the_ids_through_their_stride():
    check_sample_id_forms()


def check_sample_exact(dev='cpu'):
    """the order-free case: features and map gradient EQUAL the fp64 result, in both layouts (on the GPU: both NCHW backward forms)"""
    case, exact = ref.exact_reference()
    forms = (True, False) if dev != 'cpu' else (True,)
    for via in forms:
        view_net.NCHW_BACKWARD_VIA_WORKSPACE, keep = via, view_net.NCHW_BACKWARD_VIA_WORKSPACE
        try:
            for layout in LAYOUTS:
                got = run_sample(case, layout, dev)
                assert torch.equal(got['out'].double(), exact['out']), layout
                assert torch.equal(got['grad_map'].double(), exact['grad_map']), f'{layout} via={via}: exact sums, whatever the order'
        finally:
            view_net.NCHW_BACKWARD_VIA_WORKSPACE = keep
    assert exact['grad_map'].ne(0).any() and not exact['out'][(case['ids'] < 0) | (case['ids'] >= ref.SAMPLE_B)].any()


def test_view_sample_backward_is_exact_on_the_order_free_case():
    check_sample_exact()


def sample_entries(case, layout, dev='cpu', shift=(), workspace=False):
    """`gd3d_view_sample` and `gd3d_view_sample_backward` (or their twins) on sentinel-filled outputs with guard bands; an operand named
    in `shift` ('map', 'out', 'grad_out', 'grad_map') starts one float into a larger buffer.  Asserts that every element is written and
    no guard is -> (out (N, C), grad_map as it lies in memory) on the CPU"""
    pts, ids = case['pts'].to(dev), case['ids'].to(dev)
    m = in_layout(case['map'].to(dev), layout)
    B, C, H, W = m.shape
    N = pts.size(0)
    flag = int(layout == 'channels_last')
    dense = m.permute(0, 2, 3, 1) if flag else m
    assert dense.is_contiguous()
    dense = ref.offset_view(dense) if 'map' in shift else dense
    gout = case['grad_out'].to(dev).contiguous()
    gout = ref.offset_view(gout) if 'grad_out' in shift else gout
    axes = view_net._axes(tuple(float(v) for v in case['rng']))
    band = 64
    off = int('out' in shift)
    buf = torch.full((N * C + 2 * band + 8,), SENTINEL, device=dev)
    out = buf[off + band:off + band + N * C]
    _host.call('gd3d_view_sample', pts.device, (pts.data_ptr(), pts.stride(0), ids.data_ptr(), 1, 1, dense.data_ptr(), flag, N, B, C, H, W, *axes,
                                                out.data_ptr()))
    assert (buf[:off + band] == SENTINEL).all() and (buf[off + band + N * C:] == SENTINEL).all(), 'a guard was written'
    assert not (out == SENTINEL).any(), 'an output element was left unwritten'
    total = B * C * H * W
    off = int('grad_map' in shift)
    gbuf = torch.full((total + 2 * band + 8,), SENTINEL, device=dev)
    grad = gbuf[off + band:off + band + total]
    work = torch.full((total,), SENTINEL, device=dev) if workspace else None
    _host.call('gd3d_view_sample_backward', pts.device, (gout.data_ptr(), pts.data_ptr(), pts.stride(0), ids.data_ptr(), 1, 1, flag, N, B, C, H, W, *axes,
                                                         _host.ptr(work), grad.data_ptr()))
    assert (gbuf[:off + band] == SENTINEL).all() and (gbuf[off + band + total:] == SENTINEL).all(), 'a guard was written'
    assert not (grad == SENTINEL).any(), 'a gradient element was left unwritten'
    return out.view(N, C).cpu().clone(), grad.cpu().clone()


def check_sample_entries(dev='cpu'):
    """guard bands through the C entries, and the 4-byte path (one operand one float off) against the 16-byte path, on the exact case"""
    case, exact = ref.exact_reference()
    for layout in LAYOUTS:
        lie = exact['grad_map'].permute(0, 2, 3, 1) if layout == 'channels_last' else exact['grad_map']
        out, grad = sample_entries(case, layout, dev)
        assert torch.equal(out.double(), exact['out']) and torch.equal(grad.double(), lie.reshape(-1)), layout
        for shift in ('map', 'out', 'grad_out', 'grad_map'):
            out2, grad2 = sample_entries(case, layout, dev, shift=(shift,))
            assert torch.equal(out2, out) and torch.equal(grad2, grad), f'{layout}: {shift} one float off'
        if layout == 'nchw' and dev != 'cpu':
            out3, grad3 = sample_entries(case, layout, dev, workspace=True)
            assert torch.equal(out3, out) and torch.equal(grad3, grad), 'the workspace form'


def test_view_sample_entries_write_every_element_and_nothing_beyond():
    check_sample_entries()


def check_golden_sample(name, dev='cpu'):
    """the real SingleViewNet.forward's recorded run: features and map gradient within the bound its own fp32 and fp64 runs set"""
    g = ref.golden()
    k = int(g[f'{name}.sample.view'])
    pts = torch.from_numpy(g[f'{name}.view{k}.points32']).to(dev)
    coors = torch.from_numpy(g[f'{name}.view{k}.coors32']).to(dev)
    rng = g[f'{name}.ranges'][k].tolist()
    r32 = dict(out=torch.from_numpy(g[f'{name}.sample.out32']), grad_map=torch.from_numpy(g[f'{name}.sample.grad_map32']))
    r64 = dict(out=torch.from_numpy(g[f'{name}.sample.out64']), grad_map=torch.from_numpy(g[f'{name}.sample.grad_map64']))
    figures = {}
    for layout in LAYOUTS:
        m = in_layout(torch.from_numpy(g[f'{name}.sample.map32']).to(dev), layout).requires_grad_(True)
        out = amd.view_sample(m, pts[:, :3], coors, rng)
        out.backward(torch.from_numpy(g[f'{name}.grad_out']).to(dev))
        got = dict(out=out.detach().cpu(), grad_map=m.grad.cpu().contiguous())
        figures[layout] = ref.check_values(got, r32, r64, ref.SAMPLE_KEYS, f'{dev} {layout} golden {name}')
    # the canvas itself: the recorded map is pillar_scatter of the scatter-max features
    feats = torch.from_numpy(g[f'{name}.features'])
    keep = (coors.cpu() >= 0).all(dim=1)
    rows, inv = torch.unique(coors.cpu()[keep].long(), dim=0, return_inverse=True)
    vox = torch.zeros(rows.size(0), feats.size(1)).scatter_reduce(0, inv.unsqueeze(1).expand(-1, feats.size(1)), feats[keep], 'amax', include_self=False)
    H, W = g[f'{name}.sample.shape'].tolist()
    canvas = amd.pillar_scatter(vox.to(dev), rows.to(dev), len(g[f'{name}.counts']), (H, W))
    assert np.array_equal(canvas.cpu().numpy(), g[f'{name}.sample.map32'])
    return figures


@pytest.mark.parametrize('name', ['cyl', 'cart'])
def test_view_sample_stays_within_the_real_references_bound(name):
    check_golden_sample(name)


def test_other_striding_takes_a_copy_and_other_dtypes_are_cast_back():
    case = ref.sample_reference('outer_half_c3_2x2')[0]
    want = run_sample(case, 'nchw')
    wide = torch.randn(ref.SAMPLE_B, 3, 2, 4)
    wide[..., 1:3] = case['map']
    m = wide[..., 1:3].requires_grad_(True)
    assert not m.is_contiguous() and not m.is_contiguous(memory_format=torch.channels_last)
    out = amd.view_sample(m, case['pts'][:, :3], case['ids'], case['rng'])
    out.backward(case['grad_out'])
    assert torch.equal(out.detach(), want['out']) and torch.equal(m.grad, want['grad_map'])
    for dtype in (torch.float16, torch.float64):
        md = case['map'].to(dtype).requires_grad_(True)
        m32 = md.detach().float().requires_grad_(True)
        out, out32 = amd.view_sample(md, case['pts'].to(dtype), case['ids'], case['rng']), amd.view_sample(m32, case['pts'].to(dtype).float(), case['ids'], case['rng'])
        out.backward(case['grad_out'].to(dtype))
        out32.backward(case['grad_out'].to(dtype).float())
        assert out.dtype == dtype and md.grad.dtype == dtype and torch.equal(out.detach(), out32.detach().to(dtype)) and torch.equal(md.grad, m32.grad.to(dtype))


def _count_calls(monkeypatch):
    seen = []
    real = _host.call

    def counted(name, dev, args, cpu_tail=()):
        seen.append(name)
        return real(name, dev, args, cpu_tail)
    monkeypatch.setattr(_host, 'call', counted)
    return lambda: len(seen)


def test_autograd_wiring(monkeypatch):
    case = ref.sample_reference('outer_half_c64_5x7')[0]
    want = run_sample(case, 'nchw')
    n = _count_calls(monkeypatch)
    m = case['map'].clone().requires_grad_(True)
    out = amd.view_sample(m, case['pts'], case['ids'], case['rng'])
    assert out.requires_grad and n() == 1 and len(out.grad_fn.saved_tensors) == 2      # the points and the ids; the map is not kept
    (g1,) = torch.autograd.grad(out, m, case['grad_out'], retain_graph=True)
    (g2,) = torch.autograd.grad(out, m, case['grad_out'])
    assert torch.equal(g1, want['grad_map']) and torch.equal(g2, g1) and n() == 3
    with torch.no_grad():
        quiet = amd.view_sample(m, case['pts'], case['ids'], case['rng'])
    assert not quiet.requires_grad and quiet.grad_fn is None and torch.equal(quiet, want['out'])
    assert not amd.view_sample(case['map'], case['pts'].clone().requires_grad_(True), case['ids'], case['rng']).requires_grad
    (g,) = torch.autograd.grad(amd.view_sample(m, case['pts'], case['ids'], case['rng']).sum(), m, create_graph=True)
    with pytest.raises(RuntimeError, match='differentiate twice'):
        g.sum().backward()
    sc = ref.scatter_case(63, 3, 3, *ref.SCATTER_CANVAS)
    f = sc['feats'].clone().requires_grad_(True)
    canvas = amd.pillar_scatter(f, sc['coors'], 3, ref.SCATTER_CANVAS)
    assert canvas.requires_grad and len(canvas.grad_fn.saved_tensors) == 1
    (g,) = torch.autograd.grad(canvas.sum(), f, create_graph=True)
    with pytest.raises(RuntimeError, match='differentiate twice'):
        g.sum().backward()
    with torch.no_grad():
        assert amd.pillar_scatter(f, sc['coors'], 3, ref.SCATTER_CANVAS).grad_fn is None
    calls = n()
    assert amd.view_sample(torch.zeros(2, 3, 5, 7, requires_grad=True), torch.zeros(0, 3), torch.zeros(0, dtype=torch.int64), case['rng']).shape == (0, 3)
    assert amd.view_sample(torch.zeros(0, 3, 5, 7), torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64), case['rng']).shape == (4, 3)
    assert n() == calls, 'N == 0 or B == 0 launches nothing'


def test_every_argument_check_raises_before_touching_the_library(monkeypatch):
    def no_library(*a, **k):
        raise AssertionError('an argument check must raise before the library is reached')
    monkeypatch.setattr(_host, 'call', no_library)
    pts, m, ids, rng = torch.zeros(4, 3), torch.zeros(2, 3, 5, 7), torch.zeros(4, dtype=torch.int64), (0.0, 0.0, 0.0, 1.0, 1.0, 1.0)
    for bad in ((pts[:, :1], m, ids, rng), (pts[0], m, ids, rng), (pts.long(), m, ids, rng), (pts, m[0], ids, rng), (pts, m.long(), ids, rng),
                (pts, m, ids[:3], rng), (pts, m, torch.zeros(4, 2, 2, dtype=torch.int64), rng)):
        with pytest.raises(RuntimeError, match='shape mismatch'):
            amd.view_sample(bad[1], bad[0], bad[2], bad[3])
    with pytest.raises(RuntimeError, match='int32 or int64'):
        amd.view_sample(m, pts, ids.float(), rng)
    with pytest.raises(RuntimeError, match='is on'):
        amd.view_sample(m.to('meta'), pts, ids, rng)
    with pytest.raises(RuntimeError, match='must hold 6'):
        amd.view_sample(m, pts, ids, rng[:4])
    with pytest.raises(RuntimeError, match='positive finite extent'):
        amd.view_sample(m, pts, ids, (0.0, 0.0, 0.0, 0.0, 1.0, 1.0))
    with pytest.raises(RuntimeError, match='C >= 1'):
        amd.view_sample(torch.zeros(2, 0, 5, 7), pts, ids, rng)
    f, c = torch.zeros(4, 3), torch.zeros(4, 4, dtype=torch.int64)
    for bad in ((f[0], c), (f.long(), c), (f, c[:3]), (f, c[:, :2]), (f, c[0])):
        with pytest.raises(RuntimeError, match='shape mismatch'):
            amd.pillar_scatter(bad[0], bad[1], 2, (5, 7))
    with pytest.raises(RuntimeError, match='int32 or int64'):
        amd.pillar_scatter(f, c.float(), 2, (5, 7))
    with pytest.raises(RuntimeError, match='is on'):
        amd.pillar_scatter(f, c.to('meta'), 2, (5, 7))
    with pytest.raises(RuntimeError, match='batch_size'):
        amd.pillar_scatter(f, c, -1, (5, 7))
    with pytest.raises(RuntimeError, match='batch_size'):
        amd.pillar_scatter(f, c[:, 1:], 2, (5, 7))
    with pytest.raises(RuntimeError, match='output_shape'):
        amd.pillar_scatter(f, c, 2, (5, 7, 1))
    with pytest.raises(RuntimeError, match='ny, nx'):
        amd.pillar_scatter(f, c, 2, (0, 7))
    with pytest.raises(RuntimeError, match='shape mismatch'):
        amd.PointPillarsScatter(4, (5, 7))(f, c, 2)
    p = [torch.zeros(4, 4)]
    vs, r = [(1.0, 1.0, 1.0)], [(0.0, 0.0, 0.0, 4.0, 4.0, 4.0)]
    with pytest.raises(RuntimeError, match='1 to 4 names'):
        amd.multi_view_voxelize(p, [], [], [])
    with pytest.raises(RuntimeError, match='1 to 4 names'):
        amd.multi_view_voxelize(p, 'cartesian', vs, r)
    with pytest.raises(RuntimeError, match='1 to 4 names'):
        amd.multi_view_voxelize(p, ['cartesian'] * 5, vs * 5, r * 5)
    with pytest.raises(RuntimeError, match="'cartesian', 'cylindrical' or 'spherical'"):
        amd.multi_view_voxelize(p, ['polar'], vs, r)
    with pytest.raises(RuntimeError, match='one voxel size and one range each'):
        amd.multi_view_voxelize(p, ['cartesian', 'spherical'], vs, r)
    with pytest.raises(RuntimeError, match='must hold 3'):
        amd.multi_view_voxelize(p, ['cartesian'], [(1.0, 1.0)], r)
    with pytest.raises(RuntimeError, match='shape mismatch'):
        amd.multi_view_voxelize([torch.zeros(4, 2)], ['cartesian'], vs, r)
    with pytest.raises(RuntimeError, match='non-empty list'):
        amd.multi_view_voxelize([], ['cartesian'], vs, r)
    with pytest.raises(RuntimeError, match='shape mismatch'):
        amd.to_cylindrical(torch.zeros(4, 2))
    with pytest.raises(RuntimeError, match='shape mismatch'):
        amd.to_spherical(torch.zeros(4, 3).long())
    for name in ('multi_view_voxelize', 'to_cylindrical', 'to_spherical', 'pillar_scatter', 'PointPillarsScatter', 'view_sample'):
        assert name in amd.__all__


def test_host_twins_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """csrc/view_net_cpu.cpp compiled together with a stand-alone driver (tests/hostmath/view_net_sanitize.cpp, its own main) under
    -fsanitize=address,undefined and run as a program on the CPU: exactly sized heap blocks, every view set, both layouts, NaN, +-inf and
    +-1e30 coordinates, out-of-range ids and coors.  The device kernels share that index code.  A sanitizer build belongs on a CPU-only
    machine: with a GPU present the test skips before it compiles or starts anything."""
    if torch.cuda.is_available():
        pytest.skip('sanitizer builds run on a CPU-only machine, never where a GPU is present')
    import os
    import subprocess
    from mmdet3d_gaussian_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = _lib._build.host_cxx_path()
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'view_net_sanitize')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined,float-cast-overflow', '-fno-sanitize-recover=all', '-ffp-contract=off',
           os.path.join(root, 'tests', 'hostmath', 'view_net_sanitize.cpp'),
           os.path.join(root, 'mmdet3d-gaussian_amd', 'csrc', 'view_net_cpu.cpp'), '-o', exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.rstrip().endswith('OK') and 'runtime error' not in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
