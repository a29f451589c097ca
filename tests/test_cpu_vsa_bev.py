"""The keypoint BEV interpolation, the voxel centres and the keypoint gather through the `_cpu` twins (csrc/vsa_bev_cpu.cpp):
`bev_interpolate`, `voxel_centers` and `sample_keypoints` on CPU tensors against the statement-by-statement torch restatement of the
reference (tests/vsa_bev_ref.py).

  * the interpolated features and the map's gradient within the larger of 4x the fp32 restatement's own largest deviation from fp64 on
    the same inputs and one fp32 ulp (2^-23) of the tensor's largest fp64 magnitude, on every case and in both layouts (printed per
    case; DESIGN.md §3.13 records the largest ratios);
  * the forward bit-identical between contiguous NCHW and channels last; the integer-exact backward equal to fp64;
  * the voxel centres `torch.equal` to the fp32 restatement, the counts equal to its loop's;
  * `sample_keypoints` equal to the reference's per-sample loop;
and the autograd wiring, the dtype rule, the argument checks and the twins under sanitizers as a stand-alone program.

Figures: every case passes, on the `_cpu` twin and on gfx950; the largest |ours - fp64| / bound per tensor is in DESIGN.md §3.13's table."""
import pytest
import torch

import mmdet3d_gaussian_amd as amd
import vsa_bev_ref as ref
from mmdet3d_gaussian_amd import _host, vsa_bev

LAYOUTS = ('nchw', 'channels_last')


def in_layout(t, layout):
    """a (B, C, H, W) tensor's values in the named memory layout"""
    return t.contiguous(memory_format=torch.channels_last) if layout == 'channels_last' else t.contiguous()


def geometry(case):
    return case['voxel_size'], case['point_cloud_range'], case['scale'], case['align']


def run_interp(case, layout, dev='cpu', view=lambda t: t, backward=True):
    """the package's features and map gradient of a case on `dev` -> dict like vsa_bev_ref.evaluate_interp's (on the CPU); `backward`
    False: the features alone"""
    bev = view(in_layout(case['bev'].to(dev), layout).clone()).requires_grad_(backward)     # never the shared case tensor itself
    kp = case['keypoints'].to(dev)
    out = amd.bev_interpolate(kp[..., :3], bev, *geometry(case))
    assert out.is_contiguous() and out.dtype == torch.float32 and out.shape == (kp.size(0), kp.size(1), bev.size(1))
    if not backward:
        return dict(out=out.detach().cpu())
    out.backward(view(case['grad_out'].to(dev)))
    assert bev.grad.stride() == bev.stride(), 'the gradient comes in the caller\'s layout'
    with torch.no_grad():
        assert torch.equal(amd.bev_interpolate(kp, bev, *geometry(case)), out)       # the forward-only form: the same features
    return dict(out=out.detach().cpu(), grad_bev=bev.grad.cpu().contiguous())


def check_interp_case(got, name, what):
    """the assertions the CPU and the GPU file share"""
    case, r32, r64 = ref.interp_reference(name)
    figures = ref.check_values(got, r32, r64, ref.INTERP_KEYS, f'{what} {name}')
    if case['kind'] in ('outside_far', 'huge'):
        assert not got['out'].any() and not got['grad_bev'].any()
    if case['kind'] in ('cell_centres', 'shared_cell'):      # weights 1 and 0: the cell's value itself, bit for bit
        ix, iy = ref.pixel_coords(case['keypoints'], case['H'], case['W'], case['scale'], case['align'])
        for b in range(ref.B):
            assert torch.equal(got['out'][b], case['bev'][b][:, iy[b].long(), ix[b].long()].t())
    if case['kind'] == 'shared_cell':
        assert torch.equal(got['grad_bev'].double(), r64['grad_bev']), 'small-integer sums are exact in any order'
        for b, (cx, cy) in enumerate(case['cells']):
            untouched = torch.ones_like(got['grad_bev'][b], dtype=torch.bool)
            untouched[:, cy, cx] = False
            assert not got['grad_bev'][b][untouched].any() and got['grad_bev'][b, :, cy, cx].any()
    return figures


@pytest.mark.parametrize('name', sorted(ref.INTERP_CASES))
def test_bev_interpolate_twin_matches_the_restatement(name):
    case = ref.interp_reference(name)[0]
    got = {layout: run_interp(case, layout) for layout in LAYOUTS}
    for layout in LAYOUTS:
        check_interp_case(got[layout], name, f'cpu twin {layout}')
    assert torch.equal(got['nchw']['out'], got['channels_last']['out']), 'the forward is the same bits in both layouts'
    assert torch.equal(got['nchw']['grad_bev'], got['channels_last']['grad_bev'])     # the twin's backward is sequential: so is this
    again = run_interp(case, 'channels_last')
    for k in again:
        assert torch.equal(got['channels_last'][k], again[k]), k


def test_bev_interpolate_misaligned_base_equals_the_aligned_case():
    """C = 64 with the map and the upstream gradient viewed one float into a larger buffer (4-byte aligned pointers only): the same bits"""
    case = ref.interp_reference(ref.MISALIGNED_OF)[0]
    for layout in LAYOUTS:
        shift = (lambda t: ref.offset_view(t.permute(0, 2, 3, 1)).permute(0, 3, 1, 2) if t.dim() == 4 else ref.offset_view(t)) \
            if layout == 'channels_last' else ref.offset_view
        aligned, shifted = run_interp(case, layout), run_interp(case, layout, view=shift)
        for k in aligned:
            assert torch.equal(aligned[k], shifted[k]), (layout, k)


SENTINEL = -77.0


def interp_forward_entry(case, layout, dev='cpu', shift=()):
    """`gd3d_vsa_bev_interp` (or its twin) on a sentinel-filled output with a guard row either side; an operand named in `shift` ('bev',
    'out') starts one float into a larger buffer, every other pointer is 16-byte aligned.  Asserts that every row is written — the zero
    rows too — and no guard is -> out (B, M, C) on the CPU"""
    kp = case['keypoints'].to(dev)
    bev = in_layout(case['bev'].to(dev), layout)
    B, C, H, W = bev.shape
    M = kp.size(1)
    flag = int(layout == 'channels_last')
    dense = bev.permute(0, 2, 3, 1) if flag else bev                 # the map as it lies in memory
    assert dense.is_contiguous()
    dense = ref.offset_view(dense) if 'bev' in shift else dense
    off = 1 if 'out' in shift else 0
    buf = torch.full(((B * M + 2) * C + 8,), SENTINEL, device=dev)
    out = buf[off:off + (B * M + 2) * C].view(B * M + 2, C)
    if C % 4 == 0:
        assert dense.data_ptr() % 16 == (4 if 'bev' in shift else 0) and out[1:].data_ptr() % 16 == 4 * off
    corners = vsa_bev._corners(case['voxel_size'][:2], case['point_cloud_range'][:2], case['point_cloud_range'][3:5], case['scale'], case['align'])
    _host.call('gd3d_vsa_bev_interp', kp.device, (kp.data_ptr(), kp.stride(0), kp.stride(1), dense.data_ptr(), flag, B, M, C, H, W, *corners,
                                                  out[1:].data_ptr()))
    assert (out[0] == SENTINEL).all() and (out[-1] == SENTINEL).all(), 'a guard row was written'
    assert not (out[1:-1] == SENTINEL).any(), 'an output element was left unwritten'
    return out[1:-1].reshape(B, M, C).cpu().contiguous()


def check_sweep_forward(name, dev='cpu'):
    """a forward-only sweep case (vsa_bev_ref.SWEEP_CASES: B * M = 65542 > 16384 workgroups x 4 keypoints): within the bounds against
    fp64, bit-identical to the twin, between the layouts and from run to run; through the C entry every row is written, the zero rows
    included, and nothing past the last"""
    case, r32, r64 = ref.sweep_reference(name)
    layouts = ref.SWEEP_CASES[name][1]
    got = {layout: run_interp(case, layout, dev=dev, backward=False) for layout in layouts}
    figures = {layout: ref.check_values(got[layout], r32, r64, ('out',), f'{dev} {layout} {name}') for layout in layouts}
    first = got[layouts[0]]['out']
    zero_rows = r64['out'].eq(0).all(dim=-1)
    assert bool(zero_rows.any()) and not first[zero_rows].any() and first[~zero_rows].ne(0).any(dim=-1).all()
    twin = first if dev == 'cpu' else run_interp(case, layouts[0], dev='cpu', backward=False)['out']
    for layout in layouts:
        assert torch.equal(got[layout]['out'], twin), f'{layout}: the forward has the bits of the twin, in every layout'
        assert torch.equal(run_interp(case, layout, dev=dev, backward=False)['out'], twin), f'{layout}: run to run'
        assert torch.equal(interp_forward_entry(case, layout, dev), twin), f'{layout}: the C entry'
    return figures


def check_sweep_exact(dev='cpu'):
    """the order-free sweep case, forward and backward, both layouts: the features and the map's gradient EQUAL the exact fp64
    interpolation — a keypoint row skipped or taken twice by the grid-stride loop of interp_backward_kernel changes a sum"""
    case, r32, r64, exact = ref.sweep_exact_reference()
    figures = {}
    for layout in LAYOUTS:
        got = run_interp(case, layout, dev=dev)
        figures[layout] = ref.check_values(got, r32, r64, ref.INTERP_KEYS, f'{dev} {layout} {ref.SWEEP_EXACT}')
        assert torch.equal(got['out'].double(), exact['out']), layout
        assert torch.equal(got['grad_bev'].double(), exact['grad_bev']), f'{layout}: sums of multiples of 2^-8 below 2^16 are exact in any order'
    return figures


def check_interp_single_misaligned_operand(shift, dev='cpu'):
    """channels last, C = 64, ONE of the two pointers the launch reads as float4 one float into a larger buffer: the 4-byte path's
    bits equal the all-aligned run's"""
    case = ref.interp_reference(ref.MISALIGNED_OF)[0]
    assert case['bev'].size(1) == 64 and shift in ('bev', 'out')
    assert torch.equal(interp_forward_entry(case, 'channels_last', dev, shift=(shift,)), interp_forward_entry(case, 'channels_last', dev))


@pytest.mark.parametrize('name', sorted(ref.SWEEP_CASES))
def test_bev_interpolate_sweep_forward(name):
    check_sweep_forward(name)


def test_bev_interpolate_sweep_generators_keep_their_conditions():
    """the spilled rows of the mixed sweeps hold a keypoint inside the map and one out of reach (asserted by the builders, on the fp64
    restatement too); the order-free case keeps fp32 pixel coordinates equal to fp64 and sum |g w| x 256 < 2^24"""
    for name, (C, layouts, _) in ref.SWEEP_CASES.items():
        case = ref.sweep_reference(name)[0]
        R = case['keypoints'].size(0) * case['keypoints'].size(1)
        assert R > ref.SWEEP_CAP * ref.SWEEP_ROWS and case['spilled'].tolist() == list(range(65536, 65542)) and case['bev'].size(1) == C
    case = ref.sweep_exact_reference()[0]
    assert case['keypoints'].size(0) * case['keypoints'].size(1) > ref.SWEEP_CAP * ref.SWEEP_ROWS and case['bev'].size(1) == 64


def test_bev_interpolate_sweep_backward_is_exact():
    check_sweep_exact()


@pytest.mark.parametrize('shift', ['bev', 'out'])
def test_bev_interpolate_single_misaligned_operand_equals_the_aligned_run(shift):
    check_interp_single_misaligned_operand(shift)


def test_other_striding_takes_a_copy_and_keypoint_views_are_read_in_place():
    case, _, _ = ref.interp_reference('m63_c3_5x7_half_s8')
    want = run_interp(case, 'nchw')
    wide = torch.randn(ref.B, 3, 5, 9)
    wide[..., 1:8] = case['bev']
    bev = wide[..., 1:8].requires_grad_(True)                    # neither contiguous nor channels last: one copy inside
    assert not bev.is_contiguous() and not bev.is_contiguous(memory_format=torch.channels_last)
    points = torch.randn(ref.B, 63, 6)
    points[..., :3] = case['keypoints']
    out = amd.bev_interpolate(points[..., :3], bev, *geometry(case))     # the [..., :3] view of wider rows, as it lies
    out.backward(case['grad_out'])
    assert torch.equal(out.detach(), want['out']) and torch.equal(bev.grad, want['grad_bev'])
    xy_only = amd.bev_interpolate(case['keypoints'][..., :2].contiguous(), case['bev'], *geometry(case))
    assert torch.equal(xy_only, want['out'])
    swapped = points.transpose(1, 2).contiguous().transpose(1, 2)         # last dimension not unit-strided: copied
    assert swapped.stride(2) != 1
    assert torch.equal(amd.bev_interpolate(swapped, case['bev'], *geometry(case)), want['out'])


def check_robustness(dev='cpu'):
    """NaN, +-inf and +-1e30 coordinates: zero rows, finite outputs, no gradient from them — and the ordinary rows between them untouched"""
    kp, ordinary = ref.robustness_keypoints()
    kp = kp.to(dev)
    case = ref.interp_reference('m65_c64_5x7_halfmin_s8')[0]
    geo = (ref.VOXEL_SIZE, ref.point_cloud_range(5, 7, 8), 8, 'half')
    for layout in LAYOUTS:
        bev = in_layout(case['bev'].to(dev), layout).clone().requires_grad_(True)
        out = amd.bev_interpolate(kp, bev, *geo)
        assert bool(torch.isfinite(out).all())
        assert not out[~ordinary].any() and out[ordinary].abs().sum(dim=-1).gt(0).all()
        out.backward(torch.ones_like(out))
        assert bool(torch.isfinite(bev.grad).all())
        only = amd.bev_interpolate(kp[ordinary].reshape(ref.B, -1, 3), bev.detach().clone().requires_grad_(True), *geo)
        assert torch.equal(only, out[ordinary].reshape(ref.B, -1, 64))
        alone = bev.detach().clone().requires_grad_(True)                  # the bad rows pass no gradient (the ordinary rows are ONE point repeated: equal addends, any order)
        amd.bev_interpolate(kp[ordinary].reshape(ref.B, -1, 3), alone, *geo).backward(torch.ones_like(only))
        assert torch.equal(alone.grad, bev.grad)


def test_non_finite_and_huge_coordinates_give_zero_rows():
    check_robustness()


def _count_calls(monkeypatch):
    """counts the entry points reached through _host.call from here on -> a function returning their number"""
    seen = []
    real = _host.call

    def counted(name, dev, args, cpu_tail=()):
        seen.append(name)
        return real(name, dev, args, cpu_tail)
    monkeypatch.setattr(_host, 'call', counted)
    return lambda: len(seen)


def test_autograd_wiring(monkeypatch):
    case, _, _ = ref.interp_reference('m65_c64_5x7_halfmin_s8')
    want = run_interp(case, 'nchw')
    n = _count_calls(monkeypatch)
    bev = case['bev'].clone().requires_grad_(True)
    out = amd.bev_interpolate(case['keypoints'], bev, *geometry(case))
    assert out.requires_grad and n() == 1 and len(out.grad_fn.saved_tensors) == 1      # the keypoints; the 144 MB map is not kept
    (g1,) = torch.autograd.grad(out, bev, case['grad_out'], retain_graph=True)        # retain-graph double use
    (g2,) = torch.autograd.grad(out, bev, case['grad_out'])
    assert torch.equal(g1, want['grad_bev']) and torch.equal(g2, g1) and n() == 3
    with torch.no_grad():                                                               # nothing is saved
        quiet = amd.bev_interpolate(case['keypoints'], bev, *geometry(case))
    assert not quiet.requires_grad and quiet.grad_fn is None and torch.equal(quiet, want['out'])
    plain = amd.bev_interpolate(case['keypoints'], case['bev'], *geometry(case))        # nothing requires a gradient
    assert not plain.requires_grad
    kp = case['keypoints'].clone().requires_grad_(True)                                 # requires_grad on the keypoints is not followed
    out = amd.bev_interpolate(kp, bev, *geometry(case))
    out.backward(case['grad_out'])
    assert kp.grad is None and torch.equal(bev.grad, want['grad_bev'])
    only_kp = amd.bev_interpolate(kp, case['bev'], *geometry(case))
    assert not only_kp.requires_grad
    (g,) = torch.autograd.grad(amd.bev_interpolate(case['keypoints'], bev, *geometry(case)).sum(), bev, create_graph=True)
    with pytest.raises(RuntimeError, match='differentiate twice'):
        g.sum().backward()
    # our op is fp32: its gradient is compared with the restatement's (above, per case); finite differences are for the restatement alone
    small = ref.make_interp('m63_c3_5x7_half_s8')
    b64 = small['bev'].double().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda v: ref.interpolate_from_bev_features(small['keypoints'][:, :12].double(), v, *geometry(small)), (b64,))


def test_empty_batches_launch_nothing(monkeypatch):
    n = _count_calls(monkeypatch)
    geo = (ref.VOXEL_SIZE, ref.point_cloud_range(5, 7, 8), 8, 'half')
    bev = torch.randn(2, 3, 5, 7, requires_grad=True)
    out = amd.bev_interpolate(torch.zeros(2, 0, 3), bev, *geo)
    assert out.shape == (2, 0, 3) and out.dtype == torch.float32
    out = amd.bev_interpolate(torch.zeros(0, 4, 3), torch.zeros(0, 3, 5, 7), *geo)
    assert out.shape == (0, 4, 3) and n() == 0


@pytest.mark.parametrize('dtype', [torch.float16, torch.float64])
def test_other_dtypes_are_evaluated_in_fp32_and_cast_back(dtype):
    case = ref.interp_reference('m65_c64_5x7_halfmin_s8')[0]
    for layout in LAYOUTS:
        bev = in_layout(case['bev'], layout).to(dtype).requires_grad_(True)
        bev32 = bev.detach().float().requires_grad_(True)
        kp = case['keypoints'].to(dtype)
        out, out32 = amd.bev_interpolate(kp, bev, *geometry(case)), amd.bev_interpolate(kp.float(), bev32, *geometry(case))
        out.backward(case['grad_out'].to(dtype))
        out32.backward(case['grad_out'].to(dtype).float())
        assert out.dtype == dtype and bev.grad.dtype == dtype and bev.grad.stride() == bev.stride()
        assert torch.equal(out.detach(), out32.detach().to(dtype)) and torch.equal(bev.grad, bev32.grad.to(dtype))


# ---- voxel_centers ---------------------------------------------------------------------------------------------------------------

def check_centres(coors, align, scale, dev='cpu', batch_size=3):
    rng = ref.point_cloud_range(1600, 1408, 1)
    xyz, cnt = amd.voxel_centers(coors.to(dev), ref.VOXEL_SIZE, rng, scale, align, batch_size)
    want = ref.get_voxel_centers(coors, ref.VOXEL_SIZE, rng, scale, align)
    want_cnt = ref.count_loop(coors, want, batch_size)
    assert xyz.dtype == torch.float32 and xyz.shape == (coors.size(0), 3) and cnt.dtype == torch.int32 and cnt.shape == (batch_size,)
    assert torch.equal(xyz.cpu(), want), 'the fp32 statements\' bits'
    assert torch.equal(cnt.cpu(), want_cnt)
    return xyz, cnt


@pytest.mark.parametrize('n', ref.CENTRE_N)
@pytest.mark.parametrize('dtype', [torch.int32, torch.int64])
def test_voxel_centers_twin_equals_the_torch_statements(n, dtype):
    for i, (align, scale) in enumerate(ref.CENTRE_GEOMETRY):
        coors = ref.make_coors(n, 3, 10 * n + i, dtype)
        _, cnt = check_centres(coors, align, scale)
        assert int(cnt[1]) == 0 and int(cnt.sum()) == n - (2 if n >= 65 else 0)        # the empty middle sample; ids -1 and B counted nowhere
    big = torch.tensor([[0, 1 << 20, (1 << 24) + 1, -5]], dtype=dtype)                  # a coordinate past 2^24 rounds as .float() does; a negative one
    check_centres(big, 'half', 8)


def centres_entry(coors, align, scale, batch_size, dev='cpu'):
    """`gd3d_vsa_voxel_centers` (or its twin) on sentinel-filled outputs with a guard either side -> (xyz, cnt) on the CPU, after
    asserting that every centre is written and no guard is"""
    c = coors.to(dev).contiguous()
    N = c.size(0)
    rng = ref.point_cloud_range(1600, 1408, 1)
    size, lo, add = vsa_bev._centre_terms(ref.VOXEL_SIZE, rng[:3], scale, align)
    xyz = torch.full((N + 2, 3), SENTINEL, device=dev)
    cnt = torch.full((batch_size + 2,), -5, dtype=torch.int32, device=dev)
    _host.call('gd3d_vsa_voxel_centers', c.device, (c.data_ptr(), int(c.dtype == torch.int64), N, size, float(scale), lo, add, batch_size,
                                                    xyz[1:].data_ptr(), cnt[1:].data_ptr()))
    assert (xyz[0] == SENTINEL).all() and (xyz[-1] == SENTINEL).all() and not (xyz[1:-1] == SENTINEL).any()
    assert cnt[0] == -5 and cnt[-1] == -5
    return xyz[1:-1].cpu().contiguous(), cnt[1:-1].cpu().contiguous()


def host_bincount(coors, batch_size):
    ids = coors[:, 0].long()
    return torch.bincount(ids[(ids >= 0) & (ids < batch_size)], minlength=batch_size).int()


def check_centre_sweep(dtype, dev='cpu'):
    """N = 4096 x 256 + 65 rows (vsa_bev_ref.CENTRE_SWEEP_N): workgroup 0's second trip holds one full wave and one wave with a single
    row.  Centres: the fp32 torch statements' bits; counts: a host bincount; the guards either side intact"""
    N = ref.CENTRE_SWEEP_N
    assert N > 4096 * 256 and (N - 4096 * 256) % 64 == 1
    coors = ref.make_coors(N, 3, 77 + int(dtype == torch.int64), dtype)          # with the stray ids -1 and 3
    xyz, cnt = centres_entry(coors, 'half', 8, 3, dev)
    assert torch.equal(xyz, ref.get_voxel_centers(coors, ref.VOXEL_SIZE, ref.point_cloud_range(1600, 1408, 1), 8, 'half'))
    assert torch.equal(cnt, host_bincount(coors, 3)) and int(cnt.sum()) == N - 2 and int(cnt[1]) == 0
    return xyz, cnt


def check_centres_many_ids(dtype, dev='cpu'):
    """63, and with the ids moved on by one row 64, distinct counted batch ids in one wave (vsa_bev_ref.make_coors_many_ids): the counts
    are exact -> the counts of both forms"""
    counts = []
    for shift in (0, 1):
        coors = ref.make_coors_many_ids(dtype, shift)
        _, cnt = check_centres(coors, 'halfmin', 2, dev=dev, batch_size=ref.MANY_IDS_B)
        stray = int(((coors[:, 0] < 0) | (coors[:, 0] >= ref.MANY_IDS_B)).sum())
        assert torch.equal(cnt.cpu(), host_bincount(coors, ref.MANY_IDS_B)) and int(cnt.sum()) == 2049 - stray and stray >= 56
        _, cnt2 = centres_entry(coors, 'halfmin', 2, ref.MANY_IDS_B, dev)          # the guards either side of the 70 counts
        assert torch.equal(cnt2, cnt.cpu())
        counts.append(cnt.cpu())
    return torch.stack(counts)


@pytest.mark.parametrize('dtype', [torch.int32, torch.int64])
def test_voxel_centers_sweep(dtype):
    check_centre_sweep(dtype)


@pytest.mark.parametrize('dtype', [torch.int32, torch.int64])
def test_voxel_centers_many_distinct_ids_in_a_wave(dtype):
    check_centres_many_ids(dtype)


def test_voxel_centers_reads_coors_through_a_copy_when_strided():
    coors = ref.make_coors(65, 3, 5, torch.int64)
    wide = torch.zeros(65, 6, dtype=torch.int64)
    wide[:, 1:5] = coors
    xyz, cnt = check_centres(coors, 'half', 8)
    rng = ref.point_cloud_range(1600, 1408, 1)
    xyz2, cnt2 = amd.voxel_centers(wide[:, 1:5], ref.VOXEL_SIZE, rng, 8, 'half', 3)
    assert torch.equal(xyz, xyz2) and torch.equal(cnt, cnt2)


# ---- sample_keypoints ------------------------------------------------------------------------------------------------------------

def reference_sampled_points(points, num_keypoints):
    """the loop of get_sampled_points (:205-244) on the package's own `furthest_point_sample`"""
    out = []
    for p in points:
        src = p[..., :3]
        n = src.shape[0]
        idx = amd.furthest_point_sample(src.unsqueeze(0).contiguous(), num_keypoints).long()[0]
        if n < num_keypoints:
            times = int(num_keypoints / n) + 1
            idx = idx[:n].repeat(times)[:num_keypoints]
        out.append(src[idx])
    return torch.stack(out, dim=0)


def sample_inputs(dev='cpu'):
    g = torch.Generator().manual_seed(77)
    return [(torch.randn(n, 5, generator=g) * 10).to(dev) for n in (300, 37, 130)]      # the middle sample has n < num_keypoints


def check_sample_keypoints(dev='cpu'):
    points = sample_inputs(dev)
    K = 64
    want = reference_sampled_points(points, K)
    got = amd.sample_keypoints(points, K)
    assert got.shape == (3, K, 3) and got.dtype == torch.float32 and torch.equal(got, want)
    assert torch.equal(got[1, 37:], got[1, :27])                                        # the wrap-around
    xyz = torch.cat([p[:, :3] for p in points]).contiguous()
    for cnt_dtype in (torch.int32, torch.int64):
        cnt = torch.tensor([300, 37, 130], dtype=cnt_dtype, device=dev)
        assert torch.equal(amd.sample_keypoints(xyz, cnt, K), want)
    return want


def test_sample_keypoints_equals_the_reference_loop():
    check_sample_keypoints()
    coors = ref.make_coors(2049, 3, 9, stray=False)                                     # the voxel_center_as_source branch
    rng = ref.point_cloud_range(1600, 1408, 1)
    xyz, cnt = amd.voxel_centers(coors, ref.VOXEL_SIZE, rng, 1, 'half', 3)
    got = amd.sample_keypoints(xyz, cnt, 32)
    centres = ref.get_voxel_centers(coors, ref.VOXEL_SIZE, rng, 1, 'half')
    src = [centres[coors[:, 0] == b] for b in (0, 2)]
    want = reference_sampled_points(src, 32)
    assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[1])
    assert torch.equal(got[1], xyz[int(cnt[0])].expand(32, 3))                          # an empty sample: a clamped row, not a fault


# ---- argument checks -------------------------------------------------------------------------------------------------------------

def test_every_argument_check_raises_before_touching_the_library(monkeypatch):
    def no_library(*a, **k):
        raise AssertionError('an argument check must raise before the library is reached')
    monkeypatch.setattr(_host, 'call', no_library)
    monkeypatch.setattr(vsa_bev, 'furthest_point_sample_stacked', no_library)
    kp, bev = torch.zeros(2, 4, 3), torch.zeros(2, 3, 5, 7)
    vs, rng = ref.VOXEL_SIZE, ref.point_cloud_range(5, 7, 8)
    with pytest.raises(RuntimeError, match="'half' or 'halfmin'"):
        amd.bev_interpolate(kp, bev, vs, rng, 8, 'none')
    with pytest.raises(RuntimeError, match="'half' or 'halfmin'"):
        amd.bev_interpolate(kp, bev, vs, rng, 8, None)
    for bad_scale in (0, -1, float('nan'), '8', True):
        with pytest.raises(RuntimeError, match='scale_factor'):
            amd.bev_interpolate(kp, bev, vs, rng, bad_scale)
    with pytest.raises(RuntimeError, match='H, W >= 2'):
        amd.bev_interpolate(kp, torch.zeros(2, 3, 1, 7), vs, rng, 8)
    with pytest.raises(RuntimeError, match='H, W >= 2'):
        amd.bev_interpolate(kp, torch.zeros(2, 3, 5, 1), vs, rng, 8)
    with pytest.raises(RuntimeError, match='C >= 1'):
        amd.bev_interpolate(kp, torch.zeros(2, 0, 5, 7), vs, rng, 8)
    with pytest.raises(RuntimeError, match='must lie beyond'):                   # br <= tl: the reference divides by zero
        amd.bev_interpolate(kp, bev, vs, (0.0, 0.0, 0.0, 2.0, 40.0, 1.0), 8)
    with pytest.raises(RuntimeError, match='must lie beyond'):
        amd.bev_interpolate(kp, bev, vs, (0.0, 0.0, 0.0, 1.0, 1.0, 1.0), 8, 'halfmin')
    with pytest.raises(RuntimeError, match='shape mismatch'):
        amd.bev_interpolate(kp[..., :1], bev, vs, rng, 8)
    with pytest.raises(RuntimeError, match='shape mismatch'):
        amd.bev_interpolate(kp[0], bev, vs, rng, 8)
    with pytest.raises(RuntimeError, match='shape mismatch'):
        amd.bev_interpolate(kp[:1], bev, vs, rng, 8)
    with pytest.raises(RuntimeError, match='shape mismatch'):
        amd.bev_interpolate(kp, bev[0], vs, rng, 8)
    with pytest.raises(RuntimeError, match='shape mismatch'):
        amd.bev_interpolate(kp.long(), bev, vs, rng, 8)
    with pytest.raises(RuntimeError, match='shape mismatch'):
        amd.bev_interpolate(kp, bev.long(), vs, rng, 8)
    with pytest.raises(RuntimeError, match='is on'):
        amd.bev_interpolate(kp, bev.to('meta'), vs, rng, 8)
    with pytest.raises(RuntimeError, match='must hold 3'):
        amd.bev_interpolate(kp, bev, vs[:2], rng, 8)
    with pytest.raises(RuntimeError, match='must hold 6'):
        amd.bev_interpolate(kp, bev, vs, rng[:3], 8)
    coors = torch.zeros(4, 4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="'half' or 'halfmin'"):
        amd.voxel_centers(coors, vs, rng, 1, 'none', 2)
    with pytest.raises(RuntimeError, match='scale_factor'):
        amd.voxel_centers(coors, vs, rng, 0, 'half', 2)
    with pytest.raises(RuntimeError, match='shape mismatch'):
        amd.voxel_centers(coors[:, :3], vs, rng, 1, 'half', 2)
    with pytest.raises(RuntimeError, match='int32 or int64'):
        amd.voxel_centers(coors.float(), vs, rng, 1, 'half', 2)
    with pytest.raises(RuntimeError, match='int32 or int64'):
        amd.voxel_centers(coors.to(torch.int16), vs, rng, 1, 'half', 2)
    with pytest.raises(RuntimeError, match='batch_size'):
        amd.voxel_centers(coors, vs, rng, 1, 'half', -1)
    xyz = torch.zeros(5, 3)
    with pytest.raises(RuntimeError, match='sample_keypoints takes'):
        amd.sample_keypoints(xyz)
    with pytest.raises(RuntimeError, match='non-empty list'):
        amd.sample_keypoints([], 4)
    with pytest.raises(RuntimeError, match='shape mismatch'):
        amd.sample_keypoints([torch.zeros(5, 2)], 4)
    with pytest.raises(RuntimeError, match='shape mismatch'):
        amd.sample_keypoints(torch.zeros(5, 4), torch.tensor([5]), 4)
    with pytest.raises(RuntimeError, match='integer tensor'):
        amd.sample_keypoints(xyz, torch.tensor([5.0]), 4)
    with pytest.raises(RuntimeError, match='num_keypoints'):
        amd.sample_keypoints(xyz, torch.tensor([5]), -1)
    with pytest.raises(RuntimeError, match='no points'):
        amd.sample_keypoints(torch.zeros(0, 3), torch.tensor([0]), 4)
    for name in ('bev_interpolate', 'voxel_centers', 'sample_keypoints'):
        assert name in amd.__all__


def test_host_twins_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """csrc/vsa_bev_cpu.cpp compiled together with a stand-alone driver (tests/hostmath/vsa_bev_sanitize.cpp, its own main) under
    -fsanitize=address,undefined and run as a program on the CPU: exactly sized heap buffers, NaN, +-inf and +-1e30 coordinates, `coors`
    with out-of-range batch ids.  The device kernels share that index code.  A sanitizer build belongs on a CPU-only machine: with a GPU
    present the test skips before it compiles or starts anything."""
    if torch.cuda.is_available():
        pytest.skip('sanitizer builds run on a CPU-only machine, never where a GPU is present')
    import os
    import subprocess
    from mmdet3d_gaussian_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = _lib._build.host_cxx_path()
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'vsa_bev_sanitize')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined,float-cast-overflow', '-fno-sanitize-recover=all', '-ffp-contract=off',
           os.path.join(root, 'tests', 'hostmath', 'vsa_bev_sanitize.cpp'),
           os.path.join(root, 'mmdet3d-gaussian_amd', 'csrc', 'vsa_bev_cpu.cpp'), '-o', exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.rstrip().endswith('OK') and 'runtime error' not in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
