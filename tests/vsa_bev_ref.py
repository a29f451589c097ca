"""tests/vsa_bev_ref.py — TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Torch restatement, statement by statement, of three passages of the reference's VoxelSetAbstraction
(models/middle_encoders/voxel_set_abstraction.py):
  interpolate_from_bev_features     :153-177   (it calls F.grid_sample itself)
  get_voxel_centers                 :179-193
  the per-sample count loop         :303-305
Runs in whatever dtype its inputs have (fp32: the operation sequence a user runs at the parent commit; fp64: the yardstick); autograd
gives the gradient of the map.  Also the named cases of tests/test_cpu_vsa_bev.py and tests/test_gpu_vsa_bev.py — every builder asserts
its own preconditions — and one cached evaluation per case that both files share (never modify the tensors).  The bound is the
project's rule, taken from tests/pvrcnn_seg_ref.py."""
import functools

import torch
import torch.nn.functional as F

from pvrcnn_seg_ref import NOISE_FACTOR, ULP, bound, check_values, offset_view  # noqa: F401  (re-exported for the two test files)

VOXEL_SIZE = (0.25, 0.5, 0.125)          # exactly representable: the cell centres of every case are exact in fp32
RANGE_MIN = (-3.0, 2.0, -1.0)
B = 2                                     # two samples: the second one's offsets
ALIGNMENTS = ('half', 'halfmin')


# ---- the restatement -------------------------------------------------------------------------------------------------------------

def interpolate_from_bev_features(keypoints, bev_features, voxel_size, point_cloud_range, scale_factor, voxel_center_align):
    """:153-177"""
    voxel_size_xy = keypoints.new_tensor(voxel_size[:2])
    tl = keypoints.new_tensor(point_cloud_range[:2])
    br = keypoints.new_tensor(point_cloud_range[3:5])
    if voxel_center_align == 'half':
        tl.add_(0.5 * voxel_size_xy * scale_factor)
        br.sub_(0.5 * voxel_size_xy * scale_factor)
    elif voxel_center_align == 'halfmin':
        tl.add_(0.5 * voxel_size_xy)
        br.sub_(voxel_size_xy * (scale_factor - 0.5))
    xy = keypoints[..., :2]
    grid = (xy - tl[None, None, :]) / ((br - tl)[None, None, :])
    grid = (grid * 2 - 1).unsqueeze(1)
    sampled = F.grid_sample(bev_features, grid=grid, align_corners=True)
    return sampled.squeeze(2).permute(0, 2, 1).contiguous()


def get_voxel_centers(coors, voxel_size, point_cloud_range, scale_factor, voxel_center_align):
    """:179-193, fp32 as the reference runs it"""
    assert coors.shape[1] == 4
    centers = coors[:, [3, 2, 1]].float()
    size = centers.new_tensor(voxel_size)
    range_min = centers.new_tensor(point_cloud_range[:3])
    centers = centers * size * scale_factor + range_min
    if voxel_center_align == 'half':
        centers.add_(0.5 * size * scale_factor)
    elif voxel_center_align == 'halfmin':
        centers.add_(0.5 * size)
    else:
        raise NotImplementedError
    return centers


def count_loop(coors, xyz, batch_size):
    """:303-305"""
    xyz_batch_cnt = xyz.new_zeros(batch_size).int()
    for bs_idx in range(batch_size):
        xyz_batch_cnt[bs_idx] = (coors[:, 0] == bs_idx).sum()
    return xyz_batch_cnt


# ---- the geometry of a case ------------------------------------------------------------------------------------------------------

def point_cloud_range(H, W, scale):
    """the range whose BEV map at stride `scale` has exactly (H, W) cells"""
    lo = RANGE_MIN
    return (lo[0], lo[1], lo[2], lo[0] + W * VOXEL_SIZE[0] * scale, lo[1] + H * VOXEL_SIZE[1] * scale, lo[2] + 4.0)


def cell_grid(H, W, scale, align):
    """(first centre, step) per axis (x, y) in exact arithmetic: both alignments put cell i's centre at first + i * step"""
    step = (VOXEL_SIZE[0] * scale, VOXEL_SIZE[1] * scale)
    first = tuple(RANGE_MIN[a] + 0.5 * (step[a] if align == 'half' else VOXEL_SIZE[a]) for a in (0, 1))
    return first, step


def pixel_coords(keypoints, H, W, scale, align):
    """fp64 pixel coordinates (ix, iy) of every keypoint: what the builders assert their placements with"""
    first, step = cell_grid(H, W, scale, align)
    k = keypoints.double()
    return (k[..., 0] - first[0]) / step[0], (k[..., 1] - first[1]) / step[1]


PLACEMENTS = ('inside', 'cell_centres', 'last_row_col', 'outside_partial', 'outside_far', 'huge')


def _place(kind, m, H, W, scale, align, g):
    """m keypoints (m, 2) of one placement kind, with its preconditions asserted on the fp64 pixel coordinates"""
    first, step = cell_grid(H, W, scale, align)
    n = (W, H)
    u = torch.rand(m, 2, generator=g, dtype=torch.float64)
    pix = torch.empty(m, 2, dtype=torch.float64)
    if kind == 'inside':                       # strictly inside the centre box
        for a in (0, 1):
            pix[:, a] = (0.01 + 0.98 * u[:, a]) * (n[a] - 1)
    elif kind == 'cell_centres':               # integers: the weights are 1 and 0
        for a in (0, 1):
            pix[:, a] = torch.randint(0, n[a], (m,), generator=g).double()
    elif kind == 'last_row_col':               # the +1 neighbour is out of range with weight 0
        for a in (0, 1):
            pix[:, a] = (0.01 + 0.98 * u[:, a]) * (n[a] - 1)
        pix[0::2, 0] = n[0] - 1
        pix[1::2, 1] = n[1] - 1
        pix[0, :] = torch.tensor([n[0] - 1, n[1] - 1], dtype=torch.float64)
    elif kind == 'outside_partial':            # outside by less than one cell on one axis (both on every fourth): partial padding
        for a in (0, 1):
            pix[:, a] = (0.01 + 0.98 * u[:, a]) * (n[a] - 1)
        d = 0.05 + 0.9 * torch.rand(m, generator=g, dtype=torch.float64)
        idx = torch.arange(m)
        pix[idx % 4 == 0, 0] = -d[idx % 4 == 0]
        pix[idx % 4 == 1, 0] = (n[0] - 1) + d[idx % 4 == 1]
        pix[idx % 4 == 2, 1] = -d[idx % 4 == 2]
        pix[idx % 4 == 3, 1] = (n[1] - 1) + d[idx % 4 == 3]
        pix[idx % 8 == 3, 0] = -d[idx % 8 == 3]
    elif kind == 'outside_far':                # outside by more than one cell: every value is zero
        for a in (0, 1):
            pix[:, a] = (0.01 + 0.98 * u[:, a]) * (n[a] - 1)
        d = 1.1 + 3.0 * torch.rand(m, generator=g, dtype=torch.float64)
        idx = torch.arange(m)
        pix[idx % 4 == 0, 0] = -d[idx % 4 == 0]
        pix[idx % 4 == 1, 0] = (n[0] - 1) + d[idx % 4 == 1]
        pix[idx % 4 == 2, 1] = -d[idx % 4 == 2]
        pix[idx % 4 == 3, 1] = (n[1] - 1) + d[idx % 4 == 3]
    elif kind == 'huge':
        xy = torch.tensor([[1e6, 0.0], [-1e6, 0.0], [0.0, 1e6], [0.0, -1e6], [1e6, -1e6]])[torch.arange(m) % 5]
        return xy
    else:
        raise KeyError(kind)
    xy = torch.stack([first[0] + pix[:, 0] * step[0], first[1] + pix[:, 1] * step[1]], dim=1).float()
    ix, iy = pixel_coords(xy, H, W, scale, align)        # of the fp32 keypoints, as every implementation receives them
    if kind in ('inside', 'last_row_col'):
        assert bool(((ix >= 0) & (ix <= W - 1) & (iy >= 0) & (iy <= H - 1)).all())
    if kind == 'cell_centres':
        assert torch.equal(ix, ix.round()) and torch.equal(iy, iy.round())
    if kind == 'last_row_col':
        assert bool(((ix == W - 1) | (iy == H - 1)).all()) and ix[0] == W - 1 and iy[0] == H - 1
    if kind == 'outside_partial':
        out_x, out_y = (ix < 0) | (ix > W - 1), (iy < 0) | (iy > H - 1)
        assert bool((out_x | out_y).all()) and bool(((ix > -1) & (ix < W) & (iy > -1) & (iy < H)).all())
        assert bool((out_x & out_y).any()) or m < 4
    if kind == 'outside_far':
        assert bool(((ix < -1) | (ix > W) | (iy < -1) | (iy > H)).all())
    return xy


def _interp_case(H, W, M, C, align, scale, kind, seed, with_grad=True):
    g = torch.Generator().manual_seed(seed)
    kinds = PLACEMENTS if kind == 'mixed' else (kind,)
    if kind == 'mixed':
        assert M >= len(PLACEMENTS)
    kp = torch.empty(B, M, 3)
    kp[..., 2] = torch.rand(B, M, generator=g) * 4 - 1
    for b in range(B):
        for j, k in enumerate(kinds):            # every kind in every sample, interleaved
            rows = torch.arange(j, M, len(kinds))
            kp[b, rows, :2] = _place(k, rows.numel(), H, W, scale, align, g)
    bev = torch.randn(B, C, H, W, generator=g)
    grad_out = torch.randn(B, M, C, generator=g) if with_grad else None      # the last draw: leaving it out moves nothing
    assert kp.shape == (B, M, 3) and bool(torch.isfinite(kp).all())
    return dict(keypoints=kp, bev=bev, grad_out=grad_out, voxel_size=VOXEL_SIZE, point_cloud_range=point_cloud_range(H, W, scale),
                scale=scale, align=align, H=H, W=W, kind=kind)


def _shared_cell_case(seed):
    """the integer-exact backward: all M = 130 keypoints of a sample sit on ONE cell centre whose pixel coordinates are exact in every
    fp32 evaluation order (x index 3 of 7: 3 / 6 = 0.5), the upstream gradient is small integers: the sums are exact in any order"""
    H, W, M, C, scale, align = 5, 7, 130, 65, 8, 'half'
    g = torch.Generator().manual_seed(seed)
    first, step = cell_grid(H, W, scale, align)
    kp = torch.zeros(B, M, 3)
    for b, (cx, cy) in enumerate(((3, 2), (6, 4))):
        kp[b, :, 0], kp[b, :, 1] = first[0] + cx * step[0], first[1] + cy * step[1]
    ix, iy = pixel_coords(kp, H, W, scale, align)
    assert torch.equal(ix[0], torch.full((M,), 3.0, dtype=torch.float64)) and torch.equal(iy[1], torch.full((M,), 4.0, dtype=torch.float64))
    grad_out = torch.randint(-8, 9, (B, M, C), generator=g).float()
    bev = torch.randint(-8, 9, (B, C, H, W), generator=g).float()
    return dict(keypoints=kp, bev=bev, grad_out=grad_out, voxel_size=VOXEL_SIZE, point_cloud_range=point_cloud_range(H, W, scale),
                scale=scale, align=align, H=H, W=W, kind='shared_cell', cells=((3, 2), (6, 4)))


INTERP_CASES = {
    # name: (H, W, M, C, alignment, scale, placement) — M over 1, 63, 65, 130; C over the lane-group tails (1, 3, 65), the 16-byte
    # path (64, 256) and its tail (260); both alignments with both scales; both map sizes
    'm1_c1_2x2_half_s8': (2, 2, 1, 1, 'half', 8, 'inside'),
    'm63_c3_5x7_half_s8': (5, 7, 63, 3, 'half', 8, 'mixed'),
    'm65_c64_5x7_halfmin_s8': (5, 7, 65, 64, 'halfmin', 8, 'mixed'),
    'm130_c65_5x7_half_s2': (5, 7, 130, 65, 'half', 2, 'mixed'),
    'm65_c256_5x7_half_s8': (5, 7, 65, 256, 'half', 8, 'mixed'),
    'm63_c260_2x2_halfmin_s2': (2, 2, 63, 260, 'halfmin', 2, 'mixed'),
    'm130_c260_5x7_halfmin_s8': (5, 7, 130, 260, 'halfmin', 8, 'mixed'),
    'm65_c64_2x2_half_s2': (2, 2, 65, 64, 'half', 2, 'mixed'),
    'shared_cell': None,
}
for _kind in PLACEMENTS:                             # one placement alone, on the 16-byte path and on the scalar one
    INTERP_CASES[f'{_kind}_c64'] = (5, 7, 65, 64, 'half', 8, _kind)
    INTERP_CASES[f'{_kind}_c3'] = (5, 7, 65, 3, 'halfmin', 2, _kind)
MISALIGNED_OF = 'm65_c64_5x7_halfmin_s8'             # `offset_view`: this case's map and upstream gradient one float into a larger buffer
INTERP_KEYS = ('out', 'grad_bev')


def make_interp(name):
    seed = 3000 + sorted(INTERP_CASES).index(name)
    return _shared_cell_case(seed) if name == 'shared_cell' else _interp_case(*INTERP_CASES[name], seed)


def evaluate_interp(case, dtype):
    bev = case['bev'].to(dtype).clone().requires_grad_(True)
    out = interpolate_from_bev_features(case['keypoints'].to(dtype), bev, case['voxel_size'], case['point_cloud_range'], case['scale'], case['align'])
    out.backward(case['grad_out'].to(dtype))
    return dict(out=out.detach(), grad_bev=bev.grad)


@functools.lru_cache(maxsize=None)
def interp_reference(name):
    """(case, fp32 restatement, fp64 restatement), computed once and shared"""
    case = make_interp(name)
    r32, r64 = evaluate_interp(case, torch.float32), evaluate_interp(case, torch.float64)
    if case['kind'] in ('outside_far', 'huge'):
        assert not r64['out'].any() and not r64['grad_bev'].any()
    return case, r32, r64


# ---- the second sweep of the interpolation kernels ---------------------------------------------------------------------------------
# row_grid caps a launch at 16384 workgroups; a workgroup of 256 threads holds 256 / L keypoints, L = row_lanes(items) lanes each.
#   interp_kernel<false>, NCHW, C = 64:          L = row_lanes(64 channels) = 64 -> 4 keypoints per workgroup
#   interp_kernel<true>, channels last, C = 256:  L = row_lanes(256 / 4 = 64 quads) = 64 -> 4 keypoints per workgroup
#   interp_backward_kernel, C = 64, both layouts: L = row_lanes(64) = 64 -> 4 keypoints per workgroup
# so one sweep covers 16384 * 4 = 65536 keypoints, and B * M = 2 * 32771 = 65542 leaves 6 to the second trip: workgroup 0 takes four,
# workgroup 1 two.  (Channels last at C = 64 has L = row_lanes(16 quads) = 16, 16 keypoints per workgroup: one trip.)  These are the
# smallest shapes that get there; the map stays 5 x 7.
SWEEP_M = 32771
SWEEP_CAP, SWEEP_ROWS = 16384, 4
SWEEP_SPILL = B * SWEEP_M - SWEEP_CAP * SWEEP_ROWS
assert SWEEP_SPILL == 6
SWEEP_CASES = {
    # name: (C, layouts the forward is checked in, seed) — `mixed` placement, forward only: M keypoints around 35 cells make the
    # backward's sums long enough for the order of the float atomics to show; the order-free case below is the backward's
    'sweep_m32771_c64': (64, ('nchw', 'channels_last'), 3501),
    'sweep_m32771_c256': (256, ('channels_last',), 3502),
}
SWEEP_EXACT = 'sweep_m32771_c64_sixteenths'


def make_sweep(name):
    C, _, seed = SWEEP_CASES[name]
    case = _interp_case(5, 7, SWEEP_M, C, 'half', 8, 'mixed', seed, with_grad=False)
    spilled = torch.arange(SWEEP_CAP * SWEEP_ROWS, B * SWEEP_M)                  # the flat keypoint rows of the second trip
    ix, iy = pixel_coords(case['keypoints'].reshape(-1, 3)[spilled], 5, 7, 8, 'half')
    inside = (ix >= 0) & (ix <= 6) & (iy >= 0) & (iy <= 4)
    far = (ix < -1) | (ix > 7) | (iy < -1) | (iy > 5)
    assert bool(inside.any()) and bool(far.any()), 'the spilled rows hold a keypoint inside the map and one out of its reach'
    case['spilled'] = spilled
    return case


@functools.lru_cache(maxsize=None)
def sweep_reference(name):
    """(case, fp32 restatement, fp64 restatement) of a forward-only sweep case: `out` alone"""
    case = make_sweep(name)
    with torch.no_grad():
        r32, r64 = ({'out': interpolate_from_bev_features(case['keypoints'].to(d), case['bev'].to(d), case['voxel_size'], case['point_cloud_range'],
                                                          case['scale'], case['align'])} for d in (torch.float32, torch.float64))
    rows = r64['out'].reshape(-1, r64['out'].size(-1))[case['spilled']]
    assert bool(rows.eq(0).all(dim=1).any()) and bool(rows.ne(0).any(dim=1).any()), 'a zero row and a non-zero row among the spilled'
    return case, r32, r64


def kernel_pixel_coords(case):
    """the fp32 pixel coordinates as csrc/vsa_bev_common.h takes them: ((v - tl) * (n - 1)) / (br - tl), tl and br from the reference's
    fp32 statements :157-166"""
    vs = torch.tensor(case['voxel_size'][:2], dtype=torch.float32)
    tl = torch.tensor(case['point_cloud_range'][:2], dtype=torch.float32)
    br = torch.tensor(case['point_cloud_range'][3:5], dtype=torch.float32)
    if case['align'] == 'half':
        tl.add_(0.5 * vs * case['scale'])
        br.sub_(0.5 * vs * case['scale'])
    else:
        tl.add_(0.5 * vs)
        br.sub_(vs * (case['scale'] - 0.5))
    k = case['keypoints']
    assert k.dtype == torch.float32
    n = (case['W'], case['H'])
    return tuple(((k[..., a] - tl[a]) * float(n[a] - 1)) / (br[a] - tl[a]) for a in (0, 1))


def exact_interp(case, absolute=False):
    """bilinear interpolation and its map gradient written out in fp64 on the EXACT pixel coordinates of `pixel_coords` (the kernel's rule
    for reach and padding: within (-1, n), neighbours outside the map contribute nothing) -> dict(out, grad_bev).  `absolute`: the
    sums of |g * w| instead, the magnitude every partial sum of grad_bev stays below"""
    H, W = case['H'], case['W']
    ix, iy = pixel_coords(case['keypoints'], H, W, case['scale'], case['align'])
    bev, g = case['bev'].double(), case['grad_out'].double()
    Bn, C = bev.shape[:2]
    out, grad = torch.zeros(Bn, ix.size(1), C, dtype=torch.float64), torch.zeros(Bn, H * W, C, dtype=torch.float64)
    flat = bev.permute(0, 2, 3, 1).reshape(Bn, H * W, C)
    reach = (ix > -1) & (ix < W) & (iy > -1) & (iy < H)
    x0, y0 = ix.floor(), iy.floor()
    ax, ay = ix - x0, iy - y0
    for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
        xj, yj = x0.long() + dx, y0.long() + dy
        w = (ax if dx else 1 - ax) * (ay if dy else 1 - ay)
        use = reach & (xj >= 0) & (xj < W) & (yj >= 0) & (yj < H)
        w = torch.where(use, w, torch.zeros_like(w))
        cell = torch.where(use, yj * W + xj, torch.zeros_like(xj))
        for b in range(Bn):
            out[b] += flat[b][cell[b]] * w[b][:, None]
            gw = g[b] * w[b][:, None]
            grad[b].index_add_(0, cell[b], gw.abs() if absolute else gw)
    return dict(out=out, grad_bev=grad.reshape(Bn, H, W, C).permute(0, 3, 1, 2).contiguous())


def make_sweep_exact():
    """the sweep's backward, order-free (as `shared_cell` and the graph test are): B * M = 65542 keypoints on sixteenths of a cell of the
    5 x 7 map — within a cell of it on every side, so partial padding is there too — small-integer upstream gradients and map values.
    Every weight is a multiple of 2^-8 and every product g * w too; the builder asserts the two conditions under which every partial
    sum of the gradient, taken in any order, is exact in fp32."""
    H, W, M, C, scale, align = 5, 7, SWEEP_M, 64, 8, 'half'
    g = torch.Generator().manual_seed(3503)
    first, step = cell_grid(H, W, scale, align)
    sx = torch.randint(-15, 16 * (W - 1) + 16, (B, M), generator=g)              # sixteenths: pixel coordinates in (-1, n - 1 + 15/16]
    sy = torch.randint(-15, 16 * (H - 1) + 16, (B, M), generator=g)
    kp = torch.zeros(B, M, 3)
    kp[..., 0] = (first[0] + sx.double() / 16 * step[0]).float()
    kp[..., 1] = (first[1] + sy.double() / 16 * step[1]).float()
    case = dict(keypoints=kp, bev=torch.randint(-8, 9, (B, C, H, W), generator=g).float(), grad_out=torch.randint(-8, 9, (B, M, C), generator=g).float(),
                voxel_size=VOXEL_SIZE, point_cloud_range=point_cloud_range(H, W, scale), scale=scale, align=align, H=H, W=W, kind='sixteenths')
    ix, iy = pixel_coords(kp, H, W, scale, align)
    assert torch.equal(ix * 16, sx.double()) and torch.equal(iy * 16, sy.double())                     # the keypoints ARE the sixteenths drawn
    kx, ky = kernel_pixel_coords(case)
    assert torch.equal(kx.double(), ix) and torch.equal(ky.double(), iy), 'condition 1: the fp32 and the fp64 pixel coordinates coincide'
    assert bool((ix < 0).any()) and bool((ix > W - 1).any()) and bool((iy < 0).any()) and bool((iy > H - 1).any())
    return case


@functools.lru_cache(maxsize=None)
def sweep_exact_reference():
    """(case, fp32 restatement, fp64 restatement, exact fp64 interpolation) of the order-free sweep case"""
    case = make_sweep_exact()
    exact = exact_interp(case)
    bound_sum = float(exact_interp(case, absolute=True)['grad_bev'].max())
    assert bound_sum * 256 < 2 ** 24, f'condition 2: sum |g * w| * 256 = {bound_sum * 256} must stay below 2^24'
    assert torch.equal(exact['grad_bev'] * 256, (exact['grad_bev'] * 256).round()) and torch.equal(exact['out'] * 256, (exact['out'] * 256).round())
    r32, r64 = evaluate_interp(case, torch.float32), evaluate_interp(case, torch.float64)
    for k in INTERP_KEYS:      # the exact form IS the restatement: grid_sample in fp64 differs from it by its own rounding of the grid only
        assert float((r64[k] - exact[k]).abs().max()) <= 1e-9 * max(1.0, float(exact[k].abs().max())), k
    return case, r32, r64, exact


def robustness_keypoints():
    """(B, M, 3) keypoints whose xy are NaN, +-inf, +-1e30 — the rows that must come out as zeros — interleaved with ordinary ones"""
    bad = [float('nan'), float('inf'), float('-inf'), 1e30, -1e30]
    rows = []
    for v in bad:
        rows += [[v, 3.0], [-2.0, v], [v, v], [-2.0, 3.0]]
    rows += [[float('nan'), float('inf')], [float('inf'), -1e30]]
    kp = torch.tensor(rows, dtype=torch.float32)
    kp = torch.cat([kp, torch.zeros(len(rows), 1)], dim=1)
    ordinary = torch.tensor([r[0] == -2.0 and r[1] == 3.0 for r in rows])
    assert int(ordinary.sum()) == len(bad)
    return torch.stack([kp, kp.flip(0)]), torch.stack([ordinary, ordinary.flip(0)])


# ---- the voxel-centre cases ------------------------------------------------------------------------------------------------------

CENTRE_N = (0, 1, 65, 2049)
CENTRE_GEOMETRY = (('half', 1), ('half', 8), ('halfmin', 2), ('halfmin', 8), ('half', 1.5))


# voxel_centers_kernel: the grid is capped at 4096 workgroups of 256 rows, so one sweep covers 4096 * 256 = 1 048 576 rows and
# N = 1 048 641 leaves 65 to the second trip of workgroup 0: one full wave and one wave with a single row, whose other 63 lanes still
# have to reach the ballots.  The smallest N that gets there with a partly filled wave.
CENTRE_SWEEP_N = 4096 * 256 + 65
MANY_IDS_B = 70


def make_coors_many_ids(dtype=torch.int32, shift=0):
    """(2049, 4) rows whose batch id is (row + shift) % 72 - 1: -1 .. 70 with B = 70, so -1 and 70 are counted nowhere and a wave of 64
    consecutive rows holds 62 or 63 DISTINCT counted ids (a wave starts on a multiple of 8 of the cycle, so it always meets -1 or 70)
    — with shift = 1 the first wave holds ids 0 .. 63: the kernel's ballot loop, once per distinct id, runs its full 64 times"""
    c = make_coors(2049, 3, 4242, torch.int64, stray=False)
    c[:, 0] = (torch.arange(2049) + shift) % (MANY_IDS_B + 2) - 1
    per_wave = [len(set(v for v in c[w:w + 64, 0].tolist() if 0 <= v < MANY_IDS_B)) for w in range(0, 2048, 64)]
    assert max(per_wave) == (64 if shift == 1 else 63) and min(per_wave) >= 62
    assert int((c[:, 0] == -1).sum()) > 0 and int((c[:, 0] == MANY_IDS_B).sum()) > 0
    return c.to(dtype)


def make_coors(n, batch_size, seed, dtype=torch.int32, stray=True):
    """(n, 4) [b, z, y, x] grouped by sample, B = 3 with an EMPTY middle sample; from 65 rows on one row carries batch id -1 and one
    batch id `batch_size` (counted for no sample)"""
    assert batch_size == 3
    g = torch.Generator().manual_seed(seed)
    c = torch.stack([torch.zeros(n, dtype=torch.int64), torch.randint(0, 41, (n,), generator=g), torch.randint(0, 1600, (n,), generator=g),
                     torch.randint(0, 1408, (n,), generator=g)], dim=1)
    c[n // 3:, 0] = 2
    if stray and n >= 65:
        c[7, 0], c[n - 2, 0] = -1, batch_size
        assert (c[:, 0] == -1).sum() == 1 and (c[:, 0] == batch_size).sum() == 1
    if n >= 65:
        assert (c[:, 0] == 0).any() and not (c[:, 0] == 1).any() and (c[:, 0] == 2).any()
    return c.to(dtype)
