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


def _interp_case(H, W, M, C, align, scale, kind, seed):
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
    grad_out = torch.randn(B, M, C, generator=g)
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
