"""tests/view_net_ref.py — TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Torch restatements, statement by statement, of the multi-view pillar encoder's view passages of the reference:
  to_cylindrical / to_spherical / voxelize_view      models/detectors/pillar_od.py:29-70
  SingleViewNet.forward, the grid and the loop         models/voxel_encoders/pillar_mvf_encoder.py:88-105
  mmdet3d's PointPillarsScatter                        restated from its published text (mmdet3d is absent — PARITY UNPINNED)
They run in whatever dtype their inputs have (fp32: what a user runs at the parent commit; fp64: the yardstick).  Also a numpy
restatement of the library's FIXED fp32 sequences (include/gd3d.h) — every step one np.float32 operation — and the named cases of
tests/test_cpu_view_net.py and tests/test_gpu_view_net.py.  Every builder asserts its own preconditions; evaluations are cached and
shared by both files (never modify the tensors)."""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

from pvrcnn_seg_ref import bound, check_values, offset_view  # noqa: F401  (re-exported to the test files)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'view_net.npz')
# the shipped config's views (configs/_base_/models/pillarmvf_*_kitti.py) plus a spherical one of the same angular cell
GEOMETRY = {'cartesian': ((0.16, 0.16, 4.0), (0.0, -39.68, -3.0, 69.12, 39.68, 1.0)),
            'cylindrical': ((0.0025, 0.04, 100.0), (-1.58, -3.0, 0.0, 1.58, 1.0, 100.0)),
            'spherical': ((0.0025, 0.005, 100.0), (-1.58, -0.5, 0.0, 1.58, 0.5, 100.0))}
VIEW_SETS = (('cylindrical',), ('cartesian', 'cylindrical'), ('cartesian', 'cylindrical', 'spherical'))
TRANSFORM_N = (0, 1, 63, 64, 65, 2049)
TRANSFORM_C = (3, 4, 5)


# ---- the reference's statements ----------------------------------------------------------------------------------------------------

def to_cartesian(points):
    return points


def to_cylindrical(points):
    z = points[:, 2]
    phi = torch.atan2(points[:, 1], points[:, 0])
    rho = points[:, :2].norm(p=2, dim=-1)
    cylinder = torch.stack((phi, z, rho), dim=-1)
    return torch.cat((cylinder, points[:, 3:]), dim=-1)


def to_spherical(points):
    yaw = torch.atan2(points[:, 1], points[:, 0])
    rho = points[:, :3].norm(p=2, dim=-1)
    pitch = torch.asin(points[:, 2] / rho)
    sphere = torch.stack((yaw, pitch, rho), dim=-1)
    return torch.cat((sphere, points[:, 3:]), dim=-1)


def dynamic_voxelizer(voxel_size, point_cloud_range):
    """mmdet3d's dynamic `Voxelization(max_num_points=-1)` of ONE sample, restated: floor((p - lo) / vs) in the points' dtype -> (n, 3)
    int32 [z, y, x], a row of -1 outside the grid"""
    grid = torch.round((torch.tensor(point_cloud_range[3:], dtype=torch.float32) - torch.tensor(point_cloud_range[:3], dtype=torch.float32))
                       / torch.tensor(voxel_size, dtype=torch.float32))
    constants = {}          # per (device, dtype): the op itself takes these as launch arguments, so they are not copied per call here

    def run(res):
        key = (res.device, res.dtype)
        if key not in constants:
            constants[key] = (res.new_tensor(point_cloud_range[:3]), res.new_tensor(voxel_size), grid.to(res))
        lo, vs, g = constants[key]
        cell = torch.floor((res[:, :3] - lo) / vs)
        inside = ((cell >= 0) & (cell < g)).all(dim=-1)
        zyx = cell.flip(-1).to(torch.int32)
        return torch.where(inside.unsqueeze(-1), zyx, torch.full_like(zyx, -1))
    return run


def voxelize_view(view, voxelizer, points):
    """pillar_od.py:57-70"""
    points = [globals()[f'to_{view}'](res) for res in points]
    coors = []
    for res in points:
        res_coors = voxelizer(res)
        coors.append(res_coors)
    points = torch.cat(points, dim=0)
    coors_batch = []
    for i, coor in enumerate(coors):
        coor_pad = F.pad(coor, (1, 0), mode='constant', value=i)
        coors_batch.append(coor_pad)
    coors_batch = torch.cat(coors_batch, dim=0)
    return points, coors_batch


def pillars_scatter(voxel_features, coors, batch_size, ny, nx):
    """mmdet3d's PointPillarsScatter.forward_batch; a row outside the canvas is dropped first (the module would index out of range)"""
    ok = (coors[:, 0] >= 0) & (coors[:, 0] < batch_size) & (coors[:, 2] >= 0) & (coors[:, 2] < ny) & (coors[:, 3] >= 0) & (coors[:, 3] < nx)
    voxel_features, coors = voxel_features[ok], coors[ok]
    batch_canvas = []
    for batch_itt in range(batch_size):
        canvas = torch.zeros(voxel_features.size(1), nx * ny, dtype=voxel_features.dtype, device=voxel_features.device)
        batch_mask = coors[:, 0] == batch_itt
        this_coors = coors[batch_mask, :]
        indices = (this_coors[:, 2] * nx + this_coors[:, 3]).type(torch.long)
        canvas[:, indices] = voxel_features[batch_mask, :].t()
        batch_canvas.append(canvas)
    if batch_size == 0:
        return voxel_features.new_zeros((0, voxel_features.size(1), ny, nx))
    return torch.stack(batch_canvas, 0).view(batch_size, voxel_features.size(1), ny, nx)


def single_view_sample(out, pts_xyz, pts_ids, pcrange):
    """pillar_mvf_encoder.py:88-105; `new_empty` is `new_zeros` here (a point of no sample: restated as a zero row)"""
    grid_x = (pts_xyz[:, 0] - pcrange[0]) / ((pcrange[3] - pcrange[0]) / 2) - 1
    grid_y = (pts_xyz[:, 1] - pcrange[1]) / ((pcrange[4] - pcrange[1]) / 2) - 1
    grid_xy = torch.stack((grid_x, grid_y), dim=-1)
    pts_out = out.new_zeros((pts_xyz.size(0), out.size(1)))
    for i in range(out.size(0)):
        b_idx = torch.where(pts_ids == i)
        b_grid_xy = grid_xy[b_idx]
        b_grid_xy = b_grid_xy[None, None, ...]
        b_out = out[i:(i + 1)]
        b_pts_out = F.grid_sample(b_out, b_grid_xy, mode='bilinear', padding_mode='zeros', align_corners=False)
        b_pts_out = b_pts_out.reshape(out.size(1), -1).permute(1, 0)
        pts_out = pts_out.index_put(b_idx, b_pts_out)
    return pts_out


# ---- the library's fixed fp32 sequences in numpy -------------------------------------------------------------------------------------

f32 = np.float32


def np_atan_pos(t):
    hi, mid = t > f32(2.414213562373095), t > f32(0.4142135623730950)
    x_hi = -(f32(1.0) / t)
    x_mid = (t - f32(1.0)) / (t + f32(1.0))
    y0 = np.where(hi, f32(1.5707963267948966), np.where(mid, f32(0.7853981633974483), f32(0.0)))
    x = np.where(hi, x_hi, np.where(mid, x_mid, t))
    z = x * x
    p = (((f32(8.05374449538e-2) * z - f32(1.38776856032e-1)) * z + f32(1.99777106478e-1)) * z - f32(3.33329491539e-1)) * z * x + x
    return y0 + p


def np_atan2(y, x):
    """csrc/rbox_device.h's fx_atan2f"""
    with np.errstate(all='ignore'):
        pi = f32(3.14159265358979323846)
        t = y / x
        ap = np_atan_pos(np.where(t < 0, -t, t))
        a = np.where(t < 0, -ap, ap)
        shifted = np.where(y < 0, a - pi, a + pi)
        a = np.where(x < 0, shifted, a)
        axis = np.where(y > 0, f32(1.5707963267948966), np.where(y < 0, f32(-1.5707963267948966), f32(0.0)))
        return np.where(x == 0, axis, a).astype(np.float32)


def np_transform(view, pts):
    """(N, C) float32 -> the view's rows, include/gd3d.h's sequence"""
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    if view == 'cartesian':
        return pts.copy()
    with np.errstate(all='ignore'):
        s = x * x + y * y
        ang = np_atan2(y, x)
        if view == 'cylindrical':
            head = np.stack([ang, z, np.sqrt(s)], 1)
        else:
            r2 = np.sqrt(s)
            head = np.stack([ang, np_atan2(z, r2), np.sqrt(s + z * z)], 1)
    return np.concatenate([head.astype(np.float32), pts[:, 3:]], 1)


def np_grid(voxel_size, point_cloud_range):
    r = np.array(point_cloud_range, np.float32)
    return np.round((r[3:] - r[:3]) / np.array(voxel_size, np.float32)).astype(np.int64)


def np_coors(view_pts, sample, voxel_size, point_cloud_range):
    """(N, 4) int32 [b, z, y, x]: [b, -1, -1, -1] for a dropped point, all -1 for a row of no sample (sample == -1)"""
    lo, vs = np.array(point_cloud_range[:3], np.float32), np.array(voxel_size, np.float32)
    with np.errstate(all='ignore'):
        f = np.floor((view_pts[:, :3] - lo) / vs)
        inside = ((f >= 0) & (f < np_grid(voxel_size, point_cloud_range).astype(np.float32))).all(1) & (sample >= 0)
    cells = np.where(inside[:, None], f, 0).astype(np.int64)[:, ::-1]          # converted only where the comparison held
    zyx = np.where(inside[:, None], cells, -1)
    return np.concatenate([sample[:, None], zyx], 1).astype(np.int32)


def np_multi_view(pts, counts, views, voxel_sizes, ranges):
    sample = np.full(len(pts), -1, np.int64)
    ends = np.cumsum(np.maximum(np.asarray(counts, np.int64), 0))
    for b in range(len(ends) - 1, -1, -1):
        sample[:ends[b]] = np.where(np.arange(ends[b]) >= (ends[b - 1] if b else 0), b, sample[:ends[b]])
    out_p = [np_transform(v, pts) for v in views]
    return out_p, [np_coors(p, sample, vs, r) for p, vs, r in zip(out_p, voxel_sizes, ranges)]


def np_pixel(v, lo, hi, n):
    half = f32((hi - lo) / 2.0)
    with np.errstate(all='ignore'):
        g = (v - f32(lo)) / half - f32(1.0)
        return (((g + f32(1.0)) * f32(n) - f32(1.0)) / f32(2.0)).astype(np.float32)


def np_view_sample(view_map, xy, ids, pcrange):
    """view_map (B, C, H, W) float32, xy (N, 2) float32, ids (N,) -> (N, C) float32: include/gd3d.h's sequence"""
    B, C, H, W = view_map.shape
    ix, iy = np_pixel(xy[:, 0], pcrange[0], pcrange[3], W), np_pixel(xy[:, 1], pcrange[1], pcrange[4], H)
    with np.errstate(all='ignore'):
        reach = (ix > -1) & (ix < f32(W)) & (iy > -1) & (iy < f32(H)) & (ids >= 0) & (ids < B)
    ix, iy = np.where(reach, ix, f32(0)), np.where(reach, iy, f32(0))
    x0, y0 = np.floor(ix), np.floor(iy)
    x1, y1 = x0 + f32(1), y0 + f32(1)
    w = [(x1 - ix) * (y1 - iy), (ix - x0) * (y1 - iy), (x1 - ix) * (iy - y0), (ix - x0) * (iy - y0)]
    acc = None
    b = np.where(reach, ids, 0).astype(np.int64)
    for j in range(4):
        xj, yj = x0.astype(np.int64) + (j & 1), y0.astype(np.int64) + (j >> 1)
        use = reach & (xj >= 0) & (xj < W) & (yj >= 0) & (yj < H)
        val = np.where(use[:, None], view_map[b, :, np.clip(yj, 0, H - 1), np.clip(xj, 0, W - 1)], f32(0))
        term = (val * w[j][:, None].astype(np.float32)).astype(np.float32)
        acc = term if acc is None else (acc + term).astype(np.float32)
    return acc


# ---- transform cases ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def transform_points(n, C, seed=0):
    """(n, C) fp32 rows over and a little beyond the shipped ranges"""
    g = torch.Generator().manual_seed(1000 * n + 10 * C + seed)
    xyz = torch.rand(n, 3, generator=g) * torch.tensor([85.0, 90.0, 6.0]) + torch.tensor([-10.0, -45.0, -4.0])
    return torch.cat([xyz, torch.rand(n, C - 3, generator=g)], 1)


def split_counts(n):
    """three samples, the middle one empty"""
    a = n // 2
    return [a, 0, n - a]


def stacked_counts(n):
    """counts with an empty middle sample whose sum leaves two rows of no sample (n >= 3)"""
    return [n // 2, 0, n - n // 2 - 2] if n >= 3 else [n]


@functools.lru_cache(maxsize=None)
def transform_reference(n, C, views):
    """-> (points, r32, r64): the reference's statements on the per-sample list, per view {'v<i>.c<j>': column}"""
    pts = transform_points(n, C)
    res = []
    for dtype in (torch.float32, torch.float64):
        out = {}
        parts = list(torch.split(pts.to(dtype), split_counts(n)))
        for i, v in enumerate(views):
            vp, _ = voxelize_view(v, dynamic_voxelizer(*GEOMETRY[v]), parts)
            for j in range(C):
                out[f'v{i}.c{j}'] = vp[:, j]
        res.append(out)
    return pts, res[0], res[1]


def robustness_points():
    """rows 0-9 non-finite or huge in one coordinate, then the origin, x = 0 with y != 0 (both signs), and an ordinary row"""
    nan, inf = float('nan'), float('inf')
    rows = [[nan, 1, 0], [1, nan, 0], [1, 1, nan], [inf, 1, 0], [-inf, 1, 0], [1, inf, 0], [1, 1, -inf], [1e30, 1, 0], [1, -1e30, 0], [1, 1, 1e30],
            [0, 0, 0], [0, 2, -1], [0, -2, -1], [10, 1, -1]]
    pts = torch.tensor(rows, dtype=torch.float32)
    return torch.cat([pts, torch.arange(len(rows) * 2, dtype=torch.float32).reshape(-1, 2) + 0.5], 1), 10


def face_points():
    """cartesian points on cell faces of the shipped geometry and one fp32 ulp either side (x, and y, on faces 0, 1, 100 and the last)"""
    vs, rng = GEOMETRY['cartesian']
    rows = []
    for k in (0, 1, 100, 432):
        for axis, lo in ((0, rng[0]), (1, rng[1])):
            face = np.float32(lo) + np.float32(k) * np.float32(vs[axis])
            for v in (np.nextafter(face, np.float32(-1e9)), face, np.nextafter(face, np.float32(1e9))):
                row = [5.0, 1.0, -1.0]
                row[axis] = float(v)
                rows.append(row)
    return torch.tensor(rows, dtype=torch.float32)


# ---- scatter cases -----------------------------------------------------------------------------------------------------------------

SCATTER_V = (0, 1, 63, 65, 1025)
SCATTER_C = (1, 3, 64, 260)
SCATTER_CANVAS = (5, 7)


@functools.lru_cache(maxsize=None)
def scatter_case(V, C, B, ny, nx, seed=0):
    """unique (b, y, x) rows sorted as a Scatter's, sample 1 of 3 empty, plus (V >= 63) six rows outside the canvas: y = -1, y = ny,
    x = -1, x = nx, b = B and b = -1; voxels beyond the canvas' cells get b = B + 1: outside as well"""
    g = torch.Generator().manual_seed(7 * V + C + 31 * B + seed)
    cells = [(b, y, x) for b in range(B) if not (B == 3 and b == 1) for y in range(ny) for x in range(nx)]
    outside = [(0, -1, 0), (0, ny, 0), (0, 0, -1), (0, 0, nx), (B, 0, 0), (-1, 0, 0)] if V >= 63 else []
    inside = V - len(outside)
    many = inside > len(cells)
    pick = sorted(torch.randperm(len(cells), generator=g)[:min(inside, len(cells))].tolist())
    rows = [cells[i] for i in pick] + outside + ([(B + 1, 0, 0)] * (inside - len(cells)) if many else [])
    assert len(rows) == V
    coors = torch.tensor([[b, 0, y, x] for b, y, x in rows], dtype=torch.int64).reshape(V, 4)
    coors[:, 1] = torch.randint(0, 3, (V,), generator=g)       # z: ignored
    kept = coors[(coors[:, 0] >= 0) & (coors[:, 0] < B) & (coors[:, 2] >= 0) & (coors[:, 2] < ny) & (coors[:, 3] >= 0) & (coors[:, 3] < nx)]
    assert len(torch.unique(kept[:, [0, 2, 3]], dim=0)) == len(kept), 'coors are unique per (b, y, x)'
    feats = torch.randn(V, C, generator=g)
    grad = torch.randn(B, C, ny, nx, generator=g)
    return dict(feats=feats, coors=coors, B=B, ny=ny, nx=nx, grad=grad)


def scatter_reference(case):
    f = case['feats'].clone().requires_grad_(True)
    canvas = pillars_scatter(f, case['coors'], case['B'], case['ny'], case['nx'])
    canvas.backward(case['grad'])
    return canvas.detach(), f.grad


# ---- sampling cases ----------------------------------------------------------------------------------------------------------------

SAMPLE_B = 3
SAMPLE_KEYS = ('out', 'grad_map')
PLACEMENTS = ('inside', 'centres', 'outer_half', 'outside_near', 'outside_far', 'huge', 'bad_ids', 'empty_sample')
SAMPLE_SHAPES = {'c1_1x1': (1, 1, 1), 'c3_2x2': (3, 2, 2), 'c64_5x7': (64, 5, 7), 'c260_5x7': (260, 5, 7), 'c3_100x40': (3, 100, 40)}


def sample_range(H, W):
    """cells of 0.25 x 0.5 from (-1, 2): every cell centre and face is exactly representable"""
    return (-1.0, 2.0, 0.0, -1.0 + 0.25 * W, 2.0 + 0.5 * H, 1.0)


def pixel64(xy, rng, H, W):
    x, y = xy[:, 0].double(), xy[:, 1].double()
    return ((x - rng[0]) / ((rng[3] - rng[0]) / 2) * W - 1) / 2, ((y - rng[1]) / ((rng[4] - rng[1]) / 2) * H - 1) / 2


def make_sample(kind, C, H, W, n=65, seed=0):
    """a named placement on a (SAMPLE_B, C, H, W) map; every placement's precondition is asserted on fp64 pixel coordinates"""
    g = torch.Generator().manual_seed(97 * C + 13 * H + W + 7 * PLACEMENTS.index(kind) + seed)
    rng = sample_range(H, W)
    B = SAMPLE_B
    ids = torch.randint(0, B, (n,), generator=g)
    u = torch.rand(n, 2, generator=g)
    size = torch.tensor([float(W), float(H)])
    if kind in ('inside', 'bad_ids', 'empty_sample'):
        pix = u * (size - 1) if min(H, W) > 1 else u * 0
    elif kind == 'centres':
        pix = torch.floor(u * size)
    elif kind == 'outer_half':                     # the four borders and the four corners in turn
        side = torch.arange(n) % 8
        pix = u * (size - 1)
        half = u * 0.49 + 0.005
        left, right = -half[:, 0], size[0] - 1 + half[:, 0]
        top, bottom = -half[:, 1], size[1] - 1 + half[:, 1]
        pix[:, 0] = torch.where((side == 0) | (side == 4) | (side == 6), left, torch.where((side == 1) | (side == 5) | (side == 7), right, pix[:, 0]))
        pix[:, 1] = torch.where((side == 2) | (side == 4) | (side == 7), top, torch.where((side == 3) | (side == 5) | (side == 6), bottom, pix[:, 1]))
    elif kind == 'outside_near':                   # outside the RANGE by less than a cell: ix in (-1, -0.5) or (W - 0.5, W), one column of
        pix = u * (size - 1)                       # neighbours still in the map
        pix[:, 0] = torch.where(torch.arange(n) % 2 == 0, -0.55 - u[:, 0] * 0.4, size[0] - 0.45 + u[:, 0] * 0.4)
    elif kind == 'outside_far':
        pix = u * (size - 1)
        pix[:, 1] = torch.where(torch.arange(n) % 2 == 0, -1.5 - u[:, 1] * 3, size[1] + 0.5 + u[:, 1] * 3)
    elif kind == 'huge':
        pix = u * (size - 1)
    else:
        raise KeyError(kind)
    xy = torch.stack([rng[0] + (pix[:, 0] + 0.5) * 0.25, rng[1] + (pix[:, 1] + 0.5) * 0.5], 1).float()
    if kind == 'huge':
        bad = torch.tensor([float('nan'), float('inf'), -float('inf'), 1e30, -1e30, 3e38])
        xy[torch.arange(n), torch.arange(n) % 2] = bad[torch.arange(n) % 6]
    if kind == 'bad_ids':
        ids[::3] = -1
        ids[1::3] = B
    if kind == 'empty_sample':
        ids[ids == 1] = 2
    ix, iy = pixel64(xy, rng, H, W)
    inside = (ix > -1) & (ix < W) & (iy > -1) & (iy < H)
    if kind in ('inside', 'bad_ids', 'empty_sample', 'centres'):
        assert bool(((ix >= 0) & (ix <= W - 1) & (iy >= 0) & (iy <= H - 1)).all())
    if kind == 'centres':
        assert bool((ix == ix.round()).all() & (iy == iy.round()).all())
    if kind == 'outer_half':
        assert bool(inside.all()) and bool(((ix < 0) | (ix > W - 1) | (iy < 0) | (iy > H - 1)).all())
        assert bool(((ix < 0) & (iy < 0)).any() & ((ix > W - 1) & (iy > H - 1)).any())
    if kind == 'outside_near':
        assert bool(((ix < -0.5) & (ix > -1) | (ix > W - 0.5) & (ix < W)).all())
    if kind == 'outside_far':
        assert bool((~inside).all())
    if kind == 'huge':
        assert not bool(torch.isfinite(xy).all(dim=1).any()) or bool((xy.abs().max(dim=1).values >= 1e30)[torch.isfinite(xy).all(dim=1)].all())
    if kind == 'empty_sample':
        assert not bool((ids == 1).any())
    pts = torch.cat([xy, torch.randn(n, 3, generator=g)], 1)                 # (n, 5): the tests take the [:, :3] view
    return dict(kind=kind, map=torch.randn(B, C, H, W, generator=g), pts=pts, ids=ids, rng=rng, grad_out=torch.randn(n, C, generator=g))


def _sample_cases():
    cases = {f'{k}_c64_5x7': (k, 64, 5, 7) for k in PLACEMENTS if k != 'centres'}
    cases['centres_c64_4x8'] = ('centres', 64, 4, 8)       # half the range is 1.0 on both axes: the fp32 pixel coordinate of a centre is the integer
    cases.update({f'outer_half_{s}': ('outer_half', *SAMPLE_SHAPES[s]) for s in SAMPLE_SHAPES if s != 'c64_5x7'})
    cases.update({f'inside_{s}': ('inside', *SAMPLE_SHAPES[s]) for s in ('c3_2x2', 'c260_5x7', 'c3_100x40')})
    return cases


SAMPLE_CASES = _sample_cases()
MISALIGNED_OF = 'outer_half_c64_5x7'


def evaluate_sample(case, dtype):
    m = case['map'].to(dtype).clone().requires_grad_(True)          # never the shared case tensor itself
    ids = case['ids']
    out = single_view_sample(m, case['pts'][:, :2].to(dtype), ids, case['rng'])
    out.backward(case['grad_out'].to(dtype))
    return dict(out=out.detach(), grad_map=m.grad)


@functools.lru_cache(maxsize=None)
def sample_reference(name):
    case = make_sample(*SAMPLE_CASES[name])
    return case, evaluate_sample(case, torch.float32), evaluate_sample(case, torch.float64)


@functools.lru_cache(maxsize=None)
def exact_reference(n=4099, C=64, H=4, W=8):
    """The order-free case: points on sixteenths of a cell (weights are multiples of 2^-8), small-integer maps and gradients.  The
    two conditions under which every partial sum is exact in fp32, whatever the order: (1) the fp32 pixel coordinates equal the fp64
    ones — a 4 x 8 map of 0.25 x 0.5 cells, so that the divisor (hi - lo) / 2 is 1.0 on both axes and, with coordinates on a 2^-7 grid, every
    step of the sequence is exact (on a 5 x 7 map the divisor 0.875 rounds the first quotient); (2) every term is a multiple of 2^-8
    and sum |term| per element stays below 2^16, so no partial sum needs more than 24 bits.  -> (case, exact fp64 result)"""
    g = torch.Generator().manual_seed(4099)
    rng = sample_range(H, W)
    pix = torch.stack([torch.randint(-16, 16 * W, (n,), generator=g), torch.randint(-16, 16 * H, (n,), generator=g)], 1).double() / 16
    xy = torch.stack([rng[0] + (pix[:, 0] + 0.5) * 0.25, rng[1] + (pix[:, 1] + 0.5) * 0.5], 1)
    assert bool((xy.float().double() == xy).all())
    ids = torch.randint(-1, SAMPLE_B + 1, (n,), generator=g)
    case = dict(kind='exact', map=torch.randint(-8, 9, (SAMPLE_B, C, H, W), generator=g).float(), pts=torch.cat([xy.float(), torch.zeros(n, 3)], 1), ids=ids,
                rng=rng, grad_out=torch.randint(-4, 5, (n, C), generator=g).float())
    ix32 = torch.from_numpy(np_pixel(case['pts'][:, 0].numpy(), rng[0], rng[3], W)).double()
    iy32 = torch.from_numpy(np_pixel(case['pts'][:, 1].numpy(), rng[1], rng[4], H)).double()
    ix, iy = pixel64(xy, rng, H, W)
    assert bool((ix32 == ix).all() & (iy32 == iy).all()), 'condition 1'
    assert 4 * n * 256 < 2 ** 24 * 2 ** 8 and n * 4 < 2 ** 16, 'condition 2: |g| <= 4, w <= 1, at most n terms per element'
    exact = evaluate_sample(case, torch.float64)
    assert bool((exact['grad_map'] * 256 == (exact['grad_map'] * 256).round()).all())
    return case, exact


# ---- the golden cases --------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(GOLDEN))
