"""TEST INFRASTRUCTURE: mmdet3d's published `hard_voxelize` / `dynamic_voxelize` and `HardSimpleVFE`, restated in numpy fp32 as a plain
Python loop (the sequential walk of include/gd3d.h), and the table of named cases tests/test_cpu_hard_voxel.py and
tests/test_gpu_hard_voxel.py share.  Every case is small enough for the loop to run in milliseconds (the 70 000-point sweep: well under a
second); a case's expectation is computed once (`expected`) and never modified.

A case is a dict: samples (list of (n_b, width) fp32 arrays), voxel_size, point_cloud_range, P (max_num_points), MV (max_voxels),
F (num_features), pad (extra trailing columns the op must not copy: the points are handed over as a `[:, :C]` view of a wider tensor,
so the row stride is larger than C)."""
import functools

import numpy as np

f32 = np.float32
SMALL = dict(voxel_size=(0.5, 0.5, 1.0), point_cloud_range=(0.0, -4.0, -2.0, 8.0, 4.0, 2.0))          # grid 16 x 16 x 4
KITTI = dict(voxel_size=(0.05, 0.05, 0.1), point_cloud_range=(0.0, -40.0, -3.0, 70.4, 40.0, 1.0))      # grid 1408 x 1600 x 40: 70.4 / 0.05
PILLAR = dict(voxel_size=(0.16, 0.16, 4.0), point_cloud_range=(0.0, -39.68, -3.0, 69.12, 39.68, 1.0))  # and 4 / 0.1 are inexact in fp32


def grid_of(voxel_size, point_cloud_range):
    """round((range[3:] - range[:3]) / voxel_size) in fp32 (np.round and torch.round both round half to even) -> (Gx, Gy, Gz)"""
    rng, vs = np.asarray(point_cloud_range, f32), np.asarray(voxel_size, f32)
    return tuple(int(v) for v in np.round((rng[3:] - rng[:3]) / vs))


def cells_of(points, voxel_size, point_cloud_range):
    """(n, >= 3) fp32 -> (cells (n, 3) int64 x y z, kept (n,) bool): floor((p - lo) / vs) in fp32, compared as floats"""
    grid = np.asarray(grid_of(voxel_size, point_cloud_range), f32)
    lo, vs = np.asarray(point_cloud_range[:3], f32), np.asarray(voxel_size, f32)
    with np.errstate(all='ignore'):
        f = np.floor((points[:, :3].astype(f32) - lo) / vs)
        assert f.dtype == f32
        kept = ((f >= 0) & (f < grid)).all(1)
    return np.where(kept[:, None], f, 0).astype(np.int64), kept


def hard_voxelize_ref(samples, voxel_size, point_cloud_range, P, MV, C, F):
    """the sequential walk -> dict of the upper-bound arrays (R = min(N, B * MV) rows; tail rows -1 / 0 / 0), voxel_batch_cnt and num"""
    N, B = sum(len(s) for s in samples), len(samples)
    R = min(N, B * MV)
    voxels, mean = np.zeros((R, P, C), f32), np.zeros((R, F), f32)
    coors, num_points = np.full((R, 4), -1, np.int32), np.zeros((R,), np.int32)
    cnt, total, dropped = np.zeros((B,), np.int32), 0, 0
    for b, pts in enumerate(samples):
        cells, kept = cells_of(pts, voxel_size, point_cloud_range)
        voxel_of, base, voxel_num = {}, total, 0
        for i in range(len(pts)):
            if not kept[i]:
                dropped += 1
                continue
            key = tuple(cells[i])
            v = voxel_of.get(key)
            if v is None:
                if voxel_num >= MV:
                    continue                       # not a break: later points of numbered voxels still join them
                v = voxel_of[key] = base + voxel_num
                voxel_num += 1
                coors[v] = (b, key[2], key[1], key[0])
            if num_points[v] >= P:
                continue
            voxels[v, num_points[v]] = pts[i, :C]
            num_points[v] += 1
        cnt[b] = voxel_num
        total += voxel_num
    for v in range(total):                         # HardSimpleVFE: slots 0, 1, 2, .. added in sequence to +0 in fp32, one division
        acc = np.zeros((F,), f32)
        for k in range(num_points[v]):
            acc = acc + voxels[v, k, :F]
        mean[v] = acc / f32(num_points[v])
    assert voxels.dtype == f32 and mean.dtype == f32
    return dict(voxels=voxels, mean=mean, coors=coors, num_points=num_points, voxel_batch_cnt=cnt, num=np.array([total, dropped], np.int64))


def dynamic_voxelize_ref(samples, voxel_size, point_cloud_range):
    out = []
    for b, pts in enumerate(samples):
        cells, kept = cells_of(pts, voxel_size, point_cloud_range)
        row = np.stack([np.full(len(pts), b), cells[:, 2], cells[:, 1], cells[:, 0]], 1)
        out.append(np.where(kept[:, None], row, -1).astype(np.int32))
    return np.concatenate(out, 0) if out else np.zeros((0, 4), np.int32)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------

def _inside(rng, n, geom, width=4, margin=0.0):
    """n points, about a tenth of them outside the range; feature columns in [-1, 1)"""
    lo, hi = np.asarray(geom['point_cloud_range'][:3]), np.asarray(geom['point_cloud_range'][3:])
    span = hi - lo
    xyz = lo - margin * span + rng.random((n, 3)) * span * (1 + 2 * margin)
    return np.concatenate([xyz, rng.random((n, width - 3)) * 2 - 1], 1).astype(f32)


def _in_cell(rng, cell, geom, n, width=4):
    """n points strictly inside cell (x, y, z) of the grid"""
    lo, vs = np.asarray(geom['point_cloud_range'][:3]), np.asarray(geom['voxel_size'])
    xyz = lo + (np.asarray(cell) + 0.25 + 0.5 * rng.random((n, 3))) * vs
    return np.concatenate([xyz, rng.random((n, width - 3)) * 2 - 1], 1).astype(f32)


def _case(samples, geom=SMALL, P=5, MV=100, F=None, pad=0):
    width = samples[0].shape[1]
    C = width - pad
    return dict(samples=[np.ascontiguousarray(s, f32) for s in samples], P=P, MV=MV, C=C, F=C if F is None else F, pad=pad, **geom)


def _build_cases():
    cases = {}
    rng = np.random.default_rng(20240)
    for n in (0, 1, 63, 64, 65, 257):                                      # sample sizes
        cases[f'n{n}'] = _case([_inside(rng, n, SMALL, margin=0.05)])
    cases['three_samples_middle_empty'] = _case([_inside(rng, 70, SMALL, margin=0.05), np.zeros((0, 4), f32), _inside(rng, 40, SMALL, margin=0.05)])
    far = _inside(rng, 33, SMALL) + f32(100.0)
    cases['every_point_dropped'] = _case([far, far[:9]])
    for P in (1, 5, 32):                                                   # the max_num_points cut: P-1, P, P+1 and 3P points, interleaved
        parts = [_in_cell(rng, c, SMALL, k) for c, k in zip([(1, 2, 0), (9, 9, 3), (15, 0, 1), (4, 15, 2)], (P - 1, P, P + 1, 3 * P))]
        tag = np.concatenate([np.full(len(p), i) for i, p in enumerate(parts)])
        order = rng.permutation(len(tag))
        cases[f'slot_cut_p{P}'] = _case([np.concatenate(parts, 0)[order], _in_cell(rng, (1, 2, 0), SMALL, 2 * P + 1)], P=P)
    # the max_voxels cut: 40 distinct cells; later points fall into kept voxels (they join) and into cut cells (dropped)
    cells = [(int(i % 16), int(i // 16 + 3), int(i % 4)) for i in rng.permutation(200)[:40]]
    first = np.concatenate([_in_cell(rng, c, SMALL, 1) for c in cells], 0)
    later = np.concatenate([_in_cell(rng, cells[i], SMALL, 1) for i in rng.integers(0, 40, 90)], 0)
    mixed = np.concatenate([first[:25], later[:30], first[25:], later[30:]], 0)       # kept voxels are rejoined before the last new cells show up
    under = np.concatenate([_in_cell(rng, c, SMALL, 2) for c in cells[:10]], 0)
    cases['voxel_cut_mv16'] = _case([mixed, under], P=3, MV=16)
    cases['voxel_cut_mv1'] = _case([mixed, under[::-1]], P=4, MV=1)
    # faces: exactly lo (cell 0), exactly hi (dropped), one ulp below hi (last cell), one ulp below lo (dropped); non-finite and huge
    lo, hi = np.asarray(SMALL['point_cloud_range'][:3], f32), np.asarray(SMALL['point_cloud_range'][3:], f32)
    rows = []
    for j in range(3):
        for v in (lo[j], hi[j], np.nextafter(hi[j], f32(-np.inf)), np.nextafter(lo[j], f32(-np.inf)), f32(np.nan), f32(np.inf), f32(-np.inf),
                  f32(1e30), f32(-1e30)):
            p = _in_cell(rng, (3, 4, 1), SMALL, 1)[0]
            p[j] = v
            rows.append(p)
    cases['faces_and_non_finite'] = _case([np.stack(rows), np.stack(rows[::-1])])
    # the rounded grid: KITTI's range, points on and next to the far faces
    khi = np.asarray(KITTI['point_cloud_range'][3:], f32)
    edge = _inside(rng, 12, KITTI)
    for i in range(12):
        edge[i, i % 3] = khi[i % 3] if i < 3 else np.nextafter(khi[i % 3], f32(-np.inf)) if i < 6 else khi[i % 3] - f32(0.04) * (i - 5)
    cases['kitti_rounded_grid'] = _case([np.concatenate([_inside(rng, 120, KITTI, margin=0.02), edge], 0)], geom=KITTI, MV=16000)
    dup = _in_cell(rng, (7, 7, 2), SMALL, 1)
    cases['duplicates'] = _case([np.concatenate([np.repeat(dup, 4, 0), _inside(rng, 6, SMALL), np.repeat(dup, 3, 0)], 0)], P=5)
    cases['keys_past_32_bits'] = _case([_inside(rng, 8, KITTI) for _ in range(50)], geom=KITTI, MV=16000)    # 50 * 1408 * 1600 * 40 > 2^32
    for width in (3, 5, 7):                                                # row shapes (4 is everywhere else)
        cases[f'c{width}'] = _case([_inside(rng, 65, SMALL, width=width, margin=0.05), _inside(rng, 30, SMALL, width=width)])
    cases['trailing_columns_c4'] = _case([_inside(rng, 65, SMALL, width=6), _inside(rng, 17, SMALL, width=6)], pad=2)    # stride 6: the scalar path
    cases['trailing_columns_c4_stride8'] = _case([_inside(rng, 65, SMALL, width=8)], pad=4)                                # stride 8: 16-byte rows
    cases['trailing_columns_c3'] = _case([_inside(rng, 65, SMALL, width=4)], pad=1)
    cases['num_features_3_of_4'] = _case([_inside(rng, 130, SMALL)], F=3)
    cases['num_features_4_of_5'] = _case([_inside(rng, 130, SMALL, width=5)], F=4)
    cases['pillars_p32'] = _case([_inside(rng, 257, PILLAR, margin=0.02), _inside(rng, 64, PILLAR)], geom=PILLAR, P=32, MV=40)
    return cases


CASES = _build_cases()
SWEEP = dict(n=70_000, B=3)        # more than one workgroup per kernel by far; built on demand (`sweep_case`)


@functools.lru_cache(maxsize=None)
def sweep_case():
    rng = np.random.default_rng(7)
    geom = dict(voxel_size=(0.5, 0.5, 1.0), point_cloud_range=(0.0, -40.0, -2.0, 80.0, 40.0, 2.0))       # 160 x 160 x 4
    sizes = (30_001, 9_999, 30_000)
    return _case([_inside(rng, n, geom, margin=0.02) for n in sizes], geom=geom, P=5, MV=20_000)


@functools.lru_cache(maxsize=None)
def expected(name):
    """the restatement's outputs of a case, computed once; callers must not modify them"""
    c = sweep_case() if name == 'sweep' else CASES[name]
    out = hard_voxelize_ref(c['samples'], c['voxel_size'], c['point_cloud_range'], c['P'], c['MV'], c['C'], c['F'])
    out['dynamic'] = dynamic_voxelize_ref(c['samples'], c['voxel_size'], c['point_cloud_range'])
    for v in out.values():
        v.setflags(write=False)
    return out


def same_bits(a, b):
    """exact equality, bit for bit for floats (so -0.0 != 0.0 and NaN == the same NaN)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == f32:
        a, b = a.view(np.int32), b.view(np.int32)
    return bool(np.array_equal(a, b))
