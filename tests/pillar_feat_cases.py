"""Named inputs of the pillar-decoration tests, shared by tests/test_cpu_pillar_feat.py and tests/test_gpu_pillar_feat.py.

A stats case: points (N, 5) fp32 (x, y, z and two trailing feature columns: the tests take `[:, :3]`, `[:, :4]` or all five), coors
(N, ndim) int32 given DIRECTLY (the op takes the rows as they are), voxel_size, point_cloud_range.  The points of a voxel lie inside its
cell and are interleaved with every other voxel's in point order, so "ascending point index inside a voxel" is a real constraint.
A decoration case: features (V, P, C), num_points (V,) with 0, P and values above P among them, coors (V, 4).
"""
import numpy as np

KITTI = dict(voxel_size=(0.16, 0.16, 4.0), point_cloud_range=(0.0, -39.68, -3.0, 69.12, 39.68, 1.0))
NUS = dict(voxel_size=(0.2, 0.2, 8.0), point_cloud_range=(-51.2, -51.2, -5.0, 51.2, 51.2, 3.0))
FAR = dict(voxel_size=(0.005, 0.005, 0.005), point_cloud_range=(9999.0, 9999.0, 9999.0, 10001.0, 10001.0, 10001.0))
F32 = np.float32


def make_stats(seed, sizes, ndim, geom, samples=1, dropped=(), spread=0.98, origin=(3, 5, 2)):
    """sizes: points per voxel; voxel j sits in cell (x, y, z) = origin + (j % 9, j // 9 % 9, j // 81) of sample j % samples;
    dropped: coors rows appended as they are (points anywhere)"""
    rng = np.random.default_rng(seed)
    vs, lo = np.array(geom['voxel_size'], F32), np.array(geom['point_cloud_range'][:3], F32)
    pts, rows = [], []
    for j, n in enumerate(sizes):
        cell = np.array(origin) + np.array([j % 9, j // 9 % 9, j // 81])
        centre = lo + (cell.astype(F32) + F32(0.5)) * vs
        xyz = centre + (rng.random((n, 3), dtype=F32) - F32(0.5)) * vs * F32(spread)
        pts.append(np.concatenate([xyz, rng.random((n, 2), dtype=F32)], 1))
        row = [cell[2], cell[1], cell[0]]
        rows += [([j % samples] if ndim == 4 else []) + row] * n
    for row in dropped:
        assert len(row) == ndim
        pts.append(np.concatenate([lo + rng.random((1, 3), dtype=F32) * F32(5.0), rng.random((1, 2), dtype=F32)], 1))
        rows.append(list(row))
    if not pts:
        return dict(points=np.zeros((0, 5), F32), coors=np.zeros((0, ndim), np.int32), **geom)
    points, coors = np.concatenate(pts, 0).astype(F32), np.array(rows, np.int32).reshape(-1, ndim)
    perm = rng.permutation(len(points))
    return dict(points=np.ascontiguousarray(points[perm]), coors=np.ascontiguousarray(coors[perm]), **geom)


def _nonfinite():
    c = make_stats(7, [4, 5, 3, 6, 2, 5, 4], 4, KITTI, samples=2, dropped=[(-1, -1, -1, -1)] * 2)
    pmap = {tuple(r): None for r in c['coors'].tolist()}
    cells = [r for r in pmap if min(r) >= 0]
    first = lambda cell, k=0: np.flatnonzero((c['coors'] == np.array(cell)).all(1))[k]
    c['points'][first(cells[0]), 0] = np.nan                     # poisons its own voxel's x mean, covariance row and column
    c['points'][first(cells[1]), 1] = np.inf
    c['points'][first(cells[2]), 2] = -np.inf
    c['points'][first(cells[3], 0), 0] = np.inf                  # +inf and -inf in one voxel: the mean itself is NaN
    c['points'][first(cells[3], 1), 0] = -np.inf
    c['points'][np.flatnonzero((c['coors'] < 0).all(1))[0], 1] = np.nan   # a dropped NaN point
    return c


_RNG = np.random.default_rng(99)
STATS = {
    'n0': make_stats(1, [], 4, KITTI),
    'n1': make_stats(2, [1], 4, KITTI),
    'every_point_dropped': make_stats(3, [], 4, KITTI, dropped=[(-1, -1, -1, -1)] * 36 + [(0, 5, -1, 2)]),
    'one_voxel_300': make_stats(4, [300], 3, NUS),
    'sizes_1_to_9': make_stats(5, [1, 2, 3, 4, 5, 7, 8, 9] * 3, 4, KITTI, samples=3),                     # the 4-unroll and its tail
    'v75_unbatched': make_stats(6, _RNG.integers(1, 7, 75).tolist(), 3, NUS, dropped=[(-1, -1, -1)] * 10),   # 75 % 16 = 11, 75 % 4 = 3
    'three_samples_dropped': make_stats(8, _RNG.integers(1, 12, 40).tolist(), 4, KITTI, samples=3,
                                        dropped=[(-1, -1, -1, -1)] * 7 + [(0, 5, -1, 2), (2, -3, 4, 4), (-1, 0, 7, 9)]),
    'nonfinite': _nonfinite(),
    'near_1e4': make_stats(9, [6, 3, 9, 1, 4], 3, FAR, origin=(199, 200, 201)),                            # coordinates near 1e4, 1e-2 spread
}

DECO_SHAPES = [(0, 5, 4), (1, 1, 3), (1, 20, 4), (300, 5, 4), (300, 32, 4), (37, 33, 5), (20, 64, 3), (9, 100, 5), (300, 20, 5)]


def make_deco(V, P, C, geom=KITTI, seed=0, garbage=None):
    """voxels with num_points in [0, P + 3] (0, P and P + 2 forced where V allows); filled slots inside the voxel's cell; padded slots
    zero, or `garbage` ('finite' | 'nan')"""
    rng = np.random.default_rng(1000 * V + 10 * P + C + seed)
    vs, lo = np.array(geom['voxel_size'], F32), np.array(geom['point_cloud_range'][:3], F32)
    coors = np.stack([rng.integers(0, 4, V), np.zeros(V, np.int64), rng.integers(0, 400, V), rng.integers(0, 400, V)], 1).astype(np.int32)
    num = rng.integers(0, P + 4, V).astype(np.int32)
    for i, forced in enumerate((P, 0, P + 2)):
        if V > i:
            num[i] = forced
    centre = lo + (coors[:, :0:-1].astype(F32) + F32(0.5)) * vs
    feats = np.concatenate([centre[:, None, :] + (rng.random((V, P, 3), dtype=F32) - F32(0.5)) * vs, rng.random((V, P, C - 3), dtype=F32)], 2)
    pad = np.arange(P)[None, :] >= num[:, None]
    fill = {None: F32(0), 'finite': None, 'nan': F32(np.nan)}[garbage]
    if fill is not None:
        feats[pad] = fill
    else:
        feats[pad] = (rng.random((int(pad.sum()), C), dtype=F32) - F32(0.5)) * F32(1e3)
    return dict(features=np.ascontiguousarray(feats.astype(F32)), num_points=num, coors=coors, **geom)
