"""Seeded inputs of the voxel-set-abstraction tests (tests/test_vsa_cpu.py, tests/test_gpu_vsa.py) and their numpy-oracle
results, computed once per process and never modified.

The kernels' constants the shapes are chosen around (csrc/vsa.hip): 8 queries per workgroup, 64 points per scan step, tiles of
1024 points, 16384 points of a sample in registers for FPS."""
import functools

import numpy as np

import vsa_ref

QW, STEP, TILE, FPS_CAP = 8, 64, 1024, 16384

# (points per sample, queries per sample): B = 3 with unequal counts; a sample without points, one without queries; M no multiple
# of 8; sample sizes 1, 63, 64, 65, one tile - 1, exact, + 1, and more than two tiles
STACKS = {
    'tile+1_nopoints_64': ((1025, 0, 64), (11, 2, 6)),
    '63_tile-1_noqueries': ((63, 1023, 200), (9, 5, 0)),
    '1_tile_2tiles+': ((1, 1024, 2100), (3, 10, 13)),
    'small_1_64_65': ((1, 64, 65), (2, 3, 4)),
}


@functools.lru_cache(maxsize=None)
def stack(name):
    """Random points in a box of side 4 and query centres: most ON a point of their sample (dense balls, more members than any
    nsample used at radius 0.9; fewer at 0.25), every fourth far outside (empty balls)."""
    pts, qry = STACKS[name]
    rng = np.random.RandomState(sum(map(ord, name)))
    xyz = rng.uniform(-2, 2, (sum(pts), 3)).astype(np.float32)
    new_xyz = np.zeros((sum(qry), 3), np.float32)
    ps, row = vsa_ref.starts(pts), 0
    for b, (n, m) in enumerate(zip(pts, qry)):
        for j in range(m):
            if n == 0 or j % 4 == 3:
                new_xyz[row] = (50.0 + j, -40.0, 30.0)
            else:
                new_xyz[row] = xyz[ps[b] + rng.randint(n)] + rng.uniform(-0.05, 0.05, 3).astype(np.float32)
            row += 1
    feats = rng.uniform(-1, 1, (sum(pts), 67)).astype(np.float32)
    for a in (xyz, new_xyz, feats):
        a.setflags(write=False)
    return xyz, np.asarray(pts, np.int32), new_xyz, np.asarray(qry, np.int32), feats


# positions (in index order of the sample) of the points near the origin, listed by increasing distance: the first K of them are
# the members at radius crafted_radius(K); they straddle the 64-point step (63 | 64) and the tile boundary (1023 | 1024) already at K = 5
CRAFTED_POS = (3, 63, 64, 1023, 1024, 65, 62, 127, 128, 500, 1022, 1025, 700, 800, 900, 1000) + tuple(range(1030, 1054))
CRAFTED_N = 1100


def crafted_radius(k):
    """between member k-1 (distance 0.1 + 0.02 (k-1)) and member k: exactly k members"""
    return 0.1 + 0.02 * k - 0.01


@functools.lru_cache(maxsize=None)
def crafted():
    """One sample of 1100 points, all far away except 40 near the origin at distances 0.10, 0.12, ... (see CRAFTED_POS); a second
    sample of 70 far points only.  Queries: 5 at the origin of sample 0, 2 in sample 1 (empty)."""
    rng = np.random.RandomState(7)
    xyz = (rng.uniform(100, 200, (CRAFTED_N + 70, 3))).astype(np.float32)
    for j, pos in enumerate(CRAFTED_POS):
        d = 0.1 + 0.02 * j
        ang = 0.7 * j
        xyz[pos] = (d * np.cos(ang), d * np.sin(ang), 0.0)
    new_xyz = np.zeros((7, 3), np.float32)
    feats = rng.uniform(-1, 1, (CRAFTED_N + 70, 16)).astype(np.float32)
    for a in (xyz, new_xyz, feats):
        a.setflags(write=False)
    return xyz, np.asarray((CRAFTED_N, 70), np.int32), new_xyz, np.asarray((5, 2), np.int32), feats


@functools.lru_cache(maxsize=None)
def exact_radius():
    """Integer coordinates, radius 5: the offset (3, 4, 0) has d2 == radius2 == 25 exactly in fp32 and must be EXCLUDED (strict <);
    (3, 3, 0) and (0, 4, 2) are inside."""
    xyz = np.asarray([(13, 24, 7), (13, 23, 7), (10, 24, 9), (15, 20, 7), (10, 25, 7), (10, 20, 12), (40, 40, 40)], np.float32)
    new_xyz = np.asarray([(10, 20, 7), (40, 40, 45)], np.float32)
    return xyz, np.asarray((7,), np.int32), new_xyz, np.asarray((2,), np.int32)


@functools.lru_cache(maxsize=None)
def reference(kind, name, radius, nsample, c, use_xyz):
    """oracle (out, idx, cnt, mask) of a stack; c = 0: features=None"""
    xyz, pc, new_xyz, qc, feats = crafted() if kind == 'crafted' else stack(name)
    f = None if c == 0 else np.ascontiguousarray(feats[:, :c])
    res = vsa_ref.query_and_group(radius, nsample, xyz, pc, new_xyz, qc, f, use_xyz)
    for a in res:
        a.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def duplication():
    """Backward with heavy duplication: 2 samples; 40 queries at ONE centre of sample 0 (all name the same members), 9 spread
    queries with padded tails (fewer members than nsample), 3 empty balls."""
    rng = np.random.RandomState(11)
    pts = (300, 130)
    xyz = rng.uniform(-2, 2, (sum(pts), 3)).astype(np.float32)
    centre = xyz[17]
    far = np.asarray((90.0, 90.0, 90.0), np.float32)
    q0 = [centre] * 40 + [xyz[rng.randint(300)] for _ in range(5)] + [far] * 2
    q1 = [xyz[300 + rng.randint(130)] for _ in range(4)] + [far]
    new_xyz = np.asarray(q0 + q1, np.float32)
    for a in (xyz, new_xyz):
        a.setflags(write=False)
    return xyz, np.asarray(pts, np.int32), new_xyz, np.asarray((len(q0), len(q1)), np.int32)


FPS_SIZES = (1, 2, 63, 64, 65, 1024, 1025, FPS_CAP - 1, FPS_CAP, FPS_CAP + 1, 0)   # 0: the sharpened empty sample -> zeros


@functools.lru_cache(maxsize=None)
def fps_cloud():
    rng = np.random.RandomState(5)
    xyz = rng.uniform(-30, 30, (sum(FPS_SIZES), 3)).astype(np.float32)
    xyz.setflags(write=False)
    return xyz, np.asarray(FPS_SIZES, np.int32)


@functools.lru_cache(maxsize=None)
def fps_reference(npoint):
    xyz, cnt = fps_cloud()
    out = vsa_ref.fps_stacked(xyz, cnt, npoint)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def fps_ties():
    """Exactly equal distances: sample 0 = a 9 x 9 x 9 integer lattice in a seeded random order (many points at the same distance
    from every pick), sample 1 = 150 random points each present three times (running minima of 0 shared by the copies), sample 2 = the
    lattice again, 23 copies of it laid end to end beyond the register capacity (ties between the register part and the rest)."""
    rng = np.random.RandomState(3)
    g = np.stack(np.meshgrid(np.arange(9), np.arange(9), np.arange(9), indexing='ij'), -1).reshape(-1, 3).astype(np.float32)
    lattice = g[rng.permutation(len(g))]
    base = rng.uniform(-5, 5, (150, 3)).astype(np.float32)
    dup = np.concatenate([base, base, base])[rng.permutation(450)]
    big = np.concatenate([lattice] * 23)                                   # 16767 points > 16384
    xyz = np.ascontiguousarray(np.concatenate([lattice, dup, big]))
    xyz.setflags(write=False)
    return xyz, np.asarray((len(lattice), len(dup), len(big)), np.int32)
