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


def _stacked(pts, qry, seed, far_query):
    rng = np.random.RandomState(seed)
    xyz = rng.uniform(-2, 2, (sum(pts), 3)).astype(np.float32)
    new_xyz = np.zeros((sum(qry), 3), np.float32)
    ps, row = vsa_ref.starts(pts), 0
    for b, (n, m) in enumerate(zip(pts, qry)):
        for j in range(m):
            if n == 0 or far_query(j, m):
                new_xyz[row] = (50.0 + j, -40.0, 30.0)
            else:
                new_xyz[row] = xyz[ps[b] + rng.randint(n)] + rng.uniform(-0.05, 0.05, 3).astype(np.float32)
            row += 1
    feats = rng.uniform(-1, 1, (sum(pts), 67)).astype(np.float32)
    for a in (xyz, new_xyz, feats):
        a.setflags(write=False)
    return xyz, np.asarray(pts, np.int32), new_xyz, np.asarray(qry, np.int32), feats


# nsample above one wave of slots (the wrappers admit up to 1024): 2300 points are more than two tiles, 700 fewer than the larger
# nsample values, the last sample has no points; M = 12 is no multiple of 8
WIDE = ((2300, 700, 0), (7, 4, 1))
R_ALL, R_MID = 10.0, 1.0
# 33: first value above the older tests' 32; 63 | 64 | 65: one wave of slots; 128: a second pass of the slot loops; 543 | 544:
# channels per pass through the transpose buffer 2 -> 1; 576 | 577: the fused launch's dynamic LDS crosses 64 KiB; 960 | 961: the
# stand-alone grouping's does; 1023 | 1024: the limit
WIDE_NSAMPLE = (33, 63, 64, 65, 128, 543, 544, 576, 577, 960, 961, 1023, 1024)


@functools.lru_cache(maxsize=None)
def wide():
    """Points in the side-4 box as `stack`; every sample's LAST query lies far outside (empty ball), the others on a point of their
    sample.  At R_ALL (larger than the box's diagonal) every point of the sample is a member: sample 0 fills any nsample, sample 1
    has exactly 700 members (full up to nsample 700, a padded tail of up to 324 slots above).  At R_MID a ball holds 100 to 140
    of the 2300 points, spread over all three tiles (either side of nsample 128), or 30 to 50 of the 700."""
    return _stacked(WIDE[0], WIDE[1], 2300, lambda j, m: j == m - 1)


@functools.lru_cache(maxsize=None)
def wide_members(radius):
    """members per query before the clip to nsample, up to 1024 (the oracle at the limit)"""
    return reference('wide', '', radius, 1024, 0, True)[2]


@functools.lru_cache(maxsize=None)
def stack(name):
    """Random points in a box of side 4 and query centres: most ON a point of their sample (dense balls, more members than any
    nsample used at radius 0.9; fewer at 0.25), every fourth far outside (empty balls)."""
    pts, qry = STACKS[name]
    return _stacked(pts, qry, sum(map(ord, name)), lambda j, m: j % 4 == 3)


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


def inputs(kind, name):
    """(xyz, xyz_cnt, new_xyz, new_cnt, feats) of kind 'crafted', 'wide' or 'stack' (the latter by name)"""
    return crafted() if kind == 'crafted' else wide() if kind == 'wide' else stack(name)


@functools.lru_cache(maxsize=None)
def reference(kind, name, radius, nsample, c, use_xyz):
    """oracle (out, idx, cnt, mask) of a stack; c = 0: features=None"""
    xyz, pc, new_xyz, qc, feats = inputs(kind, name)
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


# beyond the registers a thread visits points FPS_CAP + tid, + 1024, ...: 17408 = the last size with one such visit, 17409 the first
# with two; two samples that use the workspace lie before one that does not (300), one after it
FPS_DEEP_SIZES = (FPS_CAP + 1024, FPS_CAP + 1025, 20000, 300, 18500)
FPS_DEEP_NPOINT = (1, 600, 19000)     # 19000: above four of the sizes (wrap-around) and below the fifth, in one launch


@functools.lru_cache(maxsize=None)
def fps_deep():
    rng = np.random.RandomState(17)
    xyz = rng.uniform(-30, 30, (sum(FPS_DEEP_SIZES), 3)).astype(np.float32)
    xyz.setflags(write=False)
    return xyz, np.asarray(FPS_DEEP_SIZES, np.int32)


@functools.lru_cache(maxsize=None)
def fps_deep_reference(npoint):
    xyz, cnt = fps_deep()
    out = vsa_ref.fps_stacked(xyz, cnt, npoint)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def fps_deep_ties():
    """the 729-point lattice of `fps_ties` 26 times end to end, 18954 points: exactly equal distances between the register part
    (copies 0-22), the workspace points a thread visits first (up to 17407) and those it visits second"""
    lattice = fps_ties()[0][:729]
    xyz = np.ascontiguousarray(np.concatenate([lattice] * 26))
    xyz.setflags(write=False)
    return xyz, np.asarray((len(xyz),), np.int32)


@functools.lru_cache(maxsize=None)
def fps_deep_ties_reference(npoint):
    out = vsa_ref.fps_stacked(*fps_deep_ties(), npoint)
    out.setflags(write=False)
    return out


FPS_BATCHED_SHAPE, FPS_BATCHED_NPOINT = (2, FPS_CAP + 1025, 3), 300


@functools.lru_cache(maxsize=None)
def fps_batched():
    """two equal samples that both use the workspace, for the batched entry point (sample b starts at b * n)"""
    xyz = np.random.RandomState(19).uniform(-30, 30, FPS_BATCHED_SHAPE).astype(np.float32)
    ref = np.stack([vsa_ref.fps(x, FPS_BATCHED_NPOINT) for x in xyz])
    xyz.setflags(write=False)
    ref.setflags(write=False)
    return xyz, ref


def wide_conditions(radius, nsample):
    """What a (radius, nsample) pair of `wide` must contain, asserted on the ORACLE's result before anything is compared with it
    (another seed cannot silently drop a case); returns the oracle's cnt."""
    _, idx, cnt, mask = reference('wide', '', radius, nsample, 0, True)
    members = wide_members(radius)
    s0, s1 = slice(0, 6), slice(7, 10)                                  # the queries on points of sample 0 and of sample 1
    assert mask.tolist() == [False] * 6 + [True] + [False] * 3 + [True] * 2 and (cnt[mask] == 0).all()    # empty balls
    if members.max() >= nsample:                                        # a full ball wherever the geometry has one
        assert (cnt == nsample).any()
    if radius == R_ALL:
        assert (cnt[s0] == nsample).all() and (cnt[s1] == min(700, nsample)).all()
    else:
        assert members.max() < 1024                                     # `members` is not clipped
        if nsample == 128:                                              # the second pass of the slot loops ends inside a ball
            assert ((cnt > 64) & (cnt < 128)).any()
        if nsample in (64, 65):    # a ball that fills in a LATER tile than its first member's, non-members in between
            full = cnt == nsample
            assert (full & (idx[:, nsample - 1] >= TILE) & (idx[:, 0] < TILE)).any()
            assert (idx[full, nsample - 1] - idx[full, 0] >= nsample).all()
    return cnt
