"""The cases of tests/test_gpu_ref_kernels.py: the inputs on which the REFERENCE's own device kernels (oracle/_ref/ref_vsa.so,
ref_vox.so through oracle/ref_kernels.py) are compared with the numpy restatements (tests/vsa_ref.py, tests/voxel_query_ref.py,
oracle/voxel_oracle.py), with the product on the device and with its `_cpu` twins.

Importable without a GPU and without the reference libraries.  Every case is held AT IMPORT, on the restatement alone, to contain
what it names (`_assert_*` below): boundary points, empty, exactly full and over-full queries, tie-free and tied clouds.  A change of
a seed or a shape that loses one of them fails here, on the CPU, not silently on the GPU.  All inputs are finite, in bounds and
well formed: the reference kernels are never shown anything else.
"""
import functools

import numpy as np

import vsa_ref
import voxel_query_ref as vq_ref

F = np.float32


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# ------------------------------------------------------------------------------------------------ ball query, grouping

BQ_POINTS = np.asarray((700, 0, 65), np.int32)          # a sample WITHOUT points in the middle
BQ_QUERIES = np.asarray((130, 7, 33), np.int32)         # ... that still has queries: empty balls
BQ_NSAMPLE = (1, 16, 32, 33, 64, 65)                    # both sides of the product's 32- and 64-wide paths
GROUP_C = (1, 3, 16, 35)


@functools.lru_cache(maxsize=None)
def bq_cloud():
    """-> xyz (765, 3), new_xyz (170, 3).  Sample 0: 700 points in a 10 m cube, denser towards its far corner; query 0 sits near
    the thin corner (it is the query `bq_radius` fills exactly), the last two queries of sample 0 lie 100 m away (empty at every
    radius).  Sample 2: 65 points in a 4 m cube."""
    rng = np.random.default_rng(20250301)
    p0 = (10.0 * rng.random((700, 3)) ** 0.6).astype(F)
    p2 = (4.0 * rng.random((65, 3))).astype(F)
    q0 = (10.0 * rng.random((130, 3))).astype(F)
    q0[0] = (1.5, 1.5, 1.5)
    q0[-2:] += 100.0
    q1 = (10.0 * rng.random((7, 3))).astype(F)
    q2 = (4.0 * rng.random((33, 3))).astype(F)
    return _frozen(np.concatenate([p0, p2]), np.concatenate([q0, q1, q2]))


@functools.lru_cache(maxsize=None)
def bq_radius(nsample):
    """the radius at which query 0 has EXACTLY nsample members: halfway between its nsample-th and its next squared distance"""
    xyz, new_xyz = bq_cloud()
    d2 = np.sort(vsa_ref.dist2(new_xyz[0], xyz[:700]).astype(np.float64))
    return float(F(np.sqrt(0.5 * (d2[nsample - 1] + d2[nsample]))))


def bq_members(radius):
    """uncapped member count of every query, by the restatement's own expression"""
    xyz, new_xyz = bq_cloud()
    r2 = F(radius) * F(radius)
    ps, qb = vsa_ref.starts(BQ_POINTS), vsa_ref.sample_of_rows(BQ_QUERIES)
    return np.asarray([(vsa_ref.dist2(new_xyz[q], xyz[ps[b]:ps[b] + BQ_POINTS[b]]) < r2).sum() for q, b in enumerate(qb)])


@functools.lru_cache(maxsize=None)
def bq_reference(nsample):
    """-> (idx, cnt, mask) of the restatement at bq_radius(nsample)"""
    xyz, new_xyz = bq_cloud()
    return _frozen(*vsa_ref.ball_query(bq_radius(nsample), nsample, xyz, BQ_POINTS, new_xyz, BQ_QUERIES))


def _assert_bq():
    for ns in BQ_NSAMPLE:
        members = bq_members(bq_radius(ns))
        assert members[0] == ns, (ns, members[0])                                   # exactly full, nothing to spare
        assert (members > ns).any() and (members == 0).any()                        # over-full; empty
        assert (members[:130] == 0).any() and (members[130:137] == 0).all()         # empty among points; the sample without points
        if ns > 1:
            assert ((members > 0) & (members < ns)).any()                           # a padded tail
        idx, cnt, mask = bq_reference(ns)
        assert np.array_equal(cnt, np.minimum(members, ns)) and np.array_equal(mask, members == 0)


LATTICE_RADIUS, LATTICE_NSAMPLE = 3.0, 64


@functools.lru_cache(maxsize=None)
def bq_lattice():
    """Integer coordinates: a 9 x 9 x 9 lattice (shuffled) and queries on lattice points; at radius 3 the points at offsets
    (3, 0, 0), (2, 2, 1) and their kin lie at d2 == 9 == radius2 EXACTLY: no members of the ball query (strict), members of the
    voxel query (inclusive).  -> xyz (729, 3), cnt (1,), new_xyz (12, 3), new_cnt (1,)"""
    rng = np.random.default_rng(9)
    g = np.stack(np.meshgrid(*(np.arange(9),) * 3, indexing='ij'), -1).reshape(-1, 3).astype(F)
    xyz = g[rng.permutation(len(g))]
    new_xyz = np.asarray([(4, 4, 4), (0, 0, 0), (8, 8, 8), (3, 4, 5), (4, 0, 4), (8, 4, 0), (1, 1, 1), (7, 2, 5), (4, 4, 0), (0, 8, 0),
                          (5, 5, 5), (2, 6, 3)], F)
    return _frozen(xyz, np.asarray((729,), np.int32), new_xyz, np.asarray((12,), np.int32))


def _assert_bq_lattice():
    xyz, _, new_xyz, _ = bq_lattice()
    r2 = F(LATTICE_RADIUS) * F(LATTICE_RADIUS)
    for q in new_xyz:
        d2 = vsa_ref.dist2(q, xyz)
        assert (d2 == r2).sum() >= 3 and (d2 < r2).sum() < (d2 <= r2).sum()           # every query has points ON the sphere
    d2 = vsa_ref.dist2(new_xyz[0], xyz)
    assert (d2 == r2).sum() == 30 and (d2 < r2).sum() == 93                          # the interior query: 6 + 24 on, 93 inside


@functools.lru_cache(maxsize=None)
def group_features(c, integer=False, seed=4):
    rng = np.random.default_rng(seed + c)
    n = int(BQ_POINTS.sum())
    f = rng.integers(-8, 9, (n, c)).astype(F) if integer else rng.standard_normal((n, c)).astype(F)
    return _frozen(f)


def group_rows():
    """(M,) bool: the queries whose sample has points — the rows the reference's grouping can be given (vsa_ref.has_points)"""
    return vsa_ref.has_points(BQ_POINTS, BQ_QUERIES)


def group_counts_for_reference():
    """idx_batch_cnt with the queries of point-less samples taken out: what goes to the reference with idx[group_rows()]"""
    return np.where(BQ_POINTS > 0, BQ_QUERIES, 0).astype(np.int32)


@functools.lru_cache(maxsize=None)
def group_grad_out(nsample, c, integer):
    rng = np.random.default_rng(100 * nsample + c)
    m = int(BQ_QUERIES.sum())
    g = rng.integers(-4, 5, (m, c, nsample)).astype(F) if integer else rng.standard_normal((m, c, nsample)).astype(F)
    return _frozen(g)


# ------------------------------------------------------------------------------------------------ furthest point sampling

FPS_CAP = 16384                                                    # the product keeps this many points in registers (csrc/vsa.hip)
FPS_SMALL = (1, 2, 63, 64, 65)                                     # npoint in (1, n / 2, n)
FPS_LARGE = (1000, 1024, 1025, 5000, FPS_CAP - 1, FPS_CAP, FPS_CAP + 1)   # npoint in (1, 512)
FPS_BATCH = 2


def fps_npoints(n):
    return sorted({1, max(n // 2, 1), n}) if n in FPS_SMALL else [1, 512]


@functools.lru_cache(maxsize=None)
def fps_cloud(n):
    return _frozen(np.random.default_rng(1000 + n).uniform(-30, 30, (FPS_BATCH, n, 3)).astype(F))


@functools.lru_cache(maxsize=None)
def fps_reference(n):
    """-> (picks (B, max npoint) int64 by the restatement, unique (B, max npoint) bool: the running minimum's maximum was attained
    by ONE point when the pick was taken).  The picks for a smaller npoint are a prefix."""
    xyz = fps_cloud(n)
    m = max(fps_npoints(n))
    picks, unique = [], np.ones((FPS_BATCH, m), bool)
    for b in range(FPS_BATCH):
        def trace(p, t, b=b):
            unique[b, p] = (t == t.max()).sum() == 1
        picks.append(vsa_ref.fps(xyz[b], m, trace))
    return _frozen(np.stack(picks), unique)


def _assert_fps():
    for n in FPS_SMALL + FPS_LARGE:
        picks, unique = fps_reference(n)
        assert unique.all(), f'fps cloud n = {n} is not tie-free'
        assert all(len(set(row.tolist())) == len(row) for row in picks)


FPS_TIED_NPOINT = 200


@functools.lru_cache(maxsize=None)
def fps_tied():
    """a 9 x 9 x 9 integer lattice in a seeded random order, (1, 729, 3): many points at exactly the same distance from every pick"""
    return _frozen(np.ascontiguousarray(bq_lattice()[0][None]))


@functools.lru_cache(maxsize=None)
def fps_tied_reference():
    """-> (picks (npoint,), t (npoint, 729): the running minima from which each pick was taken (row 0 unused))"""
    xyz = fps_tied()[0]
    t_at = np.zeros((FPS_TIED_NPOINT, xyz.shape[0]), F)

    def trace(p, t):
        t_at[p] = t
    picks = vsa_ref.fps(xyz, FPS_TIED_NPOINT, trace)
    return _frozen(picks, t_at)


def _assert_fps_tied():
    picks, t_at = fps_tied_reference()
    tied = [(t_at[p] == t_at[p].max()).sum() > 1 for p in range(1, FPS_TIED_NPOINT)]
    assert sum(tied) >= 10                                            # picks taken among several exactly equal maxima
    for p in range(1, FPS_TIED_NPOINT):
        assert picks[p] == np.flatnonzero(t_at[p] == t_at[p].max())[0]   # the restatement takes the lowest arg max


# ------------------------------------------------------------------------------------------------ voxel query

VQ_B, VQ_SHAPE = 2, (5, 12, 10)                                    # (Z, Y, X)
VQ_RANGES = ((0, 0, 0), (1, 1, 1), (2, 3, 4))
VQ_NSAMPLE = (1, 16, 32, 33)
VQ_DEFAULT_RADIUS = {(0, 0, 0): 0.45, (1, 1, 1): 1.3, (2, 3, 4): 2.6}
VQ_VOXEL_SIZE, VQ_PC_RANGE = (1.0, 1.0, 1.0), (0.0, 0.0, 0.0, 10.0, 12.0, 5.0)
VQ_ANCHOR = 0                                                      # the query whose window fixes the radius of a combination


@functools.lru_cache(maxsize=None)
def vq_scene():
    """-> dict(coors (N, 4) unique cells [b, z, y, x] shuffled, xyz (N, 3) = cell centre + jitter, new_xyz (M, 3), counts (B,),
    new_coords (M, 4) by the restatement).  Sample 0 is filled from 15 % (x = 0) to 95 % (x = 9), sample 1 to 12 %.  Queries: the cell
    (2, 6, 5) first (the anchor), all 8 corner cells and 6 face centres of both samples, then random cells."""
    rng = np.random.default_rng(77)
    Z, Y, X = VQ_SHAPE
    rows = []
    for b in range(VQ_B):
        fill = np.linspace(0.15, 0.95, X)[None, None, :] if b == 0 else 0.12
        take = rng.random(VQ_SHAPE) < fill
        if b == 0:
            take[2, 6, 5] = True
        rows += [(b, z, y, x) for z, y, x in np.argwhere(take)]
    coors = np.asarray(rows, np.int64)
    coors = coors[rng.permutation(len(coors))]
    xyz = (coors[:, [3, 2, 1]] + 0.5 + rng.uniform(-0.45, 0.45, (len(coors), 3))).astype(F)
    cells, counts = [], []
    for b, n_rand in ((0, 170), (1, 102)):
        c = [(2, 6, 5)] if b == 0 else []
        c += [(z, y, x) for z in (0, Z - 1) for y in (0, Y - 1) for x in (0, X - 1)]
        c += [(0, 6, 5), (Z - 1, 6, 5), (2, 0, 5), (2, Y - 1, 5), (2, 6, 0), (2, 6, X - 1)]
        c += [tuple(v) for v in np.stack([rng.integers(0, Z, n_rand), rng.integers(0, Y, n_rand), rng.integers(0, X, n_rand)], 1)]
        cells += [(b,) + tuple(int(v) for v in k) for k in c]
        counts.append(len(c))
    cells = np.asarray(cells, np.int64)
    new_xyz = (cells[:, [3, 2, 1]] + 0.5 + rng.uniform(-0.4, 0.4, (len(cells), 3))).astype(F)
    counts = np.asarray(counts, np.int32)
    new_coords = vq_ref.coords_ref(new_xyz, counts, VQ_VOXEL_SIZE, VQ_PC_RANGE, 1)
    assert np.array_equal(new_coords, cells)
    return dict(coors=coors, xyz=xyz, new_xyz=new_xyz, counts=counts, new_coords=new_coords,
                table=vq_ref.table_ref(coors, VQ_SHAPE, VQ_B))


@functools.lru_cache(maxsize=None)
def vq_radius(max_range, nsample):
    """the radius at which the anchor query has EXACTLY nsample members where its window holds more rows than that (halfway between
    its nsample-th and its next squared distance), else the range's default radius"""
    s = vq_scene()
    everything = vq_ref.query_ref(s['xyz'], s['new_xyz'][:1], s['new_coords'][:1], s['table'], max_range, 1e3, 1024)
    rows = everything['idx'][0, :everything['cnt'][0]]
    if len(rows) <= nsample:
        return VQ_DEFAULT_RADIUS[max_range]
    q = s['new_xyz'][VQ_ANCHOR]
    d2 = np.sort(vsa_ref.dist2(q, s['xyz'][rows]).astype(np.float64))
    return float(F(np.sqrt(0.5 * (d2[nsample - 1] + d2[nsample]))))


@functools.lru_cache(maxsize=None)
def vq_reference(max_range, nsample):
    s = vq_scene()
    return vq_ref.query_ref(s['xyz'], s['new_xyz'], s['new_coords'], s['table'], max_range, vq_radius(max_range, nsample), nsample)


def _assert_vq():
    s = vq_scene()
    Z, Y, X = VQ_SHAPE
    n, m = len(s['coors']), len(s['new_xyz'])
    assert 300 <= n <= 600 and len(np.unique(s['coors'], axis=0)) == n and 280 <= m <= 320
    nc = s['new_coords']
    for b in range(VQ_B):
        mine = nc[nc[:, 0] == b][:, 1:]
        have = {tuple(r) for r in mine.tolist()}
        assert all((z, y, x) in have for z in (0, Z - 1) for y in (0, Y - 1) for x in (0, X - 1))           # every corner
        assert all((mine[:, a] == v).any() for a, hi in enumerate((Z, Y, X)) for v in (0, hi - 1))          # every face
    full_for = set()
    for rng_ in VQ_RANGES:
        cells = (2 * rng_[0] + 1) * (2 * rng_[1] + 1) * (2 * rng_[2] + 1)
        for ns in VQ_NSAMPLE:
            r = vq_reference(rng_, ns)
            assert r['mask'].any() and not r['mask'].all()                                                  # empty queries, and others
            if cells > ns and r['members'][VQ_ANCHOR] == ns:
                assert (r['members'] > ns).any()                                                            # over-full beside exactly full
                full_for.add(ns)
            if ns > 1 and cells > 1:
                assert ((r['members'] > 0) & (r['members'] < ns)).any()                                     # a padded tail
    assert full_for == set(VQ_NSAMPLE)                                # every nsample has its exactly full and its over-full query


VQ_LATTICE_RANGE, VQ_LATTICE_NSAMPLE = (2, 3, 4), 33


@functools.lru_cache(maxsize=None)
def vq_lattice():
    """every cell of the (5, 12, 10) grid of sample 0 holds a point at INTEGER coordinates (x, y, z) = its cell; queries at integer
    positions with the same cell.  At radius 3 the rows at offsets (3, 0, 0), (0, 3, 0), (2, 2, 1), ... lie at d2 == 9 exactly and are
    members (inclusive)."""
    rng = np.random.default_rng(5)
    Z, Y, X = VQ_SHAPE
    cells = np.stack(np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing='ij'), -1).reshape(-1, 3)
    coors = np.concatenate([np.zeros((len(cells), 1), np.int64), cells], 1)
    coors = coors[rng.permutation(len(coors))]
    xyz = coors[:, [3, 2, 1]].astype(F)
    qc = np.asarray([(0, 2, 6, 5), (0, 0, 0, 0), (0, 4, 11, 9), (0, 2, 3, 4), (0, 1, 8, 2), (0, 3, 5, 7)], np.int32)
    new_xyz = qc[:, [3, 2, 1]].astype(F)
    counts = np.asarray((len(qc), 0), np.int32)
    assert np.array_equal(vq_ref.coords_ref(new_xyz, counts, VQ_VOXEL_SIZE, VQ_PC_RANGE, 1), qc)
    return dict(coors=coors, xyz=xyz, new_xyz=new_xyz, counts=counts, new_coords=qc, table=vq_ref.table_ref(coors, VQ_SHAPE, VQ_B))


@functools.lru_cache(maxsize=None)
def vq_lattice_reference(nsample=VQ_LATTICE_NSAMPLE):
    s = vq_lattice()
    return vq_ref.query_ref(s['xyz'], s['new_xyz'], s['new_coords'], s['table'], VQ_LATTICE_RANGE, LATTICE_RADIUS, nsample)


def _assert_vq_lattice():
    s = vq_lattice()
    r2 = F(LATTICE_RADIUS) * F(LATTICE_RADIUS)
    wide = vq_lattice_reference(1024)                                  # uncapped: every member of every query
    for m, q in enumerate(s['new_xyz']):
        rows = wide['idx'][m, :wide['cnt'][m]]
        d2 = vsa_ref.dist2(q, s['xyz'][rows])
        assert (d2 == r2).any() and (d2 <= r2).all()                   # members ON the sphere: a strict test would lose them
    first = vq_lattice_reference()
    rows = first['idx'][0, :first['cnt'][0]]
    assert (vsa_ref.dist2(s['new_xyz'][0], s['xyz'][rows]) == r2).any()   # ... also among the first nsample the test compares


# ------------------------------------------------------------------------------------------------ dynamic scatter

SC_GRID = (40, 40, 2)
SC_CLOUDS = {'n3000': 3000, 'n5': 5}
SC_C = (1, 9, 32, 33)
SC_REDUCE = ('sum', 'mean', 'max')


@functools.lru_cache(maxsize=None)
def sc_coors(name):
    """(N, 3) int32 on the (40, 40, 2) grid; 3 % of the rows (at least one) hold a negative coordinate and are dropped"""
    n = SC_CLOUDS[name]
    rng = np.random.default_rng(11 + n)
    coors = np.stack([rng.integers(0, g, n) for g in SC_GRID], 1).astype(np.int32)
    bad = rng.choice(n, max(1, int(round(0.03 * n))), replace=False)
    coors[bad, rng.integers(0, 3, len(bad))] = -rng.integers(1, 4, len(bad)).astype(np.int32)
    if n == 5:
        coors[3] = coors[0]                                         # a voxel of two points beside voxels of one
    return _frozen(coors)


@functools.lru_cache(maxsize=None)
def sc_index(name):
    """the numpy oracle's (voxel_coors, point2voxel_map, voxel_points_count)"""
    from oracle import voxel_oracle
    return _frozen(*voxel_oracle.scatter_index(sc_coors(name)))


@functools.lru_cache(maxsize=None)
def sc_feats(name, c, integer):
    """integer: |v| <= 8, so every sum is exact in fp32, and rows planted EQUAL to a voxel-mate's (tied maxima in every column)"""
    n = SC_CLOUDS[name]
    rng = np.random.default_rng(7 * n + c)
    f = rng.integers(-8, 9, (n, c)).astype(F) if integer else rng.standard_normal((n, c)).astype(F)
    if integer:
        _, pmap, _ = sc_index(name)
        order = np.argsort(pmap, kind='stable')
        mates = [(a, b) for a, b in zip(order[:-1], order[1:]) if pmap[a] == pmap[b] and pmap[a] >= 0]
        for a, b in mates[::2][:40]:
            f[b] = f[a]
    return _frozen(f)


@functools.lru_cache(maxsize=None)
def sc_grad(name, c):
    v = len(sc_index(name)[2])
    return _frozen(np.random.default_rng(3 * c + v).integers(-4, 5, (v, c)).astype(F))


def _assert_sc():
    for name, n in SC_CLOUDS.items():
        coors = sc_coors(name)
        vox, pmap, cnt = sc_index(name)
        dropped = (coors < 0).any(1)
        assert dropped.any() and np.array_equal(pmap < 0, dropped) and cnt.max() >= 2 and cnt.min() == 1
        if n == 3000:
            assert abs(dropped.mean() - 0.03) < 0.005
        for c in SC_C:
            f = sc_feats(name, c, True)
            assert np.abs(f).max() <= 8
            top = np.full((len(cnt), c), -np.inf, F)
            np.maximum.at(top, pmap[~dropped], f[~dropped])
            at_top = np.zeros((len(cnt), c), np.int64)
            np.add.at(at_top, pmap[~dropped], (f[~dropped] == top[pmap[~dropped]]).astype(np.int64))
            assert (at_top >= 2).any(), (name, c)                       # equal maxima: the max backward has a choice to make


_assert_bq()
_assert_bq_lattice()
_assert_fps()
_assert_fps_tied()
_assert_vq()
_assert_vq_lattice()
_assert_sc()
