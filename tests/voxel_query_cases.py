"""The cases of the voxel query tests, shared by tests/test_cpu_voxel_query.py (the `_cpu` twins) and tests/test_gpu_voxel_query.py (the
kernels): scenes, the calls made on them, their expected outputs from tests/voxel_query_ref.py (computed once, never changed) and the
checks both files run on a device of their choice.  Every comparison is an EXACT equality: the outputs are integers, copies and one
fp32 subtraction.

A case is a scene and one or more calls (max_range, radius, nsample).  `_assert_case` holds every case to: at least one empty, one
partly filled and one full query.  A window of ONE cell holds 0 or 1 member, so no single nsample gives it both a partly filled and a
full query: that case makes two calls (nsample 1 and 5), and the three kinds are counted over the case's calls.
"""
import functools

import numpy as np
import torch

import voxel_query_ref as ref

F = np.float32


class Scene:
    def __init__(self, B, shape, coors, xyz, new_xyz, new_coords, counts):
        self.B, self.shape = B, shape
        self.coors, self.xyz, self.new_xyz, self.new_coords = coors, xyz, new_xyz, new_coords
        self.counts = counts                                     # queries per sample (the stacked prefix of new_xyz)
        self.table = ref.table_ref(coors, shape, B)
        self.skey, self.srow = ref.index_ref(coors, shape, B)


def _cells(rng, shape, fill, forced):
    Z, Y, X = shape
    take = rng.random((Z, Y, X)) < fill
    for c in forced:
        take[c] = True
    return np.argwhere(take)


@functools.lru_cache(maxsize=None)
def base_scene():
    """B = 4 on a (5, 12, 14) grid: sample 0 densely filled, sample 1 WITHOUT voxels, sample 2 sparse, sample 3 medium and WITHOUT
    queries.  Voxels sit in the last cells of a y row, of a plane and of sample 2 and in the first cells of the next (no window may
    see them across the edge); rows are shuffled; some cells hold several rows (the lowest wins), some rows are -1 or past the grid
    (with points that WOULD be members), one point is NaN.  Queries: every corner cell, cells up to `range` outside the grid on each
    side (partly in and wholly out), b = -1 and b = B; M is not a multiple of the four queries of a workgroup."""
    rng = np.random.default_rng(20240611)
    B, shape = 4, (5, 12, 14)
    Z, Y, X = shape
    edge = [(0, 0, X - 1), (0, 1, 0), (0, Y - 1, X - 1), (1, 0, 0), (Z - 1, Y - 1, X - 1), (0, 0, 0)]
    rows = []
    for b, fill in enumerate((0.6, 0.0, 0.12, 0.35)):
        if fill > 0:
            rows += [(b, z, y, x) for z, y, x in _cells(rng, shape, fill, edge)]
    rows = np.array(rows, dtype=np.int64)
    dup = rows[rng.choice(len(rows), 12, replace=False)]         # several rows in one cell
    bad = np.array([[-1, -1, -1, -1]] * 4 + [[B, 0, 0, 0], [0, Z, 3, 3], [0, 2, -1, 3], [2, 2, 3, X], [0, 2, Y, 0]], dtype=np.int64)
    coors = np.concatenate([rows, dup, bad])
    coors = coors[rng.permutation(len(coors))]
    xyz = (coors[:, [3, 2, 1]] + 0.5 + rng.uniform(-0.45, 0.45, (len(coors), 3))).astype(F)
    live = np.nonzero(ref.cell_keys(coors, shape, B) < B * Z * Y * X)[0]
    xyz[live[7], 0] = np.nan                                     # a member of nothing
    cells, counts = [], []
    for b, n_rand in ((0, 150), (1, 20), (2, 120)):
        c = [(z, y, x) for z in (0, Z - 1) for y in (0, Y - 1) for x in (0, X - 1)]            # every corner cell
        c += [tuple(v) for v in np.stack([rng.integers(0, Z, n_rand), rng.integers(0, Y, n_rand), rng.integers(0, X, n_rand)], 1)]
        for r in (1, 2, 3, 4, 6, 10):                            # up to `range` outside on each side: partly in (r), wholly out (r + 1)
            for d in (r, r + 1):
                c += [(-d, 5, 6), (Z - 1 + d, 5, 6), (2, -d, 6), (2, Y - 1 + d, 6), (2, 5, -d), (2, 5, X - 1 + d)]
        cells += [(b,) + tuple(int(v) for v in k) for k in c]
        counts.append(len(c))
    counts += [0]                                                # sample 3: no queries
    cells += [(-1, 2, 5, 6), (B, 2, 5, 6), (-1, 0, 0, 0)]        # outside every sample (rows past the counts' sum)
    if len(cells) % 4 == 0:
        cells.append((B + 3, 1, 1, 1))
    new_coords = np.array(cells, dtype=np.int32)
    new_xyz = (new_coords[:, [3, 2, 1]] + 0.5 + rng.uniform(-0.5, 0.5, (len(cells), 3))).astype(F)
    return Scene(B, shape, coors, xyz, new_xyz, new_coords, counts)


@functools.lru_cache(maxsize=None)
def big_scene():
    """nsample = 1024 needs more than 1024 cells in one window: B = 2 on (9, 12, 14) = 1512 cells, sample 0 filled to 90 %."""
    rng = np.random.default_rng(7)
    B, shape = 2, (9, 12, 14)
    Z, Y, X = shape
    rows = np.array([(0, z, y, x) for z, y, x in _cells(rng, shape, 0.9, [])] + [(1, z, y, x) for z, y, x in _cells(rng, shape, 0.05, [])])
    coors = rows[rng.permutation(len(rows))]
    xyz = (coors[:, [3, 2, 1]] + 0.5 + rng.uniform(-0.45, 0.45, (len(coors), 3))).astype(F)
    cells = [(0, 4, 6, 7), (0, 4, 5, 6), (0, 0, 0, 0), (0, Z - 1, Y - 1, X - 1), (0, 4, 0, 7), (1, 4, 6, 7), (1, 0, 0, 0), (-1, 4, 6, 7), (2, 4, 6, 7)]
    new_coords = np.array(cells, dtype=np.int32)
    new_xyz = (new_coords[:, [3, 2, 1]] + 0.5).astype(F)
    return Scene(B, shape, coors, xyz, new_xyz, new_coords, [5, 2])


@functools.lru_cache(maxsize=None)
def integer_scene():
    """Integer coordinates, radius 5: the points at an offset of (3, 4, 0) and its kin lie at d2 == radius2 EXACTLY — members here
    (inclusive), none through `ball_query` (strict), which tests/test_*_voxel_query.py check on the same points."""
    B, shape = 1, (5, 40, 40)
    q_cells = [(2, 10, 10), (2, 30, 30), (2, 10, 30)]            # full (5 members for nsample 3), partly filled (2), empty
    pts = [(2, 10 + 4, 10 + 3), (2, 10 - 4, 10 + 3), (2, 10 + 3, 10 - 4), (2, 10 - 5, 10), (2, 10, 10 + 5),   # around query 0, all at distance 5
           (2, 30 + 5, 30), (2, 30 - 3, 30 + 4)]                                                                # around query 1
    coors = np.array([(0,) + p for p in pts], dtype=np.int64)
    xyz = coors[:, [3, 2, 1]].astype(F)
    new_coords = np.array([(0,) + c for c in q_cells], dtype=np.int32)
    new_xyz = new_coords[:, [3, 2, 1]].astype(F)
    return Scene(B, shape, coors, xyz, new_xyz, new_coords, [3])


# name -> (scene, [(max_range, radius, nsample), ...], what the case must also contain)
CASES = {
    'w1': (base_scene, [((0, 0, 0), 0.9, 1), ((0, 0, 0), 0.9, 5), ((0, 0, 0), 1e-3, 5)], 'below'),   # 1 cell; a radius below every distance
    'w27': (base_scene, [((1, 1, 1), 1.2, 5)], None),
    'w63': (base_scene, [((1, 1, 3), 2.5, 16)], None),                 # 63 cells: one short of a step
    'w65': (base_scene, [((0, 2, 6), 3.0, 16)], None),                 # 65 cells: one past a step
    'w125': (base_scene, [((2, 2, 2), 2.6, 32)], 'cell_step'),         # the 32nd member lies either side of the 64-cell step
    'w729': (base_scene, [((4, 4, 4), 3.0, 32)], None),
    'rows63': (base_scene, [((1, 10, 1), 4.0, 16)], None),             # 63 window rows
    'rows65': (base_scene, [((2, 6, 1), 4.0, 16)], None),              # 65 window rows
    'steps': (base_scene, [((2, 10, 2), 100.0, 16)], 'row_step'),      # 105 window rows: the 16th member lies either side of row 64
    'thresh': (base_scene, [((1, 1, 1), 100.0, 16)], 'around'),        # member counts 15, 16 and 17
    'ns1024': (big_scene, [((4, 6, 7), 100.0, 1024)], None),
    'inclusive': (integer_scene, [((0, 5, 5), 5.0, 3)], 'exact'),
}


def _assert_case(name, scene, calls, extra, results):
    """Every case: an empty, a partly filled and a full query, counted over its calls; plus what `extra` names."""
    kinds = set()
    for (rng_, radius, nsample), r in zip(calls, results):
        kinds |= {'empty'} if (r['members'] == 0).any() else set()
        kinds |= {'partial'} if ((r['members'] > 0) & (r['members'] < nsample)).any() else set()
        kinds |= {'full'} if (r['members'] >= nsample).any() else set()
    assert kinds == {'empty', 'partial', 'full'}, (name, kinds)
    r, nsample = results[0], calls[0][2]
    if extra == 'below':
        assert (results[2]['members'] == 0).all()
    if extra == 'cell_step':
        assert ((r['pos_cell'] >= 0) & (r['pos_cell'] < 64)).any() and (r['pos_cell'] >= 64).any(), name
    if extra == 'row_step':
        assert ((r['pos_row'] >= 0) & (r['pos_row'] < 64)).any() and (r['pos_row'] >= 64).any(), name
    if extra == 'around':
        assert {nsample - 1, nsample, nsample + 1} <= set(r['members'].tolist()), name
    if extra == 'exact':
        assert r['members'].tolist() == [5, 2, 0], name


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (scene, calls, expected results): the numpy restatement, computed once and shared by every test."""
    make, calls, extra = CASES[name]
    scene = make()
    results = [ref.query_ref(scene.xyz, scene.new_xyz, scene.new_coords, scene.table, rng_, radius, nsample) for rng_, radius, nsample in calls]
    _assert_case(name, scene, calls, extra, results)
    return scene, calls, results


def t(a, dev, dtype=None):
    x = torch.from_numpy(np.ascontiguousarray(a))
    return (x if dtype is None else x.to(dtype)).to(dev)


def same(got, want, what):
    """bit for bit (NaN payloads included: the grouped xyz of nothing is never NaN, a copied feature may be anything)"""
    got = got.detach().cpu().numpy()
    want = np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert got.tobytes() == want.tobytes(), (what, np.argwhere(np.atleast_1d(got != want))[:5].tolist())


def lookups(amd, scene, dev, coors_dtype):
    """-> {'sorted': VoxelQueryIndex, 'dense': table}, each checked against the restatement."""
    coors = t(scene.coors, dev, coors_dtype)
    index = amd.voxel_query_index(coors, scene.shape, scene.B)
    same(index.skey, scene.skey, 'skey')
    same(index.srow, scene.srow, 'srow')
    table = amd.voxel_point_indices(coors, scene.shape, scene.B)
    same(table, scene.table, 'table')
    return {'sorted': index, 'dense': table}


def check_query_case(amd, name, dev, coors_dtype):
    """idx, cnt and the mask of every call of the case, in both look-up forms."""
    scene, calls, results = case(name)
    look = lookups(amd, scene, dev, coors_dtype)
    xyz, q, nc = t(scene.xyz, dev), t(scene.new_xyz, dev), t(scene.new_coords, dev)
    for (rng_, radius, nsample), want in zip(calls, results):
        for form, index in look.items():
            idx, mask, cnt = amd.voxel_query(rng_, radius, nsample, xyz, q, nc, index, return_cnt=True)
            same(idx, want['idx'], (name, form, 'idx'))
            same(cnt, want['cnt'], (name, form, 'cnt'))
            same(mask, want['mask'], (name, form, 'mask'))


def check_group_case(amd, name, dev, C, use_xyz, call=0):
    """the grouped block (and idx) of one call, in both look-up forms; C == 0: no features"""
    scene, calls, results = case(name)
    rng_, radius, nsample = calls[call]
    want = results[call]
    feats = np.random.default_rng(C).standard_normal((len(scene.xyz), C)).astype(F) if C > 0 else None
    block = ref.group_ref(scene.xyz, scene.new_xyz, feats, want['idx'], want['cnt'], use_xyz)
    coors = t(scene.coors, dev, torch.int32)
    xyz, q, nc = t(scene.xyz, dev), t(scene.new_xyz, dev), t(scene.new_coords, dev)
    mod = amd.VoxelQueryAndGroup(rng_, radius, nsample, use_xyz=use_xyz)
    for form, index in (('sorted', amd.voxel_query_index(coors, scene.shape, scene.B)), ('dense', amd.voxel_point_indices(coors, scene.shape, scene.B))):
        out, idx = mod(xyz, q, nc, index, t(feats, dev) if C > 0 else None)
        same(idx, want['idx'], (name, form, 'idx'))
        same(out, block, (name, form, C, use_xyz, 'new_features'))


# ---- voxel_query_coords -------------------------------------------------------------------------------------------------------------
def coords_cases():
    """-> [(new_xyz, counts, voxel_size, pc_range, scale)]: points on cell faces, one ulp below hi, lo = -4 / hi = 4 (the case of
    hard_voxelize's notes), NaN, inf and 1e30, rows past the counts' sum, a negative count."""
    rng = np.random.default_rng(3)
    vs, rg = (0.05, 0.05, 0.1), (0.0, -40.0, -3.0, 70.4, 40.0, 1.0)
    faces = np.stack([rng.integers(0, 1408, 64) * F(0.05) * 8, rng.integers(-100, 100, 64) * F(0.05) * 8, rng.integers(-4, 4, 64) * F(0.1) * 8], 1)
    pts = np.concatenate([faces.astype(F), rng.uniform((-5, -45, -4), (75, 45, 2), (200, 3)).astype(F),
                          np.array([[np.nextafter(F(70.4), F(0)), np.nextafter(F(40), F(0)), np.nextafter(F(1), F(0))],
                                    [np.nan, 0, 0], [1, np.inf, 0], [1, 1, -np.inf], [1e30, 0, 0], [0, -1e30, 0], [70.4, 40.0, 1.0]], dtype=F)])
    out = [(pts, [100, -5, 120, 30], vs, rg, 8), (pts, [len(pts) + 50], vs, rg, 1), (pts[:5], [0, 0], vs, rg, 2)]
    pts4 = np.concatenate([np.arange(-41, 42, dtype=F)[:, None] * F(0.1) * np.ones(3, dtype=F),
                           np.array([[np.nextafter(F(4), F(0))] * 3, [np.nextafter(F(-4), F(0))] * 3, [4, 4, 4], [-4, -4, -4]], dtype=F)])
    out.append((pts4.astype(F), [40, 47], (0.1, 0.1, 0.1), (-4.0, -4.0, -4.0, 4.0, 4.0, 4.0), 1))
    return out


def check_coords(amd, dev):
    for pts, counts, vs, rg, scale in coords_cases():
        want = ref.coords_ref(pts, counts, vs, rg, scale)
        for cdt in (torch.int32, torch.int64):
            got = amd.voxel_query_coords(t(pts, dev), torch.tensor(counts, dtype=cdt, device=dev), vs, rg, scale)
            same(got, want, 'new_coords')
    assert (ref.coords_ref(*coords_cases()[0])[:, 0] == -1).sum() >= 5           # NaN, inf, 1e30 and the rows past the counts' sum


# ---- a caller's dense table -----------------------------------------------------------------------------------------------------------
def check_garbage_table(amd, dev):
    """entries >= N and negative entries other than -1: skipped, like an empty cell"""
    scene, calls, _ = case('w125')
    rng_, radius, nsample = calls[0]
    table = scene.table.copy()
    flat = table.reshape(-1)
    N = len(scene.xyz)
    hit = np.nonzero(flat >= 0)[0][::7]
    flat[hit] = np.resize(np.array([N, N + 5, -7, np.iinfo(np.int32).min, np.iinfo(np.int32).max], dtype=np.int32), len(hit))
    want = ref.query_ref(scene.xyz, scene.new_xyz, scene.new_coords, table, rng_, radius, nsample)
    assert (want['cnt'] > 0).any()
    idx, mask, cnt = amd.voxel_query(rng_, radius, nsample, t(scene.xyz, dev), t(scene.new_xyz, dev), t(scene.new_coords, dev), t(table, dev),
                                     return_cnt=True)
    same(idx, want['idx'], 'idx')
    same(cnt, want['cnt'], 'cnt')
    same(mask, want['mask'], 'mask')


# ---- against ball_query ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ball_scene():
    """Clean stacked data (rows sorted by sample, one row per cell, no NaN) on unit cells; radius 1.7 -> range 2 covers the ball;
    nsample 128 >= the 125 cells of a window.  Asserted here with the restatement: no point lies at d2 == radius2."""
    rng = np.random.default_rng(11)
    B, shape = 3, (5, 12, 14)
    rows = np.array([(b, z, y, x) for b, fill in enumerate((0.5, 0.0, 0.2)) for z, y, x in _cells(rng, shape, fill, [])])
    xyz = (rows[:, [3, 2, 1]] + 0.5 + rng.uniform(-0.45, 0.45, (len(rows), 3))).astype(F)
    xyz_cnt = [int((rows[:, 0] == b).sum()) for b in range(B)]
    q_cnt = [90, 10, 61]
    qb = np.repeat(np.arange(B), q_cnt)
    new_xyz = rng.uniform((0, 0, 0), (14, 12, 5), (len(qb), 3)).astype(F)
    new_coords = np.concatenate([qb[:, None], np.floor(new_xyz[:, [2, 1, 0]]).astype(np.int64)], 1).astype(np.int32)
    radius = 1.7
    r2 = F(radius) * F(radius)
    start = np.concatenate([[0], np.cumsum(xyz_cnt)])
    for m in range(len(qb)):
        p = xyz[start[qb[m]]:start[qb[m] + 1]]
        dx, dy, dz = new_xyz[m, 0] - p[:, 0], new_xyz[m, 1] - p[:, 1], new_xyz[m, 2] - p[:, 2]
        assert not (((dx * dx + dy * dy) + dz * dz) == r2).any()
    return Scene(B, shape, rows, xyz, new_xyz, new_coords, q_cnt), xyz_cnt, radius


def check_against_ball_query(amd, dev):
    scene, xyz_cnt, radius = ball_scene()
    nsample = 128
    xyz, q, nc = t(scene.xyz, dev), t(scene.new_xyz, dev), t(scene.new_coords, dev)
    index = amd.voxel_query_index(t(scene.coors, dev, torch.int32), scene.shape, scene.B)
    idx, mask, cnt = amd.voxel_query((2, 2, 2), radius, nsample, xyz, q, nc, index, return_cnt=True)
    bidx, bmask, bcnt = amd.ball_query(radius, nsample, xyz, torch.tensor(xyz_cnt, dtype=torch.int32, device=dev), q,
                                       torch.tensor(scene.counts, dtype=torch.int32, device=dev), return_cnt=True)
    idx, cnt, bidx, bcnt = idx.cpu().numpy(), cnt.cpu().numpy(), bidx.cpu().numpy(), bcnt.cpu().numpy()
    assert (cnt == bcnt).all() and cnt.max() < nsample and (cnt > 0).any() and (cnt == 0).any()
    start = np.concatenate([[0], np.cumsum(xyz_cnt)])
    for m in range(len(cnt)):
        assert set(idx[m, :cnt[m]].tolist()) == set((bidx[m, :bcnt[m]] + start[scene.new_coords[m, 0]]).tolist()), m
    assert torch.equal(mask.cpu(), bmask.cpu())


def check_inclusive_vs_ball_query(amd, dev):
    scene, calls, results = case('inclusive')
    rng_, radius, nsample = calls[0]
    xyz, q = t(scene.xyz, dev), t(scene.new_xyz, dev)
    one = lambda n: torch.tensor([n], dtype=torch.int32, device=dev)
    _, bmask = amd.ball_query(radius, nsample, xyz, one(len(scene.xyz)), q, one(len(scene.new_xyz)))
    assert bmask.all()                                                     # strict: the same points give none
    _, mask = amd.voxel_query(rng_, radius, nsample, xyz, q, t(scene.new_coords, dev), t(scene.table, dev))
    assert mask.cpu().tolist() == [False, False, True]


# ---- the C entries on sentinel-filled outputs -----------------------------------------------------------------------------------------
GUARD = 64


def _guarded(shape, dtype, dev):
    n = int(np.prod(shape))
    sent = {torch.int32: 0x5A5A5A5A, torch.int64: 0x5A5A5A5A5A5A5A5A, torch.uint8: 0x5A, torch.float32: -1.2345e33}[dtype]
    buf = torch.full((n + 2 * GUARD,), sent, dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + n].view(shape), sent


def check_entries_write_everything_and_nothing_else(amd, dev):
    """every element of every output is written (the sentinel is a value no output can take) and the guard bands either side stay"""
    import ctypes
    from mmdet3d_gaussian_amd import _host
    scene, calls, results = case('w63')
    rng_, radius, nsample = calls[0]
    want = results[0]
    N, M, C = len(scene.xyz), len(scene.new_xyz), 5
    B, (Z, Y, X) = scene.B, scene.shape
    feats = np.random.default_rng(1).standard_normal((N, C)).astype(F)
    coors, xyz, q, f = t(scene.coors, dev, torch.int32), t(scene.xyz, dev), t(scene.new_xyz, dev), t(feats, dev)
    bufs = {k: _guarded(s, d, dev) for k, (s, d) in dict(
        skey=((N,), torch.int64), srow=((N,), torch.int32), table=((B, Z, Y, X), torch.int32), coords=((M, 4), torch.int32),
        idx=((M, nsample), torch.int32), cnt=((M,), torch.int32), mask=((M,), torch.uint8), out=((M, 3 + C, nsample), torch.float32)).items()}
    p = lambda k: bufs[k][1].data_ptr()
    lib = amd.load_library()
    work = torch.empty(lib.gd3d_vsa_voxel_index_workspace_bytes(N), dtype=torch.uint8, device=dev) if dev.type == 'cuda' else None
    _host.call('gd3d_vsa_voxel_index', dev, (coors.data_ptr(), 0, N, B, Z, Y, X, _host.ptr(work), p('skey'), p('srow')))
    _host.call('gd3d_vsa_voxel_table', dev, (coors.data_ptr(), 0, N, B, Z, Y, X, p('table')))
    f3 = ctypes.c_float * 3
    qc = torch.tensor(scene.counts, dtype=torch.int32, device=dev)
    _host.call('gd3d_vsa_voxel_coords', dev, (q.data_ptr(), qc.data_ptr(), len(scene.counts), M, f3(1, 1, 1), f3(0, 0, 0), p('coords')))
    nc = t(scene.new_coords, dev)
    r3 = (ctypes.c_int32 * 3)(*rng_)
    _host.call('gd3d_vsa_voxel_query_and_group', dev,
               (xyz.data_ptr(), q.data_ptr(), nc.data_ptr(), p('skey'), p('srow'), None, f.data_ptr(), B, Z, Y, X, N, M, C, r3, radius, nsample,
                1, p('out'), p('idx'), p('cnt'), p('mask')), (0,))
    block = ref.group_ref(scene.xyz, scene.new_xyz, feats, want['idx'], want['cnt'], True)
    for k, expect in dict(skey=scene.skey, srow=scene.srow, table=scene.table, idx=want['idx'], cnt=want['cnt'],
                          mask=want['mask'].astype(np.uint8), out=block).items():
        same(bufs[k][1], expect, k)
    same(bufs['coords'][1], ref.coords_ref(scene.new_xyz, scene.counts, (1, 1, 1), (0, 0, 0), 1), 'coords')
    for k in ('idx', 'cnt', 'mask'):                                       # the stand-alone query through the dense table, same buffers
        bufs[k][1].fill_(bufs[k][2])
    _host.call('gd3d_vsa_voxel_query', dev,
               (xyz.data_ptr(), q.data_ptr(), nc.data_ptr(), None, None, p('table'), B, Z, Y, X, N, M, r3, radius, nsample, p('idx'), p('cnt'),
                p('mask')), (0,))
    same(bufs['idx'][1], want['idx'], 'idx')
    same(bufs['cnt'][1], want['cnt'], 'cnt')
    for k, (buf, view, sent) in bufs.items():
        guard = torch.cat([buf[:GUARD], buf[-GUARD:]])
        assert (guard == sent).all(), f'{k}: a guard band was written'


# ---- backward -------------------------------------------------------------------------------------------------------------------------
def check_backward(amd, dev):
    scene, calls, results = case('w125')
    rng_, radius, nsample = calls[0]
    want = results[0]
    N, M, C = len(scene.xyz), len(scene.new_xyz), 7
    rng = np.random.default_rng(5)
    xyz, q, nc = t(scene.xyz, dev), t(scene.new_xyz, dev), t(scene.new_coords, dev)
    index = amd.voxel_query_index(t(scene.coors, dev, torch.int32), scene.shape, scene.B)
    for use_xyz in (True, False):
        c_off = 3 if use_xyz else 0
        mod = amd.VoxelQueryAndGroup(rng_, radius, nsample, use_xyz=use_xyz)
        for integer in (True, False):
            g = (rng.integers(-8, 9, (M, c_off + C, nsample)) if integer else rng.standard_normal((M, c_off + C, nsample))).astype(F)
            feats = t(rng.standard_normal((N, C)).astype(F), dev).requires_grad_(True)
            out, _ = mod(xyz, q, nc, index, feats)
            out.backward(t(g, dev))
            got = feats.grad.cpu().numpy().astype(np.float64)
            total, mag, k = ref.backward_ref(g, want['idx'], want['cnt'], N, C, c_off)
            assert k.max() >= 8 and (k == 1).any()                                     # rows that many queries share, rows of one
            if integer:
                assert (got == total).all()                                            # exact in any order
            else:
                bound = np.maximum(k - 1, 0) * 2.0 ** -24 * mag                        # an fp32 sum of k terms in any order
                print('backward: worst error / bound', float(np.max(np.abs(got - total) / np.maximum(bound, 1e-300))))
                assert (np.abs(got - total) <= bound).all()


def check_empty_sizes(amd, dev):
    scene, calls, _ = case('w27')
    rng_, radius, nsample = calls[0]
    xyz, q, nc = t(scene.xyz, dev), t(scene.new_xyz, dev), t(scene.new_coords, dev)
    index = amd.voxel_query_index(t(scene.coors, dev, torch.int32), scene.shape, scene.B)
    idx, mask, cnt = amd.voxel_query(rng_, radius, nsample, xyz, q[:0], nc[:0], index, return_cnt=True)            # M = 0
    assert idx.shape == (0, nsample) and mask.shape == (0,) and cnt.shape == (0,)
    out, idx = amd.VoxelQueryAndGroup(rng_, radius, nsample)(xyz, q[:0], nc[:0], index, torch.zeros(len(scene.xyz), 4, device=dev))
    assert out.shape == (0, 7, nsample) and idx.shape == (0, nsample)
    none = torch.zeros((0, 4), dtype=torch.int32, device=dev)                                                       # N = 0
    empty = amd.voxel_query_index(none, scene.shape, scene.B)
    assert empty.skey.shape == (0,) and empty.srow.shape == (0,)
    table = amd.voxel_point_indices(none, scene.shape, scene.B)
    assert (table == -1).all()
    assert amd.voxel_query_coords(q[:0], torch.tensor(scene.counts, device=dev), (1, 1, 1), (0, 0, 0, 1, 1, 1)).shape == (0, 4)
    for look in (empty, table):
        out, idx = amd.VoxelQueryAndGroup(rng_, radius, nsample)(xyz[:0], q, nc, look, torch.zeros(0, 4, device=dev))
        assert not out.any() and not idx.any() and out.shape == (len(scene.new_xyz), 7, nsample)
        _, mask = amd.voxel_query(rng_, radius, nsample, xyz[:0], q, nc, look)
        assert mask.all()


def check_argument_errors(amd, dev):
    """every refusal raises RuntimeError before any output exists"""
    import pytest
    scene, calls, _ = case('w27')
    xyz, q, nc = t(scene.xyz, dev), t(scene.new_xyz, dev), t(scene.new_coords, dev)
    coors = t(scene.coors, dev, torch.int32)
    index = amd.voxel_query_index(coors, scene.shape, scene.B)
    table = amd.voxel_point_indices(coors, scene.shape, scene.B)
    bad = [
        lambda: amd.voxel_query((1, 1, 1), 1.0, 0, xyz, q, nc, index),                       # the nsample limit
        lambda: amd.voxel_query((1, 1, 1), 1.0, 1025, xyz, q, nc, index),
        lambda: amd.voxel_query((1, 17, 1), 1.0, 4, xyz, q, nc, index),                      # the range limit
        lambda: amd.voxel_query((1, -1, 1), 1.0, 4, xyz, q, nc, index),
        lambda: amd.voxel_query((1, 1), 1.0, 4, xyz, q, nc, index),
        lambda: amd.voxel_query((1, 1, 1), 1.0, 4, xyz[:, :2], q, nc, index),                # shapes
        lambda: amd.voxel_query((1, 1, 1), 1.0, 4, xyz, q, nc[:-1], index),
        lambda: amd.voxel_query((1, 1, 1), 1.0, 4, xyz, q, nc[:, :3], index),
        lambda: amd.voxel_query((1, 1, 1), 1.0, 4, xyz[:-1], q, nc, index),                  # the index has one entry per row of xyz
        lambda: amd.voxel_query((1, 1, 1), 1.0, 4, xyz, q, nc, table[0]),
        lambda: amd.voxel_query((1, 1, 1), 1.0, 4, xyz, q, nc, None),
        lambda: amd.voxel_query((1, 1, 1), 1.0, 4, xyz.long(), q, nc, index),                # dtypes
        lambda: amd.voxel_query((1, 1, 1), 1.0, 4, xyz, q, nc.float(), index),
        lambda: amd.voxel_query((1, 1, 1), 1.0, 4, xyz, q, nc, table.long()),
        lambda: amd.voxel_query_index(coors.float(), scene.shape, scene.B),
        lambda: amd.voxel_query_index(coors[:, :3], scene.shape, scene.B),
        lambda: amd.voxel_query_index(coors, (5, 12), scene.B),
        lambda: amd.voxel_point_indices(coors, (5, 0, 14), scene.B),
        lambda: amd.voxel_query_coords(q, torch.tensor([1.0], device=dev), (1, 1, 1), (0, 0, 0, 1, 1, 1)),
        lambda: amd.voxel_query_coords(q, torch.tensor([1], device=dev), (1, 0, 1), (0, 0, 0, 1, 1, 1)),
        lambda: amd.VoxelQueryAndGroup((1, 1, 1), 1.0, 4, use_xyz=False)(xyz, q, nc, index, None),      # nothing to group
        lambda: amd.VoxelQueryAndGroup((1, 1, 1), 1.0, 4)(xyz, q, nc, index, torch.zeros(len(scene.xyz) - 1, 3, device=dev)),
        lambda: amd.VoxelQueryAndGroup((1, 1, 1), 1.0, 4)(xyz, q, nc, index, torch.zeros(len(scene.xyz), 0, device=dev)),
        lambda: amd.VoxelQueryAndGroup((1, 1, 40), 1.0, 4),
        lambda: amd.VoxelQueryAndGroup((1, 1, 1), 1.0, 2000),
    ]
    if dev.type == 'cuda':                                                                   # device mismatch
        bad += [lambda: amd.voxel_query((1, 1, 1), 1.0, 4, xyz.cpu(), q, nc, index),
                lambda: amd.voxel_query((1, 1, 1), 1.0, 4, xyz, q, nc.cpu(), index),
                lambda: amd.voxel_query((1, 1, 1), 1.0, 4, xyz, q, nc, table.cpu()),
                lambda: amd.voxel_query((1, 1, 1), 1.0, 4, xyz, q, nc, amd.VoxelQueryIndex(index.skey.cpu(), index.srow.cpu(), *index[2:])),
                lambda: amd.VoxelQueryAndGroup((1, 1, 1), 1.0, 4)(xyz, q, nc, index, torch.zeros(len(scene.xyz), 3))]
    for k, f in enumerate(bad):
        with pytest.raises(RuntimeError):
            f()
            raise AssertionError(f'refusal {k} did not raise')
