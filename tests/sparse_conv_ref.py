"""Reference side of the sparse 3D convolution tests (include/gd3d.h, gd3d_sparse_conv_*).

* `index_ref`   the numpy restatement of the index rules, vectorised: int64 keys, a stable argsort, `searchsorted`, `np.unique`.
* `oracle`      the fp64 oracle: densify, `F.conv3d` in fp64 on the CPU, read at `out_coors`; autograd through it gives the gradients.
                Run a second time on |X|, |W|, |bias|, |gY| it gives `A`, the scale of the rounding bound.
* `bounds`      a dot product of L terms rounded in fp32 in ANY order satisfies |err| <= gamma_L * sum |x||w|, gamma_L = L u / (1 - L u),
                u = 2^-24; the tests assert |ours - o64| <= (L + 2) u A elementwise with L counted from the restated tables.
* `CASES`       the named cases; tests/test_cpu_sparse_conv.py runs them against the `_cpu` twins, tests/test_gpu_sparse_conv.py on cuda:0.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
TILE_M = 64            # output rows of one workgroup of the forward / input-gradient kernel (csrc/sparse_conv_common.h)

GEOMS = {              # the four layer geometries of the shipped encoders: kernel, stride, padding, subm
    'subm': ((3, 3, 3), (1, 1, 1), (1, 1, 1), True),
    's2p1': ((3, 3, 3), (2, 2, 2), (1, 1, 1), False),
    's2p011': ((3, 3, 3), (2, 2, 2), (0, 1, 1), False),
    'down': ((3, 1, 1), (2, 1, 1), (0, 0, 0), False),
}


def triple(v):
    return tuple(int(x) for x in v) if isinstance(v, (tuple, list)) else (int(v),) * 3


def out_shape_of(shape, kernel, stride, padding):
    return tuple(max(0, (n + 2 * p - k) // s + 1) for n, k, s, p in zip(shape, kernel, stride, padding))   # 0: the kernel does not fit


def offsets_of(kernel):
    kz, ky, kx = kernel
    return np.stack(np.meshgrid(np.arange(kz), np.arange(ky), np.arange(kx), indexing='ij'), -1).reshape(-1, 3).astype(np.int64)   # kz slowest


def active_rows(coors, shape, B):
    c = coors.astype(np.int64)
    return (c >= 0).all(1) & (c[:, 0] < B) & (c[:, 1] < shape[0]) & (c[:, 2] < shape[1]) & (c[:, 3] < shape[2])


def _key(b, zyx, shape):
    return ((b * shape[0] + zyx[..., 0]) * shape[1] + zyx[..., 1]) * shape[2] + zyx[..., 2]


def index_ref(coors, shape, B, kernel, stride, padding, subm, max_out=None):
    """-> dict(out_coors (R, 4) int32, out_shape, nbr (R, K) int32, nbr_t (N, K) int32 or None, num (2,) int64, out_batch_cnt (B,) int32);
    R = N for subm, max_out (None: the true count) otherwise"""
    shape, kernel, stride, padding = triple(shape), triple(kernel), triple(stride), triple(padding)
    coors = np.asarray(coors, np.int32).reshape(-1, 4)
    N, c = len(coors), coors.astype(np.int64)
    off = offsets_of(kernel)
    K = len(off)
    act = active_rows(coors, shape, B)
    rows = np.nonzero(act)[0]
    keys = _key(c[rows, 0], c[rows, 1:], shape)
    order = np.argsort(keys, kind='stable')                              # the lowest row of a duplicated cell comes first
    skey, srow = keys[order], rows[order]
    n_arr, s_arr, p_arr = np.array(shape), np.array(stride), np.array(padding)

    def find(b, zyx, ok):
        """rows at (b, zyx) where ok and inside the grid (checked per axis BEFORE linearising), else -1"""
        ok = ok & ((zyx >= 0) & (zyx < n_arr)).all(-1)
        if len(skey) == 0:
            return np.full(ok.shape, -1, np.int32)
        q = _key(b, np.where(ok[..., None], zyx, 0), shape)
        at = np.minimum(np.searchsorted(skey, q, side='left'), len(skey) - 1)
        return np.where(ok & (skey[at] == q), srow[at], -1).astype(np.int32)

    if subm:
        assert all(k % 2 == 1 for k in kernel) and stride == (1, 1, 1) and padding == tuple(k // 2 for k in kernel)
        zyx = c[:, None, 1:] - p_arr + off[None]
        nbr = find(c[:, None, 0], zyx, np.broadcast_to(act[:, None], (N, K)))
        cnt = np.bincount(c[rows, 0], minlength=B)[:B] if B > 0 else np.zeros(0)
        return dict(out_coors=coors.copy(), out_shape=shape, nbr=nbr.reshape(N, K), nbr_t=None, num=np.array([N, N], np.int64),
                    out_batch_cnt=cnt.astype(np.int32))
    o_shape = out_shape_of(shape, kernel, stride, padding)
    o_arr = np.array(o_shape)
    v = c[:, None, 1:] + p_arr - off[None]                               # (N, K, 3): o * s
    ok = act[:, None] & (v >= 0).all(-1) & (v % s_arr == 0).all(-1) & (v // s_arr < o_arr).all(-1)
    okeys = _key(np.broadcast_to(c[:, None, 0], (N, K)), v // s_arr, o_shape)[ok]
    ukey = np.unique(okeys)                                              # ascending (b, z, y, x)
    total = len(ukey)
    R = total if max_out is None else int(max_out)
    kept = min(total, R)
    ukey = ukey[:kept]
    out_coors = np.full((R, 4), -1, np.int32)
    rest = ukey.copy()
    for a in (3, 2, 1):
        out_coors[:kept, a] = rest % o_shape[a - 1]
        rest //= o_shape[a - 1]
    out_coors[:kept, 0] = rest
    oc = out_coors[:kept].astype(np.int64)
    nbr = np.full((R, K), -1, np.int32)
    nbr[:kept] = find(oc[:, None, 0], oc[:, None, 1:] * s_arr - p_arr + off[None], np.ones((kept, K), bool))
    nbr_t = np.full((N, K), -1, np.int32)
    o_idx, j_idx = np.nonzero(nbr >= 0)
    nbr_t[nbr[o_idx, j_idx], j_idx] = o_idx                              # the transpose, by definition
    cnt = np.bincount(oc[:, 0], minlength=B)[:B] if B > 0 else np.zeros(0)
    return dict(out_coors=out_coors, out_shape=o_shape, nbr=nbr, nbr_t=nbr_t, num=np.array([kept, total], np.int64),
                out_batch_cnt=cnt.astype(np.int32))


def conv3d_at(dense, w5, bias, stride, padding, out_coors, live):
    """dense (B, Cin, D, H, W) -> F.conv3d read at the rows of out_coors where `live`, zeros elsewhere"""
    y = F.conv3d(dense, w5.permute(4, 3, 0, 1, 2), bias, stride=stride, padding=padding)
    oc = torch.from_numpy(np.where(live[:, None], out_coors, 0).astype(np.int64))
    rows = y[oc[:, 0], :, oc[:, 1], oc[:, 2], oc[:, 3]]
    return rows * torch.from_numpy(live.astype(np.float64))[:, None]


def oracle(coors, shape, B, kernel, stride, padding, index, X, W, bias, gY):
    """The fp64 oracle over unique active rows -> dict(out, gx, gw, gb) of fp64 numpy arrays.  X (N, Cin), W (K, Cin, Cout), bias (Cout) or
    None, gY (R, Cout): any float arrays; `index`: the restated tables (which rows are live, where they lie)."""
    shape, kernel, stride, padding = triple(shape), triple(kernel), triple(stride), triple(padding)
    act = active_rows(np.asarray(coors), shape, B)
    c = torch.from_numpy(np.where(act[:, None], coors, 0).astype(np.int64))
    x = torch.tensor(np.asarray(X, np.float64), requires_grad=True)
    w = torch.tensor(np.asarray(W, np.float64), requires_grad=True)
    b = None if bias is None else torch.tensor(np.asarray(bias, np.float64), requires_grad=True)
    a = torch.from_numpy(np.nonzero(act)[0])
    dense = torch.zeros((B,) + shape + (x.shape[1],), dtype=torch.float64).index_put((c[a, 0], c[a, 1], c[a, 2], c[a, 3]), x[a])
    dense = dense.permute(0, 4, 1, 2, 3)
    live = (index['nbr'] >= 0).any(1)
    out = conv3d_at(dense, w.reshape(*kernel, w.shape[1], w.shape[2]), b, stride, padding, index['out_coors'], live)
    grads = torch.autograd.grad(out, [x, w] + ([] if b is None else [b]), torch.from_numpy(np.asarray(gY, np.float64)))
    return dict(out=out.detach().numpy(), gx=grads[0].numpy(), gw=grads[1].numpy(), gb=None if b is None else grads[2].numpy())


def sparse_oracle(index, X, W, bias, gY):
    """The same four quantities in fp64 by gather - matmul - add over the restated tables: for the grid no dense tensor can hold"""
    X, W, gY = np.asarray(X, np.float64), np.asarray(W, np.float64), np.asarray(gY, np.float64)
    nbr = index['nbr']
    live = (nbr >= 0).any(1)
    out, gx, gw = np.zeros((len(nbr), W.shape[2])), np.zeros_like(X), np.zeros_like(W)
    for j in range(W.shape[0]):
        o = np.nonzero(nbr[:, j] >= 0)[0]
        i = nbr[o, j]
        out[o] += X[i] @ W[j]
        np.add.at(gx, i, gY[o] @ W[j].T)
        gw[j] = X[i].T @ gY[o]
    if bias is not None:
        out[live] += np.asarray(bias, np.float64)
    return dict(out=out, gx=gx, gw=gw, gb=None if bias is None else gY[live].sum(0))


def term_counts(index, N, Cin, Cout, has_bias):
    """L per quantity, from the restated tables: forward (R, 1), input gradient (N, 1), weight gradient (K, 1, 1), bias gradient scalar"""
    nbr = index['nbr']
    valid = nbr >= 0
    per_in = np.zeros(N, np.int64)
    np.add.at(per_in, nbr[valid], 1)
    return dict(out=(valid.sum(1) * Cin + int(has_bias))[:, None], gx=(per_in * Cout)[:, None], gw=valid.sum(0)[:, None, None],
                gb=int(valid.any(1).sum()))


def within_bound(got, want, scale, L):
    """-> (elementwise |got - want| <= (L + 2) u scale holds everywhere, the worst |got - want| / scale)"""
    err = np.abs(np.asarray(got, np.float64) - want)
    ok = bool((err <= (L + 2) * U * scale).all())
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(scale > 0, err / scale, 0.0)
    return ok, float(ratio.max()) if ratio.size else 0.0


# ---- the cases -------------------------------------------------------------------------------------------------------------------------

def random_coors(rng, n, shape, B, empty=()):
    """n unique active rows [b, z, y, x] in random order, none in the samples of `empty`"""
    samples = [b for b in range(B) if b not in empty]
    cells = int(np.prod(shape))
    flat = rng.choice(len(samples) * cells, size=n, replace=False)
    b = np.array(samples)[flat // cells]
    cell = flat % cells
    return np.stack([b, cell // (shape[1] * shape[2]), cell // shape[2] % shape[1], cell % shape[2]], 1).astype(np.int32)


def _case(coors, shape, B, geom, cin, cout, bias=True, max_out=None, seed=0, values='dense'):
    kernel, stride, padding, subm = GEOMS[geom] if isinstance(geom, str) else geom
    return dict(coors=np.asarray(coors, np.int32).reshape(-1, 4), shape=tuple(shape), B=B, kernel=kernel, stride=stride, padding=padding, subm=subm,
                cin=cin, cout=cout, bias=bias, max_out=max_out, seed=seed, values=values)


def _make_cases():
    rng = np.random.default_rng(20)
    cases = {}
    pairs = [(4, 16), (5, 16), (16, 16), (16, 32), (64, 64), (128, 128), (3, 7), (16, 32)]
    for n, (geom, shape) in enumerate((g, s) for s in ((9, 12, 10), (7, 11, 13)) for g in GEOMS):
        # B = 3 with the middle sample empty; every channel pair on some geometry
        cases[f'{geom}_{shape[0]}x{shape[1]}x{shape[2]}_c{pairs[n][0]}_{pairs[n][1]}'] = _case(random_coors(rng, 150, shape, 3, empty=(1,)), shape, 3, geom, *pairs[n], seed=n)
    for geom in ('subm', 's2p1'):                                         # row counts around the kernel's row tile
        for name, n in (('rows_0', 0), ('rows_1', 1), ('rows_tile_minus_1', TILE_M - 1), ('rows_tile', TILE_M), ('rows_tile_plus_1', TILE_M + 1),
                        ('rows_2_tiles_plus_1', 2 * TILE_M + 1)):
            cases[f'{geom}_{name}'] = _case(random_coors(rng, n, (9, 12, 10), 2), (9, 12, 10), 2, geom, 16, 16, seed=n)
    shape = (9, 12, 10)
    D, H, W = shape
    corners = [[b, z, y, x] for b in (0, 1) for z in (0, D - 1) for y in (0, H - 1) for x in (0, W - 1)]
    faces = [[0, 0, 5, 5], [0, D - 1, 5, 5], [0, 4, 0, 5], [0, 4, H - 1, 5], [0, 4, 5, 0], [0, 4, 5, W - 1]]
    # x = W-1 beside x = 0 of the next row, y = H-1 beside y = 0 of the next plane: neighbours in the linear key only
    wraps = [[1, 3, 4, W - 1], [1, 3, 5, 0], [1, 4, H - 1, 3], [1, 5, 0, 3]]
    for geom in GEOMS:
        cases[f'{geom}_faces_corners_and_wraps'] = _case(corners + faces + wraps, shape, 2, geom, 5, 16, seed=3)
        block = [[1, z, y, x] for z in range(2, 6) for y in range(3, 7) for x in range(1, 5)]
        cases[f'{geom}_dense_block_4x4x4'] = _case(block, shape, 2, geom, 4, 16, seed=4)
        lone = [[b, z, y, x] for b in (0, 2) for z in (1, 5) for y in (1, 5, 9) for x in (1, 5)]
        cases[f'{geom}_isolated'] = _case(lone, shape, 3, geom, 16, 16, bias=False, seed=5)
        good = random_coors(rng, 90, shape, 2)
        bad = np.array([[-1, -1, -1, -1], [2, 1, 1, 1], [0, D, 1, 1], [0, 1, H, 1], [1, 1, 1, W], [0, -1, 2, 2], [1, 2, 2, -3], [-1, 0, 0, 0]], np.int32)
        mixed = np.concatenate([good[:30], bad[:4], good[30:60], bad[4:], good[60:], np.full((11, 4), -1, np.int32)])
        cases[f'{geom}_inactive_rows_scattered_and_tail'] = _case(mixed, shape, 2, geom, 16, 32, seed=6)
    big = (41, 1600, 1408)                                                # B * D * H * W = 30 * 92 352 000 > 2^31
    rows = random_coors(rng, 300, (3, 12, 12), 1) + np.array([0, 38, 1588, 1396], np.int32)
    rows = np.concatenate([rows, random_coors(rng, 100, (3, 12, 12), 1)])
    rows[:, 0] = rng.choice([0, 17, 29], len(rows))
    for geom in ('subm', 's2p1'):
        cases[f'{geom}_keys_past_31_bits'] = _case(rows, big, 30, geom, 16, 16, seed=7, values='sparse')
    base = random_coors(rng, 120, shape, 2)
    true = int(index_ref(base, shape, 2, *GEOMS['s2p1'])['num'][1])
    for name, m in (('below', true - 7), ('at', true), ('above', true + 9)):
        cases[f's2p1_max_out_{name}'] = _case(base, shape, 2, 's2p1', 16, 16, max_out=m, seed=8)
    dup = np.concatenate([base[:40], base[10:20], base[:5]])
    for geom in ('subm', 's2p1'):
        cases[f'{geom}_duplicates'] = _case(dup, shape, 2, geom, 4, 16, seed=9, values=None)     # integers only: nothing faults, the lowest row
    # the kernels tile the channels by 16, 32 or 64: pairs that put 17 .. 32 and 33 .. 64 channels on either side of every kernel
    for n, (geom, cin, cout) in enumerate((('subm', 32, 32), ('s2p1', 24, 40), ('down', 40, 24), ('s2p011', 64, 16), ('subm', 16, 64))):
        cases[f'{geom}_channel_tiles_c{cin}_{cout}'] = _case(random_coors(rng, 150, (7, 11, 13), 3, empty=(1,)), (7, 11, 13), 3, geom, cin, cout, seed=40 + n)
    return cases


# geometries beyond the shipped encoders' (NOT in GEOMS: `_make_cases` loops over that): (kernel, stride, padding, subm), Cin, Cout
MORE_GEOMS = {
    'subm_k1': (((1, 1, 1), (1, 1, 1), (0, 0, 0), True), 1, 8),
    'subm_k311': (((3, 1, 1), (1, 1, 1), (1, 0, 0), True), 24, 12),
    'subm_k133': (((1, 3, 3), (1, 1, 1), (0, 1, 1), True), 136, 72),
    'subm_k515': (((5, 1, 5), (1, 1, 1), (2, 0, 2), True), 9, 9),
    'k1': (((1, 1, 1), (1, 1, 1), (0, 0, 0), False), 8, 1),
    'k2s2': (((2, 2, 2), (2, 2, 2), (0, 0, 0), False), 65, 33),
    'k2s1p1': (((2, 2, 2), (1, 1, 1), (1, 1, 1), False), 17, 17),
    'k3s1p0': (((3, 3, 3), (1, 1, 1), (0, 0, 0), False), 2, 3),
    'k3s1p1': (((3, 3, 3), (1, 1, 1), (1, 1, 1), False), 16, 20),
    'k3s3p2': (((3, 3, 3), (3, 3, 3), (2, 2, 2), False), 1, 1),
    'k3s4p0': (((3, 3, 3), (4, 4, 4), (0, 0, 0), False), 12, 40),
    'k133s122': (((1, 3, 3), (1, 2, 2), (0, 1, 1), False), 33, 65),
    'k233s212': (((2, 3, 3), (2, 1, 2), (1, 0, 1), False), 72, 136),
    'k551s221': (((5, 5, 1), (2, 2, 1), (2, 2, 0), False), 130, 66),
    'k27x1x1': (((27, 1, 1), (1, 1, 1), (13, 0, 0), False), 16, 16),
}
MORE_GEOM_CASES = {}      # geometry name -> case name
DEAD_ROWS = (64, 256)     # the rows of the `inactive_block` cases that are [-1, -1, -1, -1]


def _make_more_cases(old):
    """the cases added after `_make_cases`, drawn from a generator of their own: no earlier case changes.  A side above 64 channels uses
    the gather - matmul oracle (`values='sparse'`)."""
    rng = np.random.default_rng(23)
    cases = {}
    how = lambda cin, cout: 'sparse' if max(cin, cout) > 64 else 'dense'
    for n, (geom, (g, cin, cout)) in enumerate(MORE_GEOMS.items()):
        shape = ((9, 12, 10), (7, 11, 13))[n % 2]
        name = f'{geom}_{shape[0]}x{shape[1]}x{shape[2]}_c{cin}_{cout}'
        cases[name] = _case(random_coors(rng, 150, shape, 3, empty=(1,)), shape, 3, g, cin, cout, seed=60 + n, values=how(cin, cout))
        MORE_GEOM_CASES[geom] = name
    shape = (9, 12, 10)
    # the channel edges on the shipped geometries: the maximum on both sides, mixed 16-byte / element-wise paths, one channel
    cases['subm_c256_256_rows_400'] = _case(random_coors(rng, 400, shape, 2), shape, 2, 'subm', 256, 256, seed=80, values='sparse')
    for n, (geom, cin, cout) in enumerate((('s2p1', 256, 256), ('subm', 16, 20), ('s2p1', 40, 8), ('down', 1, 1))):
        cases[f'{geom}_c{cin}_{cout}'] = _case(random_coors(rng, 150, (7, 11, 13), 3, empty=(1,)), (7, 11, 13), 3, geom, cin, cout, seed=81 + n,
                                               values=how(cin, cout))
    # dead tiles: whole row tiles of both kernels inactive, with live rows on both sides
    good = random_coors(rng, 108, shape, 2)
    block = np.concatenate([good[:DEAD_ROWS[0]], np.full((DEAD_ROWS[1] - DEAD_ROWS[0], 4), -1, np.int32), good[DEAD_ROWS[0]:]])
    for geom in ('subm', 's2p1'):
        cases[f'{geom}_inactive_block'] = _case(block, shape, 2, geom, 16, 32, seed=86)
    at = old['s2p1_max_out_at']
    cases['s2p1_max_out_far_above'] = _case(at['coors'], shape, 2, 's2p1', 16, 16, max_out=at['max_out'] + 200, seed=87)
    for geom in ('subm', 's2p1'):                                         # 64 -> 64: the 16-bit kernel stages the weight in chunks and skips most
        cases[f'{geom}_isolated_c64_64'] = _case(old['subm_isolated']['coors'], shape, 3, geom, 64, 64, seed=88)
    return cases


CASES = _make_cases()
CASES.update(_make_more_cases(CASES))
SWEEP_SHAPE = (8, 48, 48)


@functools.lru_cache(maxsize=None)
def sweep_case(geom):
    """about 20 000 rows over 3 samples at 16 -> 32: many workgroups, several partial sums per offset in the weight gradient"""
    rng = np.random.default_rng(21)
    return _case(random_coors(rng, 20000, SWEEP_SHAPE, 3), SWEEP_SHAPE, 3, geom, 16, 32, seed=10)


MANY_B, MANY_EMPTY = 300, (0, 7, 256, 299)


@functools.lru_cache(maxsize=None)
def many_samples_case(geom):
    """900 rows over B = 300 samples of a (2, 3, 4) grid, four samples empty: more samples than one workgroup of the counting kernel has threads"""
    rng = np.random.default_rng(24)
    return _case(random_coors(rng, 900, (2, 3, 4), MANY_B, empty=MANY_EMPTY), (2, 3, 4), MANY_B, geom, 4, 4, seed=11, values=None)


def case_of(name):
    return sweep_case(name[len('sweep_'):]) if name.startswith('sweep_') else CASES[name]


@functools.lru_cache(maxsize=None)
def expected_index(name):
    c = case_of(name)
    return index_ref(c['coors'], c['shape'], c['B'], c['kernel'], c['stride'], c['padding'], c['subm'], c['max_out'])


@functools.lru_cache(maxsize=None)
def operands(name):
    """X (N, Cin), W (K, Cin, Cout), bias (Cout) or None, gY (R, Cout) fp32, fixed by the case's seed"""
    c, idx = case_of(name), expected_index(name)
    rng = np.random.default_rng(1000 + c['seed'])
    K = idx['nbr'].shape[1]
    X = rng.standard_normal((len(c['coors']), c['cin'])).astype(np.float32)
    W = (rng.standard_normal((K, c['cin'], c['cout'])) / np.sqrt(K * c['cin'])).astype(np.float32)
    bias = rng.standard_normal(c['cout']).astype(np.float32) if c['bias'] else None
    gY = rng.standard_normal((len(idx['nbr']), c['cout'])).astype(np.float32)
    return X, W, bias, gY


@functools.lru_cache(maxsize=None)
def expected_values(name):
    """-> (o64, A, L): the fp64 oracle, the same on absolute values, the term counts; computed once and shared, never modified"""
    c, idx = case_of(name), expected_index(name)
    X, W, bias, gY = operands(name)
    if c['values'] == 'sparse':
        run = lambda x, w, b, g: sparse_oracle(idx, x, w, b, g)
    else:
        run = lambda x, w, b, g: oracle(c['coors'], c['shape'], c['B'], c['kernel'], c['stride'], c['padding'], idx, x, w, b, g)
    o64 = run(X, W, bias, gY)
    A = run(np.abs(X), np.abs(W), None if bias is None else np.abs(bias), np.abs(gY))
    return o64, A, term_counts(idx, len(X), c['cin'], c['cout'], bias is not None)
