"""Case table of the scatter-reduce tests (tests/test_voxel_scatter.py): shapes chosen from the constants of the host dispatch in
csrc/voxel_scatter.hip, each with the path it is meant to reach and the predicate that proves it does, computed from the case's own
sizes.  The predicates restate HOST arithmetic only (which kernel, which index form, how many voxels per workgroup, where the tiles
start): a condition on the inputs, not a statement about what any kernel computes.  The arbiter of every result is
oracle/voxel_oracle.py in fp64; inputs and expectations are made once per process and frozen.

    vox_scatter_reduce            c % 4 == 0, c <= 256, aligned -> reduce_v4_kernel (lp = pow2 >= c / 4 lanes a voxel), else reduce_kernel
    vox_scatter_backward          max and c < 32 -> fill + max_grad_kernel (grid capped, grid-stride loop)
                                  else gather_grad_kernel<VEC = 4 if c % 4 == 0 and aligned else 1>; point = index / lanes-per-row as a
                                  shift | one multiply-high | a 64-bit division (launch_backward)
    vox_scatter_backward_grouped  c % 4 == 0, c <= 256, aligned -> spread_grad_v4_kernel; else c <= 128 -> spread_lds_kernel with
                                  lds_plan's voxels per workgroup, tiles of 1024 points; else GD3D_E_BADARG
    the autograd node             c % 4 == 0 and 32 <= c <= 256 and an aligned gradient -> the grouped entry, else the map-ordered one
"""
import collections
import functools

import numpy as np

from oracle import voxel_oracle as vo

# constants of csrc/voxel_scatter.hip, by value
WG = 256                       # threads per workgroup, every kernel (__launch_bounds__(256))
MAX_GRAD_GRID = 8192           # vox_scatter_backward: `if (mb > 8192) mb = 8192`
MAX_GRAD_C = 32                # vox_scatter_backward: `reduce == GD3D_REDUCE_MAX && c < 32`
LDS_TP = 1024                  # LDS_MAX_TP: points per tile
LDS_MAX_GV = 128               # LDS_MAX_GV: voxels per workgroup, at most
LDS_PAIRS = 512                # 256 * LDS_PAIRS: lds_plan's `p.gv = 256 * LDS_PAIRS / c`
LDS_C_MAX = 128                # lds_plan: `if (c > 128 || v <= 0) return false`
LDS_FIT = 0.8                  # lds_plan: `fit = (int)(0.8 * p.tp / avg)`
VEC_C_MAX = 256                # vox_scatter_reduce / _grouped: `c % 4 == 0 && c <= 256 && aligned`
NODE_GROUPED_C = (32, 256)     # the node: `c % 4 == 0 and 32 <= c <= 256` (_pynode.py GDScatterReduce.backward, torch_node.cpp)
GATHER_ITEMS = 4               # gather_grad_kernel: GU items per thread, vector and scalar
U32 = 1 << 32
EPS = 2.0 ** -24               # unit roundoff of fp32
REDS = ('sum', 'mean', 'max')
BADARG = 10001                 # GD3D_E_BADARG, include/gd3d.h


# ---- the host arithmetic, restated -------------------------------------------------------------------------------------------------

def pow2_at_least(c):
    p = 1
    while p < c and p < 64:
        p <<= 1
    return p


def forward_kernel(c, aligned=True):
    """vox_scatter_reduce -> ('v4', lanes per voxel) | ('scalar', lanes per voxel)"""
    if c % 4 == 0 and c <= VEC_C_MAX and aligned:
        return 'v4', pow2_at_least(c // 4)
    return 'scalar', pow2_at_least(c)


def index_form(n, c, vec):
    """launch_backward's shift / magic: how gather_grad_kernel turns a flat index into (point, lane) -> (form, cv)"""
    cv = c // 4 if vec else c
    if cv & (cv - 1) == 0:
        return 'shift', cv
    return ('mulhi' if n * cv < U32 // cv else 'div'), cv


def map_backward_kernel(n, c, red, aligned=True):
    """vox_scatter_backward -> 'max_grad' | ('gather_v4' | 'gather', index form, cv)"""
    if red == 'max' and c < MAX_GRAD_C:
        return 'max_grad'
    vec = c % 4 == 0 and aligned
    return ('gather_v4' if vec else 'gather',) + index_form(n, c, vec)


def lds_gv(c, n, v):
    """lds_plan -> (voxels per workgroup, the term that set it: 'pairs' = 512 / c, 'cap' = LDS_MAX_GV, 'fit', 'one') | None"""
    if c > LDS_C_MAX or v <= 0:
        return None
    gv, why = LDS_PAIRS // c, 'pairs'
    if gv > LDS_MAX_GV:
        gv, why = LDS_MAX_GV, 'cap'
    avg = n / v
    fit = int(LDS_FIT * LDS_TP / (avg if avg > 1.0 else 1.0))
    if fit < gv:
        gv, why = (1, 'one') if fit < 1 else (fit, 'fit')
    return gv, why


def grouped_kernel(n, c, v, aligned=True):
    """vox_scatter_backward_grouped -> ('spread_v4', lanes per voxel) | ('spread_lds', gv, why) | 'badarg'"""
    if c % 4 == 0 and c <= VEC_C_MAX and aligned:
        return 'spread_v4', pow2_at_least(c // 4)
    plan = lds_gv(c, n, v)
    return 'badarg' if plan is None else ('spread_lds',) + plan


def node_backward(c, aligned=True):
    return 'grouped' if c % 4 == 0 and NODE_GROUPED_C[0] <= c <= NODE_GROUPED_C[1] and aligned else 'map'


def lds_tiles(cnt, dropped, gv):
    """spread_lds_kernel's loop bounds: a workgroup owns gv consecutive voxels = the run [seg[v0], seg[v0 + nv]) of `order`, walked
    in tiles of LDS_TP points.  -> what the tiles of this cloud exercise"""
    seg = dropped + np.concatenate([[0], np.cumsum(cnt, dtype=np.int64)])
    bounds = set(seg.tolist())
    w = dict(workgroups=0, max_tiles=0, starts_inside_a_voxel=0, starts_on_a_boundary=0, later_tiles_with_several_voxels=0, short_last_workgroup=False)
    for v0 in range(0, len(cnt), gv):
        nv = min(gv, len(cnt) - v0)
        pb, pe = int(seg[v0]), int(seg[v0 + nv])
        starts = list(range(pb, pe, LDS_TP))
        w['workgroups'] += 1
        w['max_tiles'] = max(w['max_tiles'], len(starts))
        w['short_last_workgroup'] |= nv < gv
        for t0 in starts[1:]:
            w['starts_on_a_boundary' if t0 in bounds else 'starts_inside_a_voxel'] += 1
            t1 = min(t0 + LDS_TP, pe)
            w['later_tiles_with_several_voxels'] += any(t0 < int(s) < t1 for s in seg[v0 + 1:v0 + nv])
    return w


# ---- clouds ------------------------------------------------------------------------------------------------------------------------

def _drop(rng, coors, frac):
    k = max(1, int(round(frac * len(coors))))
    rows = rng.choice(len(coors), k, replace=False)
    coors[rows, rng.integers(0, 3, k)] = -1
    return coors


def _cells(ids):
    """cell id -> (z, y, x); ascending id = ascending voxel index"""
    ids = np.asarray(ids, np.int64)
    return np.stack([ids // 4096, ids // 64 % 64, ids % 64], -1).astype(np.int32)


def _uniform(seed, n, cells, frac=0.03, heavy=0.0):
    """n points over `cells` cells, `frac` of them dropped; `heavy` of them in ONE cell in the middle (a long run)"""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, cells, n)
    ids[rng.random(n) < heavy] = cells // 2
    return _drop(rng, _cells(ids), frac)


def _exact(seed, n, v, frac=0.03):
    """n points, exactly v voxels (every cell holds a point that is kept), frac dropped"""
    rng = np.random.default_rng(seed)
    k = int(round(frac * n))
    ids = np.concatenate([np.arange(v), rng.integers(0, v, n - k - v)])
    coors = np.concatenate([_cells(ids), _drop(rng, _cells(rng.integers(0, v, k)), 1.0)])
    return coors[rng.permutation(n)]


def _sweep(seed=31):
    """72 000 points: 68 000 cells of their own, 3 500 more in 1 200 of those cells, 500 dropped"""
    rng = np.random.default_rng(seed)
    own = rng.permutation(300 * 300)[:68_000]
    more = own[rng.integers(0, 1200, 3500)]
    ids = np.concatenate([own, more, rng.integers(0, 90_000, 500)])
    coors = np.stack([ids // 300, ids % 300, np.ones_like(ids)], -1).astype(np.int32)
    coors[np.arange(len(ids) - 500, len(ids)), rng.integers(0, 3, 500)] = -1
    return coors[rng.permutation(len(coors))]


def _runs(sizes, seed, dropped):
    rng = np.random.default_rng(seed)
    ids = np.repeat(np.arange(len(sizes)), sizes)
    coors = np.concatenate([_cells(ids), _drop(rng, _cells(rng.integers(0, len(sizes), dropped)), 1.0)])
    return coors[rng.permutation(len(coors))]


def _lds_a(seed=41):
    """voxel 0 of exactly one tile (the next tile starts ON a voxel boundary); a voxel of 3000 and two of 1500 points between
    voxels of 40..120: about 19 700 points, mean run about 125"""
    sizes = np.random.default_rng(seed).integers(40, 121, 154)
    sizes[0], sizes[40], sizes[90], sizes[120] = LDS_TP, 3000, 1500, 1500
    return _runs(sizes, seed, 600)


CLOUDS = {
    'div_4105': lambda: _uniform(1, 4105, 300), 'div_4104': lambda: _uniform(2, 4104, 300),
    'sweep': _sweep,
    'lds_a': _lds_a,
    'lds_b': lambda: _runs([5000], 42, 150),                          # one voxel, five tiles
    'lds_b3': lambda: _runs([2500, 1, 2500], 43, 150),                # gv == 1 with more than one workgroup (an addition)
    'lds_c': lambda: _runs([1] * 2980 + [2] * 20, 44, 90),            # singletons
    'wide': lambda: _uniform(5, 6000, 797, heavy=0.1),
    'misaligned': lambda: _uniform(6, 5000, 700),
    'guard': lambda: _exact(7, 4999, 1237),
    'nonfinite': lambda: _uniform(8, 3000, 300),
}


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def cloud(name):
    """-> coors (n, 3) int32, (voxel rows, point -> voxel map, points per voxel) of the oracle"""
    coors = np.ascontiguousarray(CLOUDS[name]())
    uo, mo, co = vo.scatter_index(coors)
    return _freeze(coors, uo, mo, co)


def _poison(feats, mo, co):
    """the non-finite plants, in the four voxels with most points (>= 3 each): channel 0 +inf twice and once more as the LAST point
    (ties for +inf); channel 1 all NaN; channel 2 all -inf; channel 3 NaN first, -inf after; and 2 % NaN anywhere in channels 4.."""
    rng = np.random.default_rng(9)
    a, b, c, d = np.argsort(-co, kind='stable')[:4]
    pts = lambda v: np.flatnonzero(mo == v)
    feats[:, 4:][rng.random(feats[:, 4:].shape) < 0.02] = np.nan
    feats[pts(a)[[1, 2, -1]], 0] = np.inf
    feats[pts(b), 1] = np.nan
    feats[pts(c), 2] = -np.inf
    feats[pts(d), 3] = -np.inf
    feats[pts(d)[0], 3] = np.nan
    feats[pts(a)[0], 5] = np.nan                                        # a NaN among finite values, first in its voxel
    return dict(inf_ties=(a, 0), all_nan=(b, 1), all_ninf=(c, 2), nan_then_ninf=(d, 3))


@functools.lru_cache(maxsize=4)
def inputs(name, c):
    """-> feats (n, c) fp32: N(0, 1); `sweep`: the extra points of a shared cell repeat an earlier row of it (exact ties for the max)"""
    coors, _, mo, co = cloud(name)
    rng = np.random.default_rng(1000 * c + len(coors))
    feats = rng.normal(0, 1, (len(coors), c)).astype(np.float32)
    if name == 'sweep':
        first = np.full(len(co), -1, np.int64)
        for i in np.flatnonzero(mo >= 0)[::-1]:
            first[mo[i]] = i
        later = np.flatnonzero((mo >= 0) & (first[np.clip(mo, 0, None)] != np.arange(len(mo))))
        tie = later[::2]
        feats[tie, ::2] = feats[first[mo[tie]], ::2]
    if name == 'nonfinite':
        _poison(feats, mo, co)
    return _freeze(feats)[0]


def plants(c):
    coors, _, mo, co = cloud('nonfinite')
    return _poison(np.zeros((len(coors), c), np.float32), mo, co)


@functools.lru_cache(maxsize=6)
def expected(name, c, red):
    """fp64 oracle of a case: out (v, c), grad_vox (v, c) fp32 N(0, 1), grad (n, c) = the gradient of the points for grad_vox, and for
    sum / mean the bound of sequential fp32 summation in ANY order of the voxel's points, per voxel and channel:
        |got - want| <= (count - 1) * 2^-24 * sum|x_i| [/ count for the mean] + 2^-24 * |want|
    (Higham, Accuracy and Stability, (4.4) to first order; the last term is the mean's division, resp. nothing for the sum)."""
    _, _, mo, co = cloud(name)
    feats = inputs(name, c)
    out, _ = vo.scatter_reduce(feats, mo, co, red)
    gv = np.random.default_rng(7 + c).normal(0, 1, out.shape).astype(np.float32)
    grad = vo.scatter_backward(gv, feats, mo, co, red)
    bound = None
    if red != 'max':
        keep = mo >= 0
        mass = np.zeros(out.shape)
        np.add.at(mass, mo[keep], np.abs(feats[keep].astype(np.float64)))
        bound = (co - 1)[:, None] * EPS * mass / (co[:, None] if red == 'mean' else 1) + EPS * np.abs(out)
    return dict(zip(('out', 'gv', 'grad', 'bound'), _freeze(out, gv, grad) + (bound,)))


# ---- the table ---------------------------------------------------------------------------------------------------------------------

Case = collections.namedtuple('Case', 'family cloud c path aligned')
Case.id = property(lambda k: f'{k.cloud}-c{k.c}' + ('' if k.aligned else '-misaligned'))

DIV_CASES = (Case('div', 'div_4105', 1023, ('gather', 'div', 1023), True), Case('div', 'div_4104', 1023, ('gather', 'mulhi', 1023), True),
             Case('div', 'div_4105', 4092, ('gather_v4', 'div', 1023), True), Case('div', 'div_4104', 4092, ('gather_v4', 'mulhi', 1023), True))
SWEEP_CASE = Case('sweep', 'sweep', 31, 'max_grad', True)
LDS_CASES = tuple(Case('lds', cl, c, ('spread_lds',) + plan, c != 64)
                  for cl, plans in (('lds_a', {3: (6, 'fit'), 10: (6, 'fit'), 33: (6, 'fit'), 127: (4, 'pairs'), 64: (6, 'fit')}),
                                    ('lds_b', {3: (1, 'one'), 10: (1, 'one'), 33: (1, 'one'), 127: (1, 'one'), 64: (1, 'one')}),
                                    ('lds_b3', {3: (1, 'one'), 127: (1, 'one')}),
                                    ('lds_c', {3: (LDS_MAX_GV, 'cap')}))
                  for c, plan in plans.items())
WIDE_CASES = (Case('wide', 'wide', 132, ('v4', 64), True), Case('wide', 'wide', 200, ('v4', 64), True), Case('wide', 'wide', 256, ('v4', 64), True),
              Case('wide', 'wide', 260, ('scalar', 64), True))
MISALIGNED_CASE = Case('misaligned', 'misaligned', 64, ('scalar', 64), False)
MISALIGNED_BADARG = Case('misaligned', 'misaligned', 132, 'badarg', False)
GUARD_CASES = tuple(Case('guard', 'guard', c, None, True) for c in (10, 12, 64, 132))
NONFINITE_CASES = (Case('nonfinite', 'nonfinite', 16, None, True), Case('nonfinite', 'nonfinite', 10, None, True))
ALL_CASES = DIV_CASES + (SWEEP_CASE,) + LDS_CASES + WIDE_CASES + (MISALIGNED_CASE, MISALIGNED_BADARG) + GUARD_CASES + NONFINITE_CASES
LONG_RUN_CLOUDS = ('lds_a', 'lds_b', 'lds_b3')


def reaches(case):
    """-> the list of failed conditions (empty: the case reaches its path), from the case's own sizes and the oracle's index"""
    coors, _, mo, co = cloud(case.cloud)
    n, v, c = len(coors), len(co), case.c
    bad = []

    def need(ok, what):
        if not ok:
            bad.append(f'{case.id}: {what}')

    if case.family == 'div':
        need(map_backward_kernel(n, c, 'sum') == case.path, f'the map-ordered backward takes {map_backward_kernel(n, c, "sum")}, not {case.path}')
        need(map_backward_kernel(n, c, 'max') == case.path, 'the max backward takes another kernel')
        need(node_backward(c) == 'map', 'the node does not take the map-ordered backward')
        cv = case.path[2]
        if case.path[1] == 'mulhi':       # the LAST n for which one multiply-high is exact at this cv
            need(index_form(n + 1, c, c % 4 == 0)[0] == 'div', 'n + 1 still takes the multiply-high')
        else:                             # the FIRST n that takes the division
            need(index_form(n - 1, c, c % 4 == 0)[0] == 'mulhi', 'n - 1 already takes the division')
        need(n * cv < U32, 'the index passes 2^32')
        need(forward_kernel(c)[0] == 'scalar' and c > 64, 'the forward is not the scalar multi-pass kernel')
        need(200 <= v <= 400, 'not a few hundred voxels')
    elif case.family == 'sweep':
        need(map_backward_kernel(n, c, 'max') == 'max_grad' and node_backward(c) == 'map', 'the max backward is not max_grad_kernel')
        need(v * c > MAX_GRAD_GRID * WG, f'v * c = {v * c} does not pass {MAX_GRAD_GRID * WG}: no second sweep')
        need((co > 1).sum() >= 1000, 'fewer than 1000 voxels with several points')
    elif case.family == 'lds':
        need(grouped_kernel(n, c, v, case.aligned) == case.path, f'the grouped backward takes {grouped_kernel(n, c, v, case.aligned)}, not {case.path}')
        w = lds_tiles(co, int((mo < 0).sum()), case.path[1])
        if case.cloud == 'lds_a':
            need(w['max_tiles'] >= 3 and w['starts_inside_a_voxel'] >= 3 and w['starts_on_a_boundary'] >= 1 and
                 w['later_tiles_with_several_voxels'] >= 2 and w['workgroups'] > 20, f'tiles: {w}')
        elif case.cloud == 'lds_b':
            need(v == 1 and w['max_tiles'] == 5 and w['workgroups'] == 1, f'tiles: {w}')
        elif case.cloud == 'lds_b3':
            need(v == 3 and w['workgroups'] == 3 and w['max_tiles'] == 3, f'tiles: {w}')
        else:
            need(w['max_tiles'] == 1 and w['workgroups'] > 20 and w['short_last_workgroup'] and (co == 1).mean() > 0.95, f'tiles: {w}')
    elif case.family == 'wide':
        need(forward_kernel(c) == case.path, f'the forward takes {forward_kernel(c)}, not {case.path}')
        if c <= VEC_C_MAX:
            need(c > 128 and forward_kernel(c + 1)[0] == 'scalar' and grouped_kernel(n, c, v) == ('spread_v4', 64) and node_backward(c) == 'grouped',
                 'not a one-voxel-per-wave vector shape')
            need(c == VEC_C_MAX or c // 4 < 64, 'no idle lanes')
        else:
            need(c % 4 == 0 and grouped_kernel(n, c, v) == 'badarg' and node_backward(c) == 'map', 'c > 256 is accepted by the grouped entry')
        kern = map_backward_kernel(n, c, 'sum')
        need(kern[0] == 'gather_v4' and 33 <= kern[2] <= 65, f'the map-ordered backward is {kern}')
        need(v % 4 != 0, 'v is a multiple of the voxels per workgroup')
    elif case.family == 'misaligned':
        need(c % 4 == 0 and forward_kernel(c, True)[0] == 'v4' and forward_kernel(c, False)[0] == 'scalar', 'alignment does not decide the forward')
        need(map_backward_kernel(n, c, 'sum', True)[0] == 'gather_v4' and map_backward_kernel(n, c, 'sum', False)[0] == 'gather', 'nor the gather')
        got = grouped_kernel(n, c, v, False)
        need((got if case.path == 'badarg' else got[0]) == ('badarg' if case.path == 'badarg' else 'spread_lds'), f'grouped, misaligned: {got}')
        need(grouped_kernel(n, c, v, True)[0] == 'spread_v4', 'grouped, aligned: not the vector kernel')
    elif case.family == 'guard':
        per_wave = 64 // forward_kernel(c)[1]
        need((per_wave == 1 or v % per_wave != 0) and v % (4 * per_wave) != 0, 'v is a multiple of the voxels per wave or workgroup')
        for red in ('sum', 'max'):
            kern = map_backward_kernel(n, c, red)
            need(kern == 'max_grad' or (n * kern[2]) % (WG * GATHER_ITEMS) != 0, 'n fills the last gather workgroup')
        need((v * c) % WG != 0, 'v * c fills the last max_grad workgroup')
        plan = lds_gv(c, n, v)
        need(plan is None or v % plan[0] != 0, 'v is a multiple of the voxels per LDS workgroup')
        if c == 10:
            need(map_backward_kernel(n, c, 'max') == 'max_grad' and grouped_kernel(n, c, v)[0] == 'spread_lds', 'c = 10 misses max_grad / spread_lds')
    elif case.family == 'nonfinite':
        need(map_backward_kernel(n, c, 'max') == 'max_grad', 'the map-ordered max backward is not max_grad_kernel')
        need(grouped_kernel(n, c, v, False)[0] == 'spread_lds', 'grouped, misaligned: not spread_lds')
        need(grouped_kernel(n, c, v, True)[0] == ('spread_v4' if c % 4 == 0 else 'spread_lds'), 'grouped, aligned')
        need(co[np.argsort(-co, kind='stable')[:4]].min() >= 3, 'a planted voxel has fewer than 3 points')
    # every cloud: dropped points, a voxel with several points; the long-run clouds a run beyond one tile
    need((mo < 0).any(), 'no dropped point')
    need((co > 1).any(), 'no voxel with more than one point')
    if case.cloud in LONG_RUN_CLOUDS:
        need(co.max() > LDS_TP, 'no run longer than one tile')
    return bad
