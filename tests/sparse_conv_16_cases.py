"""Cases, oracle and bounds of the fp16 / bf16 sparse 3D convolution tests (include/gd3d.h, gd3d_sparse_conv_*_16).

* the cases    every value case of tests/sparse_conv_ref.py (their channel pairs put every path of csrc/sparse_conv_16.hip under test:
               4, 5 and 3 input channels the element-wise gather and a ragged end of the reduction axis, 16 channels two offsets per
               step of 32 and a half-filled last step, 24 / 40 an offset that straddles a step, K = 3 of `down` one and a half steps,
               `isolated` steps that are skipped; the further geometries and channel edges add K Cin < 32, partial second to fourth column
               tiles and chunks that are never staged), and `ROW_CASES`: row counts around the 16 rows of a wave and the 128 rows of a
               workgroup of the 16-bit kernel, at 16 -> 16, built with `ref._case` / `ref.random_coors`.
* the oracle   `ref.oracle` / `ref.sparse_oracle` (the fp64 dense conv3d) on the operands AFTER rounding X, W and gY to the 16-bit
               type (`.to(dtype).double()`); the bias stays fp32.  A: the same on absolute values.  L: `ref.term_counts`.
* the bounds   u = 2^-24.  fp32 outputs (gw, gb): (L + 2) u A, `ref.within_bound` unchanged — the products of two 16-bit values are exact
               in fp32 and the sum is the fp32 kernel's.  16-bit outputs (out, gx): |got - want| <= E + u16 (|want| + E) + s with
               E = 2 (L + 2) u A (the factor 2 allows the matrix core's internal adds one full ulp each, truncation instead of
               rounding), u16 = 2^-11 (fp16) or 2^-8 (bf16) for the ONE rounding of the accumulated value, and s = 2^-25 for fp16 (half
               the subnormal spacing), 0 for bf16.
"""
import functools

import numpy as np
import torch

import sparse_conv_ref as ref

WAVE_ROWS = 16          # rows of one wave's MFMA tile (csrc/sparse_conv_16.hip)
TILE_M16 = 128          # output rows of one workgroup of the 16-bit kernel (csrc/sparse_conv_common.h)
DTYPES = {'fp16': torch.float16, 'bf16': torch.bfloat16}
U16 = {'fp16': 2.0 ** -11, 'bf16': 2.0 ** -8}
SUB = {'fp16': 2.0 ** -25, 'bf16': 0.0}


def _make_row_cases():
    rng = np.random.default_rng(22)
    cases = {}
    counts = (('rows_0', 0), ('rows_1', 1), ('rows_wave_minus_1', WAVE_ROWS - 1), ('rows_wave', WAVE_ROWS), ('rows_wave_plus_1', WAVE_ROWS + 1),
              ('rows_tile16_minus_1', TILE_M16 - 1), ('rows_tile16', TILE_M16), ('rows_tile16_plus_1', TILE_M16 + 1),
              ('rows_2_tiles16_plus_1', 2 * TILE_M16 + 1))
    for geom in ('subm', 's2p1'):
        for name, n in counts:
            cases[f'{geom}_{name}'] = ref._case(ref.random_coors(rng, n, (9, 12, 10), 2), (9, 12, 10), 2, geom, 16, 16, seed=100 + n)
    return cases


ROW_CASES = _make_row_cases()
VALUE_CASES = sorted(n for n, c in ref.CASES.items() if c['values']) + sorted('16:' + n for n in ROW_CASES)
# the seven first cases of the fp32 guard test, the 4 -> 16 submanifold case (the element-wise gather), the submanifold case of the other
# grid, and the dead-tile cases: a workgroup whose 128 rows are all inactive or past num[0], weight chunks that are never staged
DEAD_TILE_CASES = ('subm_inactive_block', 's2p1_inactive_block', 's2p1_max_out_far_above', 'subm_isolated_c64_64', 's2p1_isolated_c64_64')
GUARD_CASES = ('subm_inactive_rows_scattered_and_tail', 's2p1_max_out_below', 's2p1_max_out_above', 'down_7x11x13_c16_32', 's2p011_7x11x13_c3_7',
               'subm_rows_1', 's2p1_rows_tile_plus_1', 'subm_9x12x10_c4_16', 'subm_7x11x13_c64_64') + DEAD_TILE_CASES


def case_of(name):
    """'16:<name>' is a row case of this file, 'sweep_<geom>' and every other name a case of sparse_conv_ref.py"""
    return ROW_CASES[name[3:]] if name.startswith('16:') else ref.case_of(name)


@functools.lru_cache(maxsize=None)
def expected_index(name):
    if not name.startswith('16:'):
        return ref.expected_index(name)
    c = case_of(name)
    return ref.index_ref(c['coors'], c['shape'], c['B'], c['kernel'], c['stride'], c['padding'], c['subm'], c['max_out'])


@functools.lru_cache(maxsize=None)
def operands(name):
    """X, W, bias, gY fp32: `ref.operands`' draws (standard normal, the weights scaled by 1 / sqrt(K Cin)), fixed by the case's seed"""
    if not name.startswith('16:'):
        return ref.operands(name)
    c, idx = case_of(name), expected_index(name)
    rng = np.random.default_rng(1000 + c['seed'])
    K = idx['nbr'].shape[1]
    X = rng.standard_normal((len(c['coors']), c['cin'])).astype(np.float32)
    W = (rng.standard_normal((K, c['cin'], c['cout'])) / np.sqrt(K * c['cin'])).astype(np.float32)
    bias = rng.standard_normal(c['cout']).astype(np.float32) if c['bias'] else None
    gY = rng.standard_normal((len(idx['nbr']), c['cout'])).astype(np.float32)
    return X, W, bias, gY


def rounded(a, kind):
    """an fp32 array after rounding to the 16-bit type, in fp64"""
    return torch.from_numpy(np.ascontiguousarray(a)).to(DTYPES[kind]).double().numpy()


def oracle_on(case, idx, X, W, bias, gY):
    """the fp64 oracle and the same on absolute values -> (o64, A)"""
    if case['values'] == 'sparse':
        run = lambda x, w, b, g: ref.sparse_oracle(idx, x, w, b, g)
    else:
        run = lambda x, w, b, g: ref.oracle(case['coors'], case['shape'], case['B'], case['kernel'], case['stride'], case['padding'], idx, x, w, b, g)
    return run(X, W, bias, gY), run(np.abs(X), np.abs(W), None if bias is None else np.abs(bias), np.abs(gY))


@functools.lru_cache(maxsize=None)
def expected_values(name, kind):
    """-> (o64, A, L) on the operands rounded to `kind`; computed once and shared, never modified"""
    c, idx = case_of(name), expected_index(name)
    X, W, bias, gY = operands(name)
    o64, A = oracle_on(c, idx, rounded(X, kind), rounded(W, kind), bias, rounded(gY, kind))
    return o64, A, ref.term_counts(idx, len(X), c['cin'], c['cout'], bias is not None)


def within_bound_16(got, want, scale, L, kind):
    """-> (elementwise |got - want| <= E + u16 (|want| + E) + s with E = 2 (L + 2) u scale holds everywhere, the worst |got - want| / scale)"""
    err = np.abs(np.asarray(got, np.float64) - want)
    E = 2 * (L + 2) * ref.U * scale
    ok = bool((err <= E + U16[kind] * (np.abs(want) + E) + SUB[kind]).all())
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(scale > 0, err / scale, 0.0)
    return ok, float(ratio.max()) if ratio.size else 0.0
