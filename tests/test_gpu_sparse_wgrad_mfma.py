"""The matrix-core weight gradient of the 16-bit sparse convolution on the MI355X (csrc/sparse_conv_wgrad_16.hip,
gd3d_sparse_conv_backward_weight_16_mfma), through `_backward_entries(..., 'mfma')` on the cases of the existing
weight-gradient test (`WGRAD_CASES`), in fp16 and bf16, with and without a bias gradient:
  1  grad_weight within 2 (L + 2) 2^-24 A of the fp64 oracle on the rounded operands (the matrix-core allowance of DESIGN.md §3.19: the
     derived (L + 2) u A with one full ulp per internal add), grad_bias bit-equal to gd3d_sparse_conv_backward_weight_16's, the same bits
     from run to run;
  2  on integer operands from {-2 .. 2}, where every order of addition is exact in fp32, grad_weight equals the old entry's and the
     integer sum BIT FOR BIT: what a swapped lane map, a transposed tile or a masking error cannot survive;
  3  step and chunk edges on a line of voxels (R = 1 .. 2080, num[0] below, at and above R);
  4  a NaN in a row that offset j does not use does not reach grad_weight[j];
  5  the C entry between guard bands, from aligned bases and with either operand shifted by 2 bytes;
  6  the 20 000-row sweeps, and a two-layer static stack with the switch on under graph capture;
  7  MlvlSparseEncoder in bf16 with `set_weight_grad('mfma')`."""
import functools

import numpy as np
import pytest
import torch

import mmdet3d_gaussian_amd as amd
import sparse_conv_16_cases as c16
import sparse_conv_ref as ref
from mmdet3d_gaussian_amd import _lib
from mmdet3d_gaussian_amd.sparse_conv import _backward_entries
from test_cpu_sparse_conv import ENC_B, SWEEPS, build_encoder, count_calls, encoder_inputs, run_index
from test_cpu_sparse_conv_16 import KINDS, convs_of

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
S = -77.0           # the sentinel of the guard test
WIDE = 'wide_subm_c65_130'   # 200 rows at 65 -> 130, seed 26: the case of tests/test_gpu_sparse_conv_16.py, rebuilt here
WGRAD_CASES = tuple(dict.fromkeys(list(c16.VALUE_CASES) + list(c16.DEAD_TILE_CASES))) + (WIDE,)
NEW, OLD = 'gd3d_sparse_conv_backward_weight_16_mfma', 'gd3d_sparse_conv_backward_weight_16'


@functools.lru_cache(maxsize=None)
def wide():
    """-> (case, restated index, X, gY fp32 numpy)"""
    rng = np.random.default_rng(26)
    case = ref._case(ref.random_coors(rng, 200, (9, 12, 10), 2), (9, 12, 10), 2, 'subm', 65, 130)
    X, gY = rng.standard_normal((200, 65)).astype(np.float32), rng.standard_normal((200, 130)).astype(np.float32)
    return case, ref.index_ref(case['coors'], case['shape'], case['B'], case['kernel'], case['stride'], case['padding'], case['subm'], case['max_out']), X, gY


def case_tables(name):
    """-> (case, restated index, X, gY fp32 numpy)"""
    if name == WIDE:
        return wide()
    X, _, _, gY = c16.operands(name)
    return c16.case_of(name), c16.expected_index(name), X, gY


@functools.lru_cache(maxsize=None)
def expected_gw(name, kind):
    """-> (o64, A, L) of grad_weight on the operands rounded to `kind`: `c16.expected_values`, and the same by `ref.sparse_oracle` for WIDE"""
    if name != WIDE:
        o64, A, L = c16.expected_values(name, kind)
        return o64['gw'], A['gw'], L['gw']
    case, idx, X, gY = wide()
    Xr, Gr = c16.rounded(X, kind), c16.rounded(gY, kind)
    W = np.zeros((idx['nbr'].shape[1], case['cin'], case['cout']))
    return (ref.sparse_oracle(idx, Xr, W, None, Gr)['gw'], ref.sparse_oracle(idx, np.abs(Xr), W, None, np.abs(Gr))['gw'],
            ref.term_counts(idx, len(X), case['cin'], case['cout'], False)['gw'])


def weight_grad(x16, g16, nbr, nbr_t, num, subm, has_bias, mode):
    """(grad_weight, grad_bias) through `_backward_entries`, no input gradient; x16 / g16 in the compute dtype"""
    w = torch.empty((nbr.size(1), x16.size(1), g16.size(1)), device=DEV)           # its shape alone is read
    return _backward_entries(x16, w, g16, nbr, nbr_t, num, subm, False, True, has_bias, x16.dtype, mode)[1:]


def within_mfma_bound(got, o64, A, L):
    """-> (|got - o64| <= 2 (L + 2) u A everywhere, the worst |got - o64| / A)"""
    err = np.abs(np.asarray(got, np.float64) - o64)
    ok = bool((err <= 2 * (L + 2) * ref.U * A).all())
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(A > 0, err / A, 0.0)
    return ok, float(ratio.max()) if ratio.size else 0.0


def integer_operands(n, cin, r, cout, seed):
    """integers from {-2 .. 2}: exact in fp16 and bf16, every partial sum far below 2^24 -> (X, gY) fp32 numpy"""
    rng = np.random.default_rng(seed)
    return rng.integers(-2, 3, (n, cin)).astype(np.float32), rng.integers(-2, 3, (r, cout)).astype(np.float32)


def integer_sum(nbr, X, gY):
    """X^T gY per offset over the pairs of `nbr`, exactly, as fp32 (every value an integer below 2^24)"""
    out = np.zeros((nbr.shape[1], X.shape[1], gY.shape[1]), np.int64)
    for j in range(nbr.shape[1]):
        o = np.nonzero(nbr[:, j] >= 0)[0]
        out[j] = X[nbr[o, j]].astype(np.int64).T @ gY[o].astype(np.int64)
    assert np.abs(out).max(initial=0) < 2 ** 24
    return out.astype(np.float32)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', WGRAD_CASES)
def test_grad_weight_within_the_matrix_core_bound_and_grad_bias_the_old_entrys_bits(name, kind):
    case, idx, X, gY = case_tables(name)
    o64, A, L = expected_gw(name, kind)
    index = run_index(case, DEV)
    dtype = c16.DTYPES[kind]
    x16, g16 = torch.from_numpy(X).to(DEV).to(dtype), torch.from_numpy(gY).to(DEV).to(dtype)
    for has_bias in (True, False):
        run = lambda mode: weight_grad(x16, g16, index.nbr, index.nbr_t, index.num, case['subm'], has_bias, mode)
        gw, gb = run('mfma')
        assert gw.dtype == torch.float32 and gw.shape == o64.shape
        ok, worst = within_mfma_bound(gw.cpu().numpy(), o64, A, L)
        print(f'{name} {kind} mfma: gw: worst |ours - o64| / A = {worst:.3e} (L up to {int(np.max(L, initial=0))})')
        assert ok, f'{name} {kind}: grad_weight misses 2 (L + 2) u A: worst ratio {worst:.3e}'
        gw_old, gb_old = run(None)
        gw2, gb2 = run('mfma')
        assert torch.equal(gw, gw2), f'{name} {kind}: grad_weight differs from run to run'
        assert bool(gw.any()) == bool((idx['nbr'] >= 0).any())
        if has_bias:
            assert gb.dtype == torch.float32 and torch.equal(gb, gb_old) and torch.equal(gb, gb2), f'{name} {kind}: grad_bias is not the old entry\'s'
        else:
            assert gb is None and gb_old is None


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', WGRAD_CASES)
def test_exact_operands_give_the_old_entrys_grad_weight_bit_for_bit(name, kind):
    case, idx, X, gY = case_tables(name)
    Xi, Gi = integer_operands(len(X), case['cin'], len(gY), case['cout'], 1 + case['seed'])
    want = integer_sum(idx['nbr'], Xi, Gi)
    index = run_index(case, DEV)
    dtype = c16.DTYPES[kind]
    x16, g16 = torch.from_numpy(Xi).to(DEV).to(dtype), torch.from_numpy(Gi).to(DEV).to(dtype)
    for has_bias in (True, False):
        gw, gb = weight_grad(x16, g16, index.nbr, index.nbr_t, index.num, case['subm'], has_bias, 'mfma')
        gw_old, gb_old = weight_grad(x16, g16, index.nbr, index.nbr_t, index.num, case['subm'], has_bias, None)
        assert torch.equal(gw, gw_old), f'{name} {kind}: grad_weight differs from {OLD} on exact operands'
        assert np.array_equal(gw.cpu().numpy(), want), f'{name} {kind}: grad_weight is not the integer sum'
        assert bool(gw.any()) == bool((idx['nbr'] >= 0).any()), f'{name} {kind}: grad_weight is all zero'
        assert (gb is None and gb_old is None) if not has_bias else torch.equal(gb, gb_old)


# ---- step and chunk edges: a line of R voxels, kernel (1, 1, 3), 16 -> 16 -------------------------------------------------------------

LINE_ROWS = (1, 31, 32, 33, 127, 128, 129, 2049, 2080)          # 2049, 2080: chunks of 64 rows, two steps a chunk; the last chunk 1 row / 32 rows


def chunk_rows(R, kcc):
    """`weight_parts` (csrc/sparse_conv_common.h) restated: the rows of one chunk"""
    cap = max(1, min(64, (64 << 20) // (kcc * 4)))
    return max(32, -(-(-(-R // cap)) // 32) * 32)


def line_index(R):
    coors = torch.zeros((R, 4), dtype=torch.int32)
    coors[:, 3] = torch.arange(R, dtype=torch.int32)
    return amd.sparse_conv_index(coors.to(DEV), (1, 1, R), 1, (1, 1, 3), 1, (0, 0, 1), True)


def check_line(R, kind, num0):
    """both oracles on the line of R rows; num0 None: the index's own count, else the static form's num[0]"""
    index = line_index(R)
    nbr = index.nbr.cpu().numpy().copy()
    assert nbr.shape == (R, 3) and (nbr[:, 1] == np.arange(R)).all()
    num = index.num
    if num0 is not None:
        num = torch.tensor([num0, num0], dtype=torch.int64, device=DEV)
        nbr[min(max(num0, 0), R):] = -1                            # rows at and past num[0] take no part
    idx = dict(nbr=nbr)
    dtype = c16.DTYPES[kind]
    rng = np.random.default_rng(300 + R)
    X, gY = rng.standard_normal((R, 16)).astype(np.float32), rng.standard_normal((R, 16)).astype(np.float32)
    Xr, Gr, W = c16.rounded(X, kind), c16.rounded(gY, kind), np.zeros((3, 16, 16))
    o64, A = ref.sparse_oracle(idx, Xr, W, None, Gr)['gw'], ref.sparse_oracle(idx, np.abs(Xr), W, None, np.abs(Gr))['gw']
    L = ref.term_counts(idx, R, 16, 16, False)['gw']
    run = lambda x, g, mode: weight_grad(torch.from_numpy(x).to(DEV).to(dtype), torch.from_numpy(g).to(DEV).to(dtype), index.nbr, None, num, True, True, mode)
    gw, gb = run(X, gY, 'mfma')
    ok, worst = within_mfma_bound(gw.cpu().numpy(), o64, A, L)
    print(f'line R = {R} num[0] = {num0} {kind} mfma: gw: worst |ours - o64| / A = {worst:.3e}')
    assert ok, f'R = {R}, num[0] = {num0}, {kind}: grad_weight misses its bound: {worst:.3e}'
    assert torch.equal(gb, run(X, gY, None)[1])
    Xi, Gi = integer_operands(R, 16, R, 16, 400 + R)
    gwi = run(Xi, Gi, 'mfma')[0]
    assert torch.equal(gwi, run(Xi, Gi, None)[0]) and np.array_equal(gwi.cpu().numpy(), integer_sum(nbr, Xi, Gi)), (R, num0, kind)
    assert bool(gwi.any()) == bool((nbr >= 0).any())


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('R', LINE_ROWS)
def test_step_and_chunk_edges_on_a_line_of_voxels(R, kind):
    assert chunk_rows(R, 3 * 16 * 16) == (64 if R >= 2049 else 32)
    check_line(R, kind, None)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('R', [129, 2080])
def test_the_static_count_cuts_the_rows_on_a_line_of_voxels(R, kind):
    for num0 in (0, 1, 32, R - 1, R + 71):
        check_line(R, kind, num0)


# ---- containment ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', ['subm_inactive_rows_scattered_and_tail', 's2p1_max_out_above'])
def test_a_nan_reaches_only_the_offsets_that_read_it(name, kind):
    case, idx, X, gY = case_tables(name)
    index = run_index(case, DEV)
    dtype, nbr = c16.DTYPES[kind], idx['nbr']
    run = lambda x, g: weight_grad(torch.from_numpy(x).to(DEV).to(dtype), torch.from_numpy(g).to(DEV).to(dtype), index.nbr, index.nbr_t, index.num,
                                   case['subm'], True, 'mfma')
    gw, gb = run(X, gY)
    assert torch.isfinite(gw).all() and gw.any() and gb.any()
    inactive = ~ref.active_rows(case['coors'], case['shape'], case['B'])
    unused = ~(nbr >= 0).any(1)                                   # no neighbour at any offset, or at / past num[0] (the restated rows hold -1)
    assert (nbr[int(idx['num'][0]):] == -1).all() and unused.any() and (inactive.any() or not case['subm'])
    Xn, Gn = X.copy(), gY.copy()
    Xn[inactive] = np.nan
    Gn[unused] = np.nan
    gw_n, gb_n = run(Xn, Gn)
    assert torch.equal(gw_n, gw) and torch.equal(gb_n, gb), f'{name} {kind}: a NaN in a row that nothing reads reached a gradient'
    some = np.nonzero(((nbr >= 0).sum(1) > 0) & ((nbr >= 0).sum(1) < nbr.shape[1]))[0]
    o = int(some[0])                                              # a row with a neighbour at some offsets only
    reads = nbr[o] >= 0
    Gn = gY.copy()
    Gn[o] = np.nan
    gw_n = run(X, Gn)[0]
    for j in range(nbr.shape[1]):
        if reads[j]:
            assert torch.isnan(gw_n[j]).all(), f'{name} {kind}: offset {j} reads row {o}'
        else:
            assert torch.equal(gw_n[j], gw[j]), f'{name} {kind}: offset {j} does not read row {o}'


# ---- the C entry between guard bands -----------------------------------------------------------------------------------------------------

def run_c_entry_between_bands(name, kind, shift_x, shift_g, has_bias):
    """gd3d_sparse_conv_backward_weight_16_mfma on sentinel-filled grad_weight, grad_bias and workspace with a band either side;
    shift_x / shift_g: elements (of 2 bytes) past a 16-byte aligned address for features / grad_out -> (gw, gb) between the bands"""
    dtype, code = c16.DTYPES[kind], {'fp16': 1, 'bf16': 2}[kind]
    case, idx, X, gY = case_tables(name)
    index = run_index(case, DEV)
    N, Cin, R, Cout, K = len(X), case['cin'], len(idx['nbr']), case['cout'], idx['nbr'].shape[1]
    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
    G, band = 64, 4096

    def shifted(a, by):
        buf = torch.zeros(a.size + 8, dtype=dtype, device=DEV)
        buf[by:by + a.size] = torch.from_numpy(a).to(DEV).to(dtype).flatten()
        assert buf.data_ptr() % 16 == 0
        return buf, buf.data_ptr() + 2 * by
    (xb, x_at), (gb_, g_at) = shifted(X, shift_x), shifted(gY, shift_g)
    gw_buf = torch.full((K * Cin * Cout + 2 * G,), S, device=DEV)
    gb_buf = torch.full((Cout + 2 * G,), S, device=DEV)
    nbytes = lib.gd3d_sparse_conv_backward_weight_workspace_bytes(R, K, Cin, Cout)
    work = torch.full((nbytes + 2 * band,), 0x5a, dtype=torch.uint8, device=DEV)
    assert nbytes % 256 == 0 and (work.data_ptr() + band) % 256 == 0
    _lib.check(lib.gd3d_sparse_conv_backward_weight_16_mfma(x_at, g_at, index.nbr.data_ptr(), index.num.data_ptr(), N, R, K, Cin, Cout, code,
                                                            work.data_ptr() + band, gw_buf.data_ptr() + 4 * G,
                                                            gb_buf.data_ptr() + 4 * G if has_bias else None, stream), NEW)
    torch.cuda.synchronize()
    assert (gw_buf[:G] == S).all() and (gw_buf[-G:] == S).all(), 'a band of grad_weight was written'
    assert (gb_buf[:G] == S).all() and (gb_buf[-G:] == S).all() and (has_bias or (gb_buf == S).all()), 'a band of grad_bias was written'
    assert (work[:band] == 0x5a).all() and (work[-band:] == 0x5a).all(), 'a workspace band was written'
    return gw_buf[G:-G].reshape(K, Cin, Cout).clone(), gb_buf[G:-G].clone() if has_bias else None


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', c16.GUARD_CASES)
def test_the_c_entry_between_guard_bands_aligned_and_shifted_by_2_bytes(name, kind):
    """every element between the bands is written (it holds the bits `_backward_entries` gives on plain buffers, never the sentinel);
    with features or grad_out 2 bytes past an aligned base the element-wise staging gives the aligned call's bits"""
    case, idx, X, gY = case_tables(name)
    index = run_index(case, DEV)
    dtype = c16.DTYPES[kind]
    want_gw, want_gb = weight_grad(torch.from_numpy(X).to(DEV).to(dtype), torch.from_numpy(gY).to(DEV).to(dtype), index.nbr, index.nbr_t, index.num,
                                   case['subm'], True, 'mfma')
    ok, worst = within_mfma_bound(want_gw.cpu().numpy(), *expected_gw(name, kind))
    assert ok, worst
    for shift_x, shift_g in ((0, 0), (1, 0), (0, 1)):
        for has_bias in (True, False):
            gw, gb = run_c_entry_between_bands(name, kind, shift_x, shift_g, has_bias)
            assert torch.equal(gw, want_gw), f'{name} {kind}: grad_weight with shifts ({shift_x}, {shift_g})'
            assert gb is None or torch.equal(gb, want_gb), f'{name} {kind}: grad_bias with shifts ({shift_x}, {shift_g})'


# ---- replay --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', SWEEPS)
def test_sweep_of_20000_rows_in_bf16(name):
    """about 20 000 rows at 16 -> 32: 64 partial sums per offset, 10 steps a chunk"""
    case, idx, X, gY = case_tables(name)
    index = run_index(case, DEV)
    x16, g16 = torch.from_numpy(X).to(DEV).bfloat16(), torch.from_numpy(gY).to(DEV).bfloat16()
    run = lambda mode: weight_grad(x16, g16, index.nbr, index.nbr_t, index.num, case['subm'], True, mode)
    gw, gb = run('mfma')
    ok, worst = within_mfma_bound(gw.cpu().numpy(), *expected_gw(name, 'bf16'))
    print(f'{name} bf16 mfma: gw: worst |ours - o64| / A = {worst:.3e}')
    assert ok, f'{name}: grad_weight misses its bound: {worst:.3e}'
    again, old = run('mfma'), run(None)
    assert torch.equal(gw, again[0]) and torch.equal(gb, again[1]) and torch.equal(gb, old[1])


def test_static_two_layer_stack_with_the_switch_on_under_graph_capture(monkeypatch):
    """tests/test_gpu_sparse_conv_16.py's graph test with weight_grad='mfma': SparseConv3d(k3 s2 p1, max_out) -> SubMConv3d in bf16, forward and
    backward recorded on one stream in ONE graph, replayed on fresh inputs, bit-equal to the eager run of the same inputs"""
    shape, B, N, MO = (9, 12, 10), 2, 200, 230
    rng = np.random.default_rng(17)

    def rows(n_active):
        c = np.full((N, 4), -1, np.int32)
        c[:n_active] = ref.random_coors(rng, n_active, shape, B)
        return torch.from_numpy(c)
    torch.manual_seed(18)
    down = amd.SparseConv3d(16, 32, 3, 2, 1, bias=True, max_out=MO, compute_dtype=torch.bfloat16, weight_grad='mfma').to(DEV)
    subm = amd.SubMConv3d(32, 32, 3, bias=False, compute_dtype=torch.bfloat16, weight_grad='mfma').to(DEV)
    params = [down.weight, down.bias, subm.weight]
    coors, feats, gy = rows(180).to(DEV), torch.randn(N, 16, device=DEV).requires_grad_(True), torch.randn(MO, 32, device=DEV).bfloat16()

    def step():
        y = subm(down(amd.SparseConvTensor(feats, coors, shape, B)))
        return [y.indices, y.features] + list(torch.autograd.grad(y.features, [feats] + params, gy))

    calls = count_calls(monkeypatch)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        warm = [t.clone() for t in step()]                        # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    assert calls.get(NEW) == 2 and OLD not in calls, calls
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(captured, warm):
        assert torch.equal(got, want)
    with torch.no_grad():
        coors.copy_(rows(120))
        feats.copy_(torch.randn(N, 16, device=DEV))
        gy.copy_(torch.randn(MO, 32, device=DEV))
    graph.replay()
    torch.cuda.synchronize()
    eager = step()
    assert captured[3].dtype == torch.float32 and captured[4].dtype == torch.float32 and captured[5].dtype == torch.float32
    assert not torch.equal(eager[3], warm[3]) and not torch.equal(eager[5], warm[5])
    for got, want in zip(captured, eager):
        assert torch.equal(got, want)
    assert all(torch.isfinite(t).all() for t in captured[1:]) and captured[3].any() and captured[5].any()


# ---- through the modules -------------------------------------------------------------------------------------------------------------------

def test_mlvl_sparse_encoder_in_bf16_with_the_switch_on(monkeypatch):
    """`MlvlSparseEncoder(compute_dtype=bf16).set_weight_grad('mfma')` on the (25, 24, 20) grid: one backward calls the new entry once per
    conv and gives every conv weight a finite fp32 gradient.  The bound is asserted PER LAYER ON THE CONV'S OWN SAVED OPERANDS (its bf16
    input rows and the bf16 gradient that reached its output, both recorded by hooks), through `_backward_entries`: the gradient with the
    switch on is the conv's `weight.grad` bit for bit, lies within 2 (L + 2) u A of the fp64 sum over the layer's tables, the gradient with
    the switch off within (L + 2) u A of it, and so the two within 3 (L + 2) u A of each other."""
    grid = (25, 24, 20)
    coors, feats = encoder_inputs(grid)
    ref_state = build_encoder(DEV, grid).state_dict()
    torch.manual_seed(6)
    enc = amd.MlvlSparseEncoder(in_channels=4, sparse_shape=list(grid), order=('conv', 'norm', 'act'), compute_dtype=torch.bfloat16).to(DEV).eval()
    enc.load_state_dict(ref_state)
    assert enc.set_weight_grad('mfma') is enc
    seen = {}

    def record(mod, args, out):
        seen[mod] = dict(x=args[0].features.detach(), index=mod.index_of(args[0]))
        out.features.register_hook(lambda g, mod=mod: seen[mod].__setitem__('gy', g.detach().clone()))
    hooks = [m.register_forward_hook(record) for m in convs_of(enc)]
    got = enc(torch.from_numpy(feats).to(DEV), torch.from_numpy(coors).to(DEV), ENC_B)
    for h in hooks:
        h.remove()
    calls = count_calls(monkeypatch)
    loss = got['spatial_features'].float().square().sum() + sum(f.features.float().square().sum() for f in got['encode_features'])
    loss.backward()
    assert len(seen) == len(convs_of(enc)) == 12 and calls.get(NEW) == 12 and OLD not in calls, calls
    worst_on = worst_off = 0.0
    for conv, rec in seen.items():
        assert conv.weight.grad is not None and conv.weight.grad.dtype == torch.float32 and torch.isfinite(conv.weight.grad).all()
        index, x16, gy16 = rec['index'], rec['x'].to(torch.bfloat16).contiguous(), rec['gy'].to(torch.bfloat16).contiguous()
        assert index.nbr.size(0) > 0 and conv.weight.grad.any()
        on = weight_grad(x16, gy16, index.nbr, index.nbr_t, index.num, conv.subm, False, 'mfma')[0]
        off = weight_grad(x16, gy16, index.nbr, index.nbr_t, index.num, conv.subm, False, None)[0]
        assert torch.equal(on.reshape(conv.weight.shape), conv.weight.grad), f'{conv}: weight.grad is not the new entry on the saved operands'
        idx = dict(nbr=index.nbr.cpu().numpy())
        X, G = x16.double().cpu().numpy(), gy16.double().cpu().numpy()
        W = np.zeros((idx['nbr'].shape[1], conv.in_channels, conv.out_channels))
        o64, A = ref.sparse_oracle(idx, X, W, None, G)['gw'], ref.sparse_oracle(idx, np.abs(X), W, None, np.abs(G))['gw']
        L = ref.term_counts(idx, len(X), conv.in_channels, conv.out_channels, False)['gw']
        ok_on, r_on = within_mfma_bound(on.cpu().numpy(), o64, A, L)
        ok_off, r_off = ref.within_bound(off.cpu().numpy(), o64, A, L)
        worst_on, worst_off = max(worst_on, r_on), max(worst_off, r_off)
        assert ok_on and ok_off, f'{conv}: on {r_on:.3e}, off {r_off:.3e}'
        assert (np.abs(on.double().cpu().numpy() - off.double().cpu().numpy()) <= 3 * (L + 2) * ref.U * A).all(), f'{conv}: on and off differ by more than 3 (L + 2) u A'
    print(f'MlvlSparseEncoder bf16 weight gradients: worst |ours - o64| / A with the switch on {worst_on:.3e}, off {worst_off:.3e}')
    for n, p in enc.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32 and torch.isfinite(p.grad).all(), n
