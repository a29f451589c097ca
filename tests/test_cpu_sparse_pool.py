"""Sparse max pooling on the `_cpu` twins (gd3d_sparse_max_pool_*; csrc/sparse_pool_cpu.cpp).

Forward: BIT-equal to the fp64 oracle — the -inf-filled dense `max_pool3d` read at `out_coors`, and the restatement over the table —
in fp32, fp16 and bf16: the output element is a copy of an input element, the inputs hold no zero of either sign, and no element is left
out of the comparison.  Backward: |got - want| <= (m - 1) 2^-24 S against the restated tie rule (m terms of magnitudes summing to S, m <=
prod(ceil(k / s))), E + u16 (|want| + E) on the 16-bit types; exact on integer-valued data.
The check functions take the device: tests/test_gpu_sparse_decoder.py runs them on cuda:0."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mmdet3d_gaussian_amd as amd
import sparse_conv_ref as ref
import sparse_decoder_ref as dref
from mmdet3d_gaussian_amd import _host, _lib
from sparse_decoder_ref import POOL_MAX_BLOCKS, pool_rows

KINDS = ('fp32', 'fp16', 'bf16')
B = 2
GEOMS = {       # name -> (shape, kernel, stride, padding); K = 1, 8, 27, 27
    'k1s1': ((6, 10, 9), (1, 1, 1), (1, 1, 1), (0, 0, 0)),
    'k2s2': ((9, 11, 12), (2, 2, 2), (2, 2, 2), (0, 0, 0)),
    'k3s1p1': ((6, 10, 9), (3, 3, 3), (1, 1, 1), (1, 1, 1)),
    'k3s2p1': ((9, 11, 12), (3, 3, 3), (2, 2, 2), (1, 1, 1)),
}
CHANNELS = {'fp32': (1, 3, 4, 5, 16, 20, 64, 256), 'fp16': (1, 7, 8, 9, 16, 24, 64, 256), 'bf16': (1, 7, 8, 9, 16, 24, 64, 256)}
N_ROWS = 250
S = -77.0                   # the sentinel of the guard bands: exact in every type
PAD = 64                    # elements of a guard band: a multiple of 16 bytes in every type


@functools.lru_cache(maxsize=None)
def case_of(geom, max_out=None, inactive=False):
    shape, kernel, stride, padding = GEOMS[geom]
    rng = np.random.default_rng(800 + sorted(GEOMS).index(geom))
    coors = ref.random_coors(rng, N_ROWS, shape, B)
    if inactive:
        coors = coors.copy()
        coors[rng.choice(N_ROWS, 30, replace=False)] = -1
        coors[7] = [0, shape[0], 1, 1]
    if isinstance(max_out, str):
        total = int(ref.index_ref(coors, shape, B, kernel, stride, padding, False)['num'][1])
        max_out = total + 300 if max_out == 'above' else total - 13
    return coors, ref.index_ref(coors, shape, B, kernel, stride, padding, False, max_out), max_out


def run_index(geom, dev, max_out=None, inactive=False):
    shape, kernel, stride, padding = GEOMS[geom]
    coors, _, mo = case_of(geom, max_out, inactive)
    return amd.sparse_conv_index(torch.from_numpy(coors).to(dev), shape, B, kernel, stride, padding, False, mo)


def synthetic_index(tables, dev):
    """a `SparseConvIndex` around restated or synthetic tables (no count: every row is considered)"""
    nbr, nbr_t = torch.from_numpy(tables['nbr']).to(dev), torch.from_numpy(tables['nbr_t']).to(dev)
    return amd.SparseConvIndex(torch.zeros((len(nbr), 4), dtype=torch.int32, device=dev), (1, 1, max(1, len(nbr))), nbr, nbr_t, None, None, False, len(nbr_t))


def draws(shape, kind, seed, how='normal'):
    """fp32 numpy values that the kind holds exactly, without a zero of either sign"""
    rng = np.random.default_rng(seed)
    if how == 'normal':
        a = rng.standard_normal(shape)
    elif how == 'negative':
        a = -np.abs(rng.standard_normal(shape)) - 0.5
    else:                                                                # small integers: every sum is exact in every type
        a = rng.integers(1, 4, shape).astype(np.float64)
    a = dref.rounded(a.astype(np.float32), kind).astype(np.float32)
    assert a.all()
    return a


def run_pool(dev, kind, index, X, gY):
    """`sparse_max_pool` and its gradient -> (out, gx) as tensors of the kind's dtype on the CPU"""
    x = torch.from_numpy(X).to(dev).to(dref.DTYPES[kind]).requires_grad_(True)
    out = amd.sparse_max_pool(x, index)
    assert out.dtype == x.dtype and out.shape == (index.nbr.size(0), X.shape[1])
    (gx,) = torch.autograd.grad(out, x, torch.from_numpy(gY).to(dev).to(x.dtype))
    assert gx.dtype == x.dtype and gx.shape == x.shape
    return out.detach().cpu(), gx.cpu()


def same_bits(a, b):
    """two tensors of one dtype hold the same bits, NaN payloads included"""
    view = torch.int32 if a.dtype == torch.float32 else torch.int16
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(view), b.contiguous().view(view))


def assert_against_tables(tables, X, gY, out, gx, kind, what):
    """forward equal to the restatement element for element; backward within the derived bound of the restated tie rule"""
    want = dref.pool_ref(tables, X)
    got = out.double().numpy()
    assert np.array_equal(got, want, equal_nan=True), f'{what} {kind}: {int((got != want).sum())} forward elements differ from the restatement'
    wgx, Ssum, m = dref.unpool_ref(tables, X, want, gY)
    ok, err = dref.within_pool_backward_bound(gx.double().numpy(), wgx, Ssum, m, kind)
    assert ok, f'{what} {kind}: the gradient misses its bound, worst error {err:.3e}'
    return want, wgx, m


def check_geometry(dev, kind, geom, C, max_out=None, inactive=False, how='normal'):
    shape, kernel, stride, padding = GEOMS[geom]
    coors, idx, _ = case_of(geom, max_out, inactive)
    index = run_index(geom, dev, max_out, inactive)
    X, gY = draws((len(coors), C), kind, 10 + C, how), draws((len(idx['nbr']), C), kind, 20 + C)
    act = ref.active_rows(coors, shape, B)
    Xdev = X.copy()
    Xdev[~act] = np.nan                                                  # what an inactive row holds never shows
    out, gx = run_pool(dev, kind, index, Xdev, gY)
    dense = dref.pool_oracle(coors, shape, B, kernel, stride, padding, idx, X)
    assert np.array_equal(out.double().numpy(), dense), f'{geom} C={C} {kind}: differs from the dense max_pool3d'
    live = (idx['nbr'] >= 0).any(1)
    assert np.isfinite(dense[live]).all() and live.sum() == idx['num'][0] and not out[torch.from_numpy(~live)].any()
    want, wgx, m = assert_against_tables(idx, np.where(act[:, None], X, 0.0), gY, out, gx, kind, f'{geom} C={C}')
    assert m.max() <= np.prod([-(-k // s) for k, s in zip(kernel, stride)])
    fed = (idx['nbr_t'] >= 0).any(1)
    assert not gx[torch.from_numpy(~fed)].any(), 'an input that feeds no kept output gets an exactly zero gradient'
    return idx, fed, act


def check_tables(dev, kind, R, N, K, C, seed):
    tables = dref.synthetic_tables(R, N, K, seed)
    X, gY = draws((N, C), kind, seed + 1), draws((R, C), kind, seed + 2)
    out, gx = run_pool(dev, kind, synthetic_index(tables, dev), X, gY)
    assert_against_tables(tables, X, gY, out, gx, kind, f'R={R} N={N} K={K} C={C}')


def row_cases(kind):
    """(name, R, C): around the rows one workgroup covers at the narrowest and the widest channel path, past a second workgroup, past the grid"""
    cases = [('rows_0', 0, 16), ('rows_1', 1, 16)]
    for C in (1, 256):
        rows = pool_rows(C, kind)
        cases += [(f'c{C}_rows_minus_1', rows - 1, C), (f'c{C}_rows', rows, C), (f'c{C}_rows_plus_1', rows + 1, C), (f'c{C}_two_workgroups_plus_1', 2 * rows + 1, C)]
    cases.append(('c256_past_the_grid', POOL_MAX_BLOCKS * pool_rows(256, kind) + 1, 256))
    return cases


ROW_CASES = [(kind,) + case for kind in KINDS for case in row_cases(kind)]


def check_values(dev, kind):
    """all-negative inputs (a zero-initialised maximum would show), a window of -inf, one NaN input"""
    geom, C = 'k3s2p1', 16
    coors, idx, _ = case_of(geom)
    index = run_index(geom, dev)
    gY = draws((len(idx['nbr']), C), kind, 31)
    X = draws((len(coors), C), kind, 30, 'negative')
    out, gx = run_pool(dev, kind, index, X, gY)
    want, _, _ = assert_against_tables(idx, X, gY, out, gx, kind, 'negative')
    assert (want < 0).all()
    o = int(np.argmax((idx['nbr'] >= 0).sum(1)))                         # the fullest window: all of its inputs become -inf
    Xi = X.copy()
    Xi[idx['nbr'][o][idx['nbr'][o] >= 0]] = -np.inf
    out_i, gx_i = run_pool(dev, kind, index, Xi, gY)
    assert_against_tables(idx, Xi, gY, out_i, gx_i, kind, '-inf window')
    assert torch.isinf(out_i[o]).all() and (out_i[o] < 0).all() and torch.isfinite(gx_i).all()
    i, c = int(np.argmax((idx['nbr_t'] >= 0).sum(1))), 5                 # the input most windows hold
    Xn = X.copy()
    Xn[i, c] = np.nan
    out_n, gx_n = run_pool(dev, kind, index, Xn, gY)
    assert_against_tables(idx, Xn, gY, out_n, gx_n, kind, 'NaN input')
    hit = np.zeros(want.shape, bool)
    hit[idx['nbr_t'][i][idx['nbr_t'][i] >= 0], c] = True
    assert hit.sum() >= 2 and torch.isnan(out_n[torch.from_numpy(hit)]).all()
    view = torch.int32 if kind == 'fp32' else torch.int16
    keep = torch.from_numpy(~hit)
    assert torch.equal(out_n.view(view)[keep], out.view(view)[keep]), 'every other element keeps the bits of the clean call'
    assert gx_n[i, c] == 0 and not torch.isnan(gx_n).any(), 'a NaN window passes no gradient'


@functools.lru_cache(maxsize=None)
def tied_operands(kind):
    geom, C = 'k3s2p1', 8
    coors, idx, _ = case_of(geom)
    X = draws((len(coors), C), kind, 77, 'integers')
    gY = (np.random.default_rng(78).integers(-3, 4, (len(idx['nbr']), C))).astype(np.float32)
    return idx, X, gY


def check_ties(dev, kind):
    idx, X, gY = tied_operands(kind)
    out, gx = run_pool(dev, kind, run_index('k3s2p1', dev), X, gY)
    want = dref.pool_ref(idx, X)
    wgx, _, _ = dref.unpool_ref(idx, X, want, gY)
    assert np.array_equal(out.double().numpy(), want) and np.array_equal(gx.double().numpy(), wgx), 'small integers sum exactly'


def carve(t, shift):
    """t copied into the middle of a sentinel-filled buffer, `shift` elements past an aligned address -> (buffer, view)"""
    flat = torch.full((t.numel() + 2 * PAD + shift,), S if t.dtype.is_floating_point else -7, dtype=t.dtype, device=t.device)
    view = flat[PAD + shift:PAD + shift + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == (shift * t.element_size()) % 16
    return flat, view


def bands_intact(flat, view, shift):
    n = view.numel()
    lo, hi = flat[:PAD + shift], flat[PAD + shift + n:]
    return bool((lo == S).all() and (hi == S).all()) and hi.numel() == PAD


def run_entries(dev, kind, tables, X, gY, shift, num=None):
    """the two C entries on operands between guard bands, every operand `shift` elements past an aligned address -> (out, gx) on the CPU"""
    dtype, d = dref.DTYPES[kind], torch.device(dev)
    t = lambda a, dt=dtype: torch.from_numpy(np.ascontiguousarray(a)).to(d).to(dt)
    (N, C), (R, K) = X.shape, tables['nbr'].shape
    bufs = {k: carve(v, shift) for k, v in dict(x=t(X), gy=t(gY), nbr=t(tables['nbr'], torch.int32), nbr_t=t(tables['nbr_t'], torch.int32),
                                                  out=torch.full((R, C), S, dtype=dtype, device=d), gx=torch.full((N, C), S, dtype=dtype, device=d)).items()}
    p = {k: v[1].data_ptr() for k, v in bufs.items()}
    numt = None if num is None else torch.tensor([num, num], dtype=torch.int64, device=d)
    _host.call('gd3d_sparse_max_pool_forward', d, (p['x'], p['nbr'], _host.ptr(numt), N, R, K, C, dref.CODES[kind], p['out']))
    _host.call('gd3d_sparse_max_pool_backward', d, (p['gy'], p['x'], p['out'], p['nbr_t'], N, R, K, C, dref.CODES[kind], p['gx']))
    for k in ('out', 'gx', 'x', 'gy'):
        assert bands_intact(*bufs[k], shift), f'{k}: a guard band was written ({kind}, shift {shift})'
    return bufs['out'][1].cpu().clone(), bufs['gx'][1].cpu().clone()


def check_guards_and_alignment(dev, kind, C):
    """a static index far above the count (whole workgroups of dead rows) between guard bands, aligned and one element off: the same bits,
    and the bits of the call through `sparse_max_pool`"""
    coors, idx, mo = case_of('k3s2p1', 'above')
    kept = int(idx['num'][0])
    assert mo - kept >= 2 * pool_rows(C, kind) or C > 16
    X, gY = draws((len(coors), C), kind, 50 + C), draws((mo, C), kind, 51 + C)
    aligned = run_entries(dev, kind, idx, X, gY, 0, num=kept)
    shifted = run_entries(dev, kind, idx, X, gY, 1, num=kept)
    api = run_pool(dev, kind, run_index('k3s2p1', dev, 'above'), X, gY)
    for a, b, c in zip(aligned, shifted, api):
        assert same_bits(a, b) and same_bits(a, c)
    assert not aligned[0][kept:].any() and aligned[0][:kept].all()
    assert_against_tables(idx, X, gY, *aligned, kind, f'guards C={C}')


def check_bad_arguments():
    """BADARG / TOOLARGE before any launch, from the device entries and the twins alike"""
    lib = _lib.load()
    buf = torch.zeros(4096, dtype=torch.float32)
    tab = torch.full((64,), -1, dtype=torch.int32)
    p, q = buf.data_ptr(), tab.data_ptr()
    BADARG, TOOLARGE = 10001, 10002
    for fwd, bwd, tail in ((lib.gd3d_sparse_max_pool_forward, lib.gd3d_sparse_max_pool_backward, (None,)),
                           (lib.gd3d_sparse_max_pool_forward_cpu, lib.gd3d_sparse_max_pool_backward_cpu, ())):
        assert fwd(None, q, None, 4, 4, 8, 4, 0, p, *tail) == BADARG and fwd(p, None, None, 4, 4, 8, 4, 0, p, *tail) == BADARG
        assert fwd(p, q, None, 4, 4, 8, 4, 0, None, *tail) == BADARG and fwd(p, q, None, 4, 4, 8, 0, 0, p, *tail) == BADARG
        assert fwd(p, q, None, 4, 4, 8, 257, 0, p, *tail) == TOOLARGE and fwd(p, q, None, 4, 4, 28, 4, 0, p, *tail) == TOOLARGE
        assert fwd(p, q, None, 4, 4, 0, 4, 0, p, *tail) == BADARG and fwd(p, q, None, 4, 4, 8, 4, 3, p, *tail) == BADARG
        assert fwd(p, q, None, -1, 4, 8, 4, 0, p, *tail) == BADARG and fwd(p, q, None, 4, 1 << 31, 8, 4, 0, p, *tail) == TOOLARGE
        assert fwd(p + 2, q, None, 4, 4, 8, 4, 0, p, *tail) == BADARG      # fp32 at an odd half-word
        assert bwd(None, p, p, q, 4, 4, 8, 4, 0, p, *tail) == BADARG and bwd(p, None, p, q, 4, 4, 8, 4, 0, p, *tail) == BADARG
        assert bwd(p, p, None, q, 4, 4, 8, 4, 0, p, *tail) == BADARG and bwd(p, p, p, None, 4, 4, 8, 4, 0, p, *tail) == BADARG
        assert bwd(p, p, p, q, 4, 4, 8, 4, 0, None, *tail) == BADARG and bwd(p, p, p, q, 4, 4, 8, 0, 0, p, *tail) == BADARG
        assert bwd(p, p, p, q, 4, 4, 8, 257, 0, p, *tail) == TOOLARGE and bwd(p, p, p, q, 4, 4, 28, 4, 0, p, *tail) == TOOLARGE
        assert fwd(None, None, None, 0, 0, 8, 4, 0, None, *tail) == 0 and bwd(None, None, None, None, 0, 0, 8, 4, 0, None, *tail) == 0
    assert not buf.any()


def check_module(dev):
    shape, kernel, stride, padding = GEOMS['k3s2p1']
    coors, idx, _ = case_of('k3s2p1')
    x = amd.SparseConvTensor(torch.from_numpy(draws((len(coors), 6), 'fp32', 3)).to(dev), torch.from_numpy(coors).to(dev), shape, B)
    pool = amd.SparseMaxPool3d(3, 2, 1)
    y = pool(x)
    assert np.array_equal(y.indices.cpu().numpy(), idx['out_coors']) and tuple(y.spatial_shape) == tuple(idx['out_shape']) and y.indice_dict is x.indice_dict
    assert np.array_equal(y.features.double().cpu().numpy(), dref.pool_ref(idx, x.features.double().cpu().numpy())) and not x.indice_dict
    static = amd.SparseMaxPool3d(kernel, stride, padding, max_out=len(idx['nbr']) + 20)(x)
    assert static.features.shape[0] == len(idx['nbr']) + 20 and torch.equal(static.features[:len(idx['nbr'])], y.features) and not static.features[len(idx['nbr']):].any()
    wide = amd.sparse_max_pool(x.features.double(), amd.sparse_conv_index(x.indices, shape, B, kernel, stride, padding))      # another dtype goes through fp32
    assert wide.dtype == torch.float64 and torch.equal(wide, y.features.double())
    subm = amd.sparse_conv_index(x.indices, shape, B, 3, 1, 1, True)
    bad = [lambda: amd.SparseMaxPool3d(3, 2, 1, dilation=2), lambda: amd.SparseMaxPool3d(4), lambda: pool(x.features), lambda: amd.sparse_max_pool(x.features, subm),
           lambda: amd.sparse_max_pool(x.features[:-1], amd.sparse_conv_index(x.indices, shape, B, kernel, stride, padding)),
           lambda: amd.sparse_max_pool(x.features.int(), amd.sparse_conv_index(x.indices, shape, B, kernel, stride, padding))]
    for i, call in enumerate(bad):
        with pytest.raises(RuntimeError):
            call()
            pytest.fail(f'call {i} did not raise')


# ---- the tests -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('geom', sorted(GEOMS))
def test_every_window_size_bit_equal_to_the_dense_max_pool(geom, kind):
    check_geometry('cpu', kind, geom, 16)


@pytest.mark.parametrize('kind,C', [(k, c) for k in KINDS for c in CHANNELS[k]])
def test_every_channel_path(kind, C):
    check_geometry('cpu', kind, 'k2s2', C)


@pytest.mark.parametrize('kind,name,R,C', ROW_CASES, ids=lambda v: str(v))
def test_row_counts_around_a_workgroup_and_past_the_grid(kind, name, R, C):
    check_tables('cpu', kind, R, R + 3, 2, C, 400 + R % 89)


def test_the_cases_hold_what_they_claim():
    assert pool_rows(1, 'fp32') == 256 and pool_rows(256, 'fp32') == 4 and pool_rows(256, 'bf16') == 8 and pool_rows(5, 'fp32') == 51 and pool_rows(24, 'fp16') == 85
    assert [dref.synthetic_tables(5, 8, k, 0)['nbr'].shape[1] for k in (1, 8, 27)] == [1, 8, 27]
    assert [case_of(g)[1]['nbr'].shape[1] for g in sorted(GEOMS)] == [1, 8, 27, 27]
    _, idx, mo = case_of('k3s2p1', 'below')
    assert idx['num'][0] == mo < idx['num'][1]
    act = ref.active_rows(case_of('k3s2p1', 'below')[0], GEOMS['k3s2p1'][0], B)
    assert (act & ~(idx['nbr_t'] >= 0).any(1)).any(), 'active inputs that feed only dropped outputs'
    for kind in KINDS:                                                   # the committed seed: at least a quarter of the windows hold a tie
        idx, X, _ = tied_operands(kind)
        want = dref.pool_ref(idx, X)
        valid = idx['nbr'] >= 0
        at_max = (valid[:, :, None] & (X[np.maximum(idx['nbr'], 0)] == want[:, None, :])).sum(1)
        assert (at_max >= 2).mean() >= 0.25, (at_max >= 2).mean()


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('form', ['above', 'below', 'inactive'])
def test_dead_rows_static_tail_dropped_outputs_and_nan_in_inactive_rows(form, kind):
    if form == 'inactive':
        idx, fed, act = check_geometry('cpu', kind, 'k3s2p1', 16, inactive=True)
        assert (~act).sum() >= 31
    else:
        idx, fed, act = check_geometry('cpu', kind, 'k3s2p1', 16, max_out=form)
        assert (form == 'above') == bool(fed.all())


@pytest.mark.parametrize('kind', KINDS)
def test_negative_inputs_an_inf_window_and_one_nan(kind):
    check_values('cpu', kind)


@pytest.mark.parametrize('kind', KINDS)
def test_every_tied_input_receives_the_gradient(kind):
    check_ties('cpu', kind)


def test_untied_gradient_equals_torch_autograd_through_the_dense_pool():
    shape, kernel, stride, padding = GEOMS['k3s2p1']
    coors, idx, _ = case_of('k3s2p1')
    X, gY = draws((len(coors), 4), 'fp32', 60).astype(np.float64), draws((len(idx['nbr']), 4), 'fp32', 61).astype(np.float64)
    c, oc = torch.from_numpy(coors.astype(np.int64)), torch.from_numpy(idx['out_coors'].astype(np.int64))
    x = torch.tensor(X, requires_grad=True)
    dense = torch.full((B,) + shape + (4,), -np.inf, dtype=torch.float64).index_put((c[:, 0], c[:, 1], c[:, 2], c[:, 3]), x)
    y = F.max_pool3d(dense.permute(0, 4, 1, 2, 3), kernel, stride, padding)[oc[:, 0], :, oc[:, 1], oc[:, 2], oc[:, 3]]
    (g,) = torch.autograd.grad(y, x, torch.from_numpy(gY))
    want = dref.pool_ref(idx, X)
    assert np.array_equal(y.detach().numpy(), want)
    assert np.allclose(dref.unpool_ref(idx, X, want, gY)[0], g.numpy(), rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('C', [16, 20])
def test_c_entries_between_guard_bands_aligned_and_one_element_off(C, kind):
    check_guards_and_alignment('cpu', kind, C)


def test_bad_arguments_return_codes_without_a_launch():
    check_bad_arguments()


def test_module_static_form_and_bad_arguments():
    check_module('cpu')
