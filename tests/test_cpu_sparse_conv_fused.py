"""The fused sparse convolution layer on the CPU (gd3d_sparse_conv_forward_fused[_16]_cpu): conv -> * scale + shift ->
+ residual -> ReLU in one call, in fp32, fp16 and bf16, on a named subset of the cases of tests/sparse_conv_ref.py and
tests/sparse_conv_16_cases.py.

* the oracle   pre = the fp64 oracle's `out` with bias=None (on the operands rounded to the 16-bit type, residual included, for fp16 /
               bf16); want = act(pre * scale + shift' + residual) in fp64, zero on the rows without a neighbour.  The value cases run
               without the conv's own bias (shift' = shift: a standard normal bias would decide the sign of most outputs of a channel);
               that the host folds it, shift' = bias * scale + shift in fp32, is held bit for bit against the call that is handed shift'.
* the bounds   A' = A |scale| + |shift'| + |residual| with A the convolution of absolute values.  fp32: (L + 4) u A', L the term count
               without the bias; the two extra terms are the fma and the residual add; the ReLU is exact and 1-Lipschitz.  16-bit:
               E + u16 (|want| + E) + s, E = 2 (L + 4) u A', u16 and s as in `within_bound_16`.  Derived, not tuned.
* the rest     the same bits from run to run; bit identity with the plain entry; dead rows exactly zero under shift 3.0 and a NaN
               residual; the C entries between guard bands, aligned and with the residual alone shifted by one element; act = 2;
               non-finite values; the gradients against the fp64 chain; `fuse_sparse_conv_bn` on the encoders, layer by layer.
tests/test_gpu_sparse_conv_fused.py runs the same helpers on the device."""
import copy
import functools
import itertools

import numpy as np
import pytest
import torch

import mmdet3d_gaussian_amd as amd
import sparse_conv_16_cases as c16
import sparse_conv_ref as ref
from mmdet3d_gaussian_amd import _lib
from test_cpu_sparse_conv import ENC_B, ENC_SHAPES, build_encoder, count_calls, encoder_inputs, run_index

KINDS = ('fp32', 'fp16', 'bf16')
DTYPES = dict(c16.DTYPES, fp32=None)                                     # the compute_dtype of a kind
WIDE = ref.MORE_GEOM_CASES['k233s212']                                   # 72 -> 136: a second and a third column tile
FUSED_CASES = ('subm_9x12x10_c4_16', 's2p011_7x11x13_c3_7', 'down_7x11x13_c16_32', 's2p1_channel_tiles_c24_40', 'subm_channel_tiles_c32_32',
               'subm_7x11x13_c64_64', WIDE, 'subm_inactive_rows_scattered_and_tail', 's2p1_max_out_below', 's2p1_max_out_above',
               'subm_inactive_block', 's2p1_max_out_far_above', '16:subm_rows_wave_plus_1', '16:s2p1_rows_tile16_plus_1')
DEAD_CASES = ('subm_inactive_rows_scattered_and_tail', 's2p1_max_out_above', 'subm_inactive_block', 's2p1_max_out_far_above')
COMBOS = tuple(itertools.product((True, False), (True, False), (None, 'relu')))      # scale given, residual given, activation
S = -77.0                                                                # the sentinel of the guard test: exact in every type


def rounded(a, kind):
    """an fp32 array in fp64, after rounding to the kind's 16-bit type if it has one"""
    return np.asarray(a, np.float64) if kind == 'fp32' else c16.rounded(a, kind)


@functools.lru_cache(maxsize=None)
def fused_operands(name):
    """scale (Cout) of both signs, shift (Cout), residual (R, Cout): fp32 normal draws, fixed by the case's seed.  The shift's spread is
    0.1, below that of pre * scale and of the residual (1): the sign of pre * scale + shift + residual is not decided per channel, and
    about half the pre-activations are negative"""
    case, idx = c16.case_of(name), c16.expected_index(name)
    rng = np.random.default_rng(5000 + case['seed'])
    scale = rng.standard_normal(case['cout']).astype(np.float32)
    shift = (0.1 * rng.standard_normal(case['cout'])).astype(np.float32)
    residual = rng.standard_normal((len(idx['nbr']), case['cout'])).astype(np.float32)
    assert (scale > 0).any() and (scale < 0).any()
    return scale, shift, residual


@functools.lru_cache(maxsize=None)
def expected_pre(name, kind):
    """-> (pre, A, L, live): the fp64 oracle's out with bias=None on the (rounded) operands, the same on absolute values, the term counts
    without the bias, the rows that have a neighbour; computed once and shared, never modified"""
    case, idx = c16.case_of(name), c16.expected_index(name)
    X, W, _, gY = c16.operands(name)
    o64, A = c16.oracle_on(case, idx, rounded(X, kind), rounded(W, kind), None, np.zeros(gY.shape))
    L = ref.term_counts(idx, len(X), case['cin'], case['cout'], False)['out']
    return o64['out'], A['out'], L, (idx['nbr'] >= 0).any(1)


def folded_shift(bias, scale, shift):
    """shift' = bias * scale + shift in fp32, in the host's order (a product, then a sum; None where nothing is left)"""
    if bias is None:
        return shift
    b = bias if scale is None else bias * scale
    return b if shift is None else b + shift


def expected_fused(name, kind, with_scale, with_residual, activation, with_bias=False):
    """-> (want, A'): act(pre * scale + shift' + residual) in fp64, zero on the rows without a neighbour, and the scale of its terms"""
    pre, A, _, live = expected_pre(name, kind)
    bias = c16.operands(name)[2] if with_bias else None
    scale, shift, residual = fused_operands(name)
    sc = scale if with_scale else None
    sh = folded_shift(bias, sc, shift).astype(np.float64)
    t, a = (pre * sc.astype(np.float64), A * np.abs(sc.astype(np.float64))) if with_scale else (pre, A)
    t, a = t + sh, a + np.abs(sh)
    if with_residual:
        r = rounded(residual, kind)
        t, a = t + r, a + np.abs(r)
    if activation == 'relu':
        t = np.maximum(t, 0.0)
    return t * live[:, None], a * live[:, None]


def within_fused_bound(got, want, scale, L, kind):
    """-> (the bound holds everywhere, the worst |got - want| / A')"""
    err = np.abs(np.asarray(got, np.float64) - want)
    if kind == 'fp32':
        ok = bool((err <= (L + 4) * ref.U * scale).all())
    else:
        E = 2 * (L + 4) * ref.U * scale
        ok = bool((err <= E + c16.U16[kind] * (np.abs(want) + E) + c16.SUB[kind]).all())
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(scale > 0, err / scale, 0.0)
    return ok, float(ratio.max()) if ratio.size else 0.0


def tensors_of(name, dev, kind):
    """X, W in the kind's type, bias fp32 (or None), scale, shift fp32, residual in the kind's type, on dev"""
    dtype = DTYPES[kind] or torch.float32
    X, W, bias, _ = c16.operands(name)
    scale, shift, residual = fused_operands(name)
    t = lambda a, dt=torch.float32: None if a is None else torch.from_numpy(a).to(dev).to(dt)
    return t(X, dtype), t(W, dtype), t(bias), t(scale), t(shift), t(residual, dtype)


def run_fused(name, dev, kind, with_scale, with_residual, activation, index=None):
    """the fused call through `amd.sparse_conv` -> (R, Cout) fp32 numpy (exact: the 16-bit values widen without rounding)"""
    X, W, bias, scale, shift, residual = tensors_of(name, dev, kind)
    index = run_index(c16.case_of(name), dev) if index is None else index
    out = amd.sparse_conv(X, W, None, index, DTYPES[kind], scale=scale if with_scale else None, shift=shift,
                          residual=residual if with_residual else None, activation=activation)
    assert out.dtype == (DTYPES[kind] or torch.float32)
    return out.float().cpu().numpy()


def check_fused_values(name, dev, kind):
    """every combination of {scale given or not} x {residual given or not} x {none, relu}: within the derived bound of the fp64 oracle, zero on
    the rows without a neighbour, the same bits from run to run; under the ReLU 25 % .. 75 % of the live outputs are clipped"""
    _, _, L, live = expected_pre(name, kind)
    index = run_index(c16.case_of(name), dev)
    for with_scale, with_residual, activation in COMBOS:
        want, scale = expected_fused(name, kind, with_scale, with_residual, activation)
        who = f'{name} {kind} on {dev} (scale {with_scale}, residual {with_residual}, {activation})'
        if activation == 'relu':
            clipped = float((want[live] == 0).mean())
            assert 0.25 <= clipped <= 0.75, f'{who}: {clipped:.2f} of the live outputs are clipped: the ReLU is not under test'
        got = run_fused(name, dev, kind, with_scale, with_residual, activation, index)
        assert got.shape == want.shape, who
        ok, worst = within_fused_bound(got, want, scale, L, kind)
        print(f'{who}: worst |ours - o64| / A\' = {worst:.3e} (L up to {int(np.max(L, initial=0))})')
        assert ok, f'{who}: misses its bound: worst ratio {worst:.3e}'
        assert not got[~live].any(), f'{who}: a row without neighbours is not zero'
        again = run_fused(name, dev, kind, with_scale, with_residual, activation, index)
        assert got.tobytes() == again.tobytes(), f'{who}: differs from run to run'


def check_bit_identity(name, dev, kind):
    """shift = bias with nothing else, and the same with a scale of ones, give the bits of the plain entry"""
    X, W, bias, _, _, _ = tensors_of(name, dev, kind)
    index = run_index(c16.case_of(name), dev)
    plain = amd.sparse_conv(X, W, bias, index, DTYPES[kind])
    assert torch.equal(amd.sparse_conv(X, W, None, index, DTYPES[kind], shift=bias), plain), f'{name} {kind}: shift = bias'
    assert torch.equal(amd.sparse_conv(X, W, None, index, DTYPES[kind], scale=torch.ones_like(bias), shift=bias), plain), f'{name} {kind}: scale = ones'
    assert torch.equal(amd.sparse_conv(X, W, bias, index, DTYPES[kind], scale=torch.ones_like(bias)), plain), f'{name} {kind}: the folded bias'
    assert plain.any()
    _, _, _, scale, shift, residual = tensors_of(name, dev, kind)         # the conv's own bias is folded on the host: shift' = bias * scale + shift
    folded = amd.sparse_conv(X, W, bias, index, DTYPES[kind], scale=scale, shift=shift, residual=residual, activation='relu')
    assert torch.equal(folded, amd.sparse_conv(X, W, None, index, DTYPES[kind], scale=scale, shift=bias * scale + shift, residual=residual, activation='relu'))
    assert not torch.equal(folded, amd.sparse_conv(X, W, None, index, DTYPES[kind], scale=scale, shift=shift, residual=residual, activation='relu'))


def check_dead_rows(name, dev, kind):
    """the rows without a neighbour are exactly zero when shift is 3.0 and the residual there is NaN; the live rows stay finite"""
    X, W, bias, scale, _, residual = tensors_of(name, dev, kind)
    live = torch.from_numpy((c16.expected_index(name)['nbr'] >= 0).any(1)).to(dev)
    assert 0 < int(live.sum()) < len(live)
    residual = residual.clone()
    residual[~live] = float('nan')
    index = run_index(c16.case_of(name), dev)
    for activation in (None, 'relu'):
        out = amd.sparse_conv(X, W, bias, index, DTYPES[kind], scale=scale, shift=torch.full_like(scale, 3.0), residual=residual, activation=activation)
        assert torch.equal(out[~live], torch.zeros_like(out[~live])), f'{name} {kind}: a dead row is not exactly zero'
        assert torch.isfinite(out[live]).all() and out[live].any()


def run_entry_between_bands(name, dev, kind, res_shift, act=1):
    """the C entry on a sentinel-filled output with a guard band either side; the residual's base `res_shift` elements past an aligned
    address.  -> (rc, the band-free part as fp32 numpy, whether the bands are untouched)"""
    X, W, bias, scale, shift, residual = tensors_of(name, dev, kind)
    index = run_index(c16.case_of(name), dev)
    N, (K, Cin, Cout), R, G = len(X), W.shape, len(residual), 64
    res = torch.empty(residual.numel() + 8, dtype=residual.dtype, device=dev)
    res[res_shift:res_shift + residual.numel()] = residual.flatten()
    out = torch.full((R * Cout + 2 * G,), S, dtype=residual.dtype, device=dev)
    assert res.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    lib, cuda, size = _lib.load(), torch.device(dev).type == 'cuda', residual.element_size()
    fn = getattr(lib, 'gd3d_sparse_conv_forward_fused' + ('' if kind == 'fp32' else '_16') + ('' if cuda else '_cpu'))
    code = () if kind == 'fp32' else ({'fp16': 1, 'bf16': 2}[kind],)
    tail = (torch.cuda.current_stream().cuda_stream,) if cuda else ()
    rc = fn(X.data_ptr(), W.data_ptr(), scale.data_ptr(), shift.data_ptr(), res.data_ptr() + size * res_shift, index.nbr.data_ptr(), index.num.data_ptr(),
            N, R, K, Cin, Cout, act, *code, out.data_ptr() + size * G, *tail)
    if cuda:
        torch.cuda.synchronize()
    bands = bool((out[:G] == S).all() and (out[G + R * Cout:] == S).all())
    return rc, out[G:G + R * Cout].float().cpu().numpy().reshape(R, Cout), bands


def check_guards(name, dev, kind):
    """aligned, then the residual alone shifted by one element: the bands stay untouched, every element is written and within the bound,
    and the shifted call gives the aligned call's bits; act = 2 is refused and writes nothing"""
    want, scale = expected_fused(name, kind, True, True, 'relu')
    L = expected_pre(name, kind)[2]
    rc, aligned, bands = run_entry_between_bands(name, dev, kind, 0)
    assert rc == 0 and bands, f'{name} {kind}: rc {rc}, bands untouched: {bands}'
    ok, worst = within_fused_bound(aligned, want, scale, L, kind)
    assert ok, f'{name} {kind}: the C entry misses its bound (a sentinel survives?): worst ratio {worst:.3e}'
    rc, shifted, bands = run_entry_between_bands(name, dev, kind, 1)
    assert rc == 0 and bands and shifted.tobytes() == aligned.tobytes(), f'{name} {kind}: a misaligned residual changes the result'
    rc, untouched, bands = run_entry_between_bands(name, dev, kind, 0, act=2)
    assert rc == 10001 and bands and (untouched == S).all(), f'{name} {kind}: act = 2 must return GD3D_E_BADARG and write nothing'


def check_nonfinite(dev, kind):
    """a NaN in one residual row poisons that row only; in fp16 a value beyond the range is inf under NONE and under RELU, -inf is 0 under RELU"""
    name = 'subm_9x12x10_c4_16'
    X, W, bias, scale, shift, residual = tensors_of(name, dev, kind)
    index = run_index(c16.case_of(name), dev)
    live = (c16.expected_index(name)['nbr'] >= 0).any(1)
    assert live.all()
    o = 17
    dirty = residual.clone()
    dirty[o, 3] = float('nan')
    for activation in (None, 'relu'):
        run = lambda r: amd.sparse_conv(X, W, bias, index, DTYPES[kind], scale=scale, shift=shift, residual=r, activation=activation).float()
        clean, got = run(residual), run(dirty)
        assert torch.isfinite(clean).all()
        rest = torch.ones_like(got, dtype=torch.bool)
        rest[o, 3] = False
        assert torch.isnan(got[o, 3]) and torch.equal(got[rest], clean[rest]), f'{kind} {activation}: the NaN left its element or did not pass'
    if kind == 'fp16':
        big = torch.full_like(shift, 1e6)
        for sign, activation, value in ((1, None, float('inf')), (1, 'relu', float('inf')), (-1, None, float('-inf')), (-1, 'relu', 0.0)):
            out = amd.sparse_conv(X, W, None, index, DTYPES[kind], shift=sign * big, residual=residual, activation=activation)
            assert torch.equal(out.float(), torch.full(out.shape, value, device=out.device)), (sign, activation)


def check_gradients(name, dev, kind):
    """gx, gw, gb and grad_residual against the fp64 chain: g = grad_out * (out > 0), grad_residual = g exactly, and the three others at
    the existing gradient bounds with g * scale (as the host computes it, in fp32, rounded to the 16-bit type on that path) as the operand"""
    case, idx = c16.case_of(name), c16.expected_index(name)
    X, W, bias, scale, shift, residual = tensors_of(name, dev, kind)
    gY = torch.from_numpy(c16.operands(name)[3]).to(dev).to(X.dtype)
    index = run_index(case, dev)
    x, w, b, r = (t.clone().requires_grad_(True) for t in (X, W.float(), bias, residual))
    out = amd.sparse_conv(x, w, b, index, DTYPES[kind], scale=scale, shift=shift, residual=r, activation='relu')
    gx, gw, gb, gr = torch.autograd.grad(out, [x, w, b, r], gY)
    want, _ = expected_fused(name, kind, True, True, 'relu', with_bias=True)
    mask = out.detach().float().cpu().numpy() > 0
    assert np.array_equal(mask, want > 0), f'{name} {kind}: an output within rounding of zero: the ReLU masks differ, pick another case'
    g = gY.float().cpu().numpy() * mask                                  # exact
    assert gr.dtype == residual.dtype and np.array_equal(gr.float().cpu().numpy(), g), f'{name} {kind}: grad_residual is not grad_out * (out > 0)'
    gyc = g * fused_operands(name)[0]                                    # fp32 x fp32 in fp32: the host's one rounding
    assert gyc.dtype == np.float32
    Xn, Wn = c16.operands(name)[:2]
    o64, A = c16.oracle_on(case, idx, rounded(Xn, kind), rounded(Wn, kind), np.zeros(case['cout']), rounded(gyc, kind))
    L = ref.term_counts(idx, len(Xn), case['cin'], case['cout'], True)
    assert gx.dtype == X.dtype and gw.dtype == torch.float32 and gb.dtype == torch.float32
    for k, t in (('gx', gx), ('gw', gw), ('gb', gb)):
        got = t.float().cpu().numpy()
        if k == 'gx' and kind != 'fp32':
            ok, worst = c16.within_bound_16(got, o64[k], A[k], L[k], kind)
        else:
            ok, worst = ref.within_bound(got, o64[k], A[k], L[k])
        print(f'{name} {kind} on {dev}: {k}: worst |ours - o64| / A = {worst:.3e}')
        assert ok and np.abs(got).sum() > 0, f'{name} {kind}: {k} misses its bound on {dev}: worst ratio {worst:.3e}'


# ---- the modules -----------------------------------------------------------------------------------------------------------------------

BASIC = dict(block_type='basicblock', encoder_channels=((16, 16, 32), (32, 32, 64), (64, 64, 128), (128, 128)),
             encoder_paddings=((0, 0, 1), (0, 0, 1), (0, 0, (0, 1, 1)), (0, 0)))
ENC_GRID = min(ENC_SHAPES, key=lambda s: s[0] * s[1] * s[2])


def randomise_batchnorms(module, seed):
    """running statistics and affine parameters a trained model would hold: nothing shows with mean 0, var 1, gamma 1, beta 0"""
    gen = torch.Generator().manual_seed(seed)
    for m in module.modules():
        if isinstance(m, torch.nn.BatchNorm1d):
            m.running_mean.copy_(torch.randn(m.num_features, generator=gen) * 0.1)
            m.running_var.copy_(torch.rand(m.num_features, generator=gen) + 0.5)
            m.weight.data.copy_((torch.rand(m.num_features, generator=gen) + 0.5) * (torch.randint(0, 2, (m.num_features,), generator=gen) * 2 - 1))
            m.bias.data.copy_(torch.randn(m.num_features, generator=gen) * 0.1)
    return module


def build_fusable_encoder(dev, block_type, kind):
    """MlvlSparseEncoder in eval() with randomised BatchNorms: `build_encoder`'s for conv_module in fp32, the same recipe otherwise"""
    if block_type == 'conv_module' and kind == 'fp32':
        return build_encoder(dev, ENC_GRID)
    torch.manual_seed(6)
    enc = amd.MlvlSparseEncoder(in_channels=4, sparse_shape=list(ENC_GRID), order=('conv', 'norm', 'act'), compute_dtype=DTYPES[kind],
                                **(BASIC if block_type == 'basicblock' else {}))
    return randomise_batchnorms(enc, 7).to(dev).eval()


def check_fused_encoder(dev, block_type, kind, monkeypatch):
    coors, feats = encoder_inputs(ENC_GRID)
    enc = build_fusable_encoder(dev, block_type, kind)
    fused = copy.deepcopy(enc)
    assert fused.fuse() is fused
    layers = [m for m in fused.modules() if isinstance(m, amd.FusedSparseConv)]
    norms = [m for m in enc.modules() if isinstance(m, torch.nn.BatchNorm1d)]
    blocks = [m for m in fused.modules() if isinstance(m, amd.FusedSparseBasicBlock)]
    assert len(layers) == len(norms) == dict(conv_module=12, basicblock=21)[block_type] and len(blocks) == dict(conv_module=0, basicblock=8)[block_type]
    assert not any(isinstance(m, (torch.nn.BatchNorm1d, torch.nn.ReLU, amd.SparseBasicBlock)) for m in fused.modules())
    for layer, bn in zip(layers, norms):                                 # fp64, kept in fp32
        s = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
        assert layer.scale.dtype == torch.float32 and torch.equal(layer.scale, s.float()) and torch.equal(layer.shift, (bn.bias.detach().double() - bn.running_mean.double() * s).float())
        assert layer.activation == 'relu' and layer.compute_dtype == DTYPES[kind] and 'indice_key' in layer.extra_repr() and 'max_out' in layer.extra_repr()
        assert (DTYPES[kind] is None) == ('compute_dtype' not in layer.extra_repr())
    seen = []
    hooks = [m.register_forward_hook(lambda mod, args, kwargs, out: seen.append((mod, args[0].features.detach(), args[0].indices, list(args[0].spatial_shape),
                                                                                 kwargs.get('residual'), out.features.detach())), with_kwargs=True) for m in layers]
    x, c = torch.from_numpy(feats).to(dev), torch.from_numpy(coors).to(dev)
    calls = count_calls(monkeypatch)
    with torch.no_grad():
        got, want = fused(x, c, ENC_B), enc(x, c, ENC_B)
    for h in hooks:
        h.remove()
    entry = 'gd3d_sparse_conv_forward_fused' + ('' if kind == 'fp32' else '_16')
    assert calls[entry] == len(layers) and len(seen) == len(layers), calls       # one fused entry a fused layer
    assert calls['gd3d_sparse_conv_forward' + ('' if kind == 'fp32' else '_16')] == len(layers), calls      # the unfused encoder's
    assert got['spatial_features'].shape == want['spatial_features'].shape and got['spatial_features'].dtype == want['spatial_features'].dtype
    assert [f.features.shape for f in got['encode_features']] == [f.features.shape for f in want['encode_features']]
    assert all(a[0] is b for a, b in zip(seen, layers))                  # the layers run in the order `modules()` lists them
    worst, with_residual = 0.0, 0
    for (layer, xin, cin, shape, residual, y), bn in zip(seen, norms):
        conv = layer.conv
        idx = ref.index_ref(cin.cpu().numpy(), shape, ENC_B, conv.kernel_size, conv.stride, conv.padding, conv.subm)
        if len(idx['nbr']) == 0:                                         # the kernel does not fit the grid: no output cell
            assert y.shape[0] == 0
            continue
        cast = (lambda t: t.detach().double().cpu().numpy()) if kind == 'fp32' else (lambda t: t.detach().to(DTYPES[kind]).double().cpu().numpy())
        X, W = cast(xin), cast(conv.weight).reshape(-1, conv.in_channels, conv.out_channels)
        zeros = np.zeros((len(idx['nbr']), conv.out_channels))
        pre = ref.sparse_oracle(idx, X, W, None, zeros)['out']
        A = ref.sparse_oracle(idx, np.abs(X), np.abs(W), None, zeros)['out']
        L = ref.term_counts(idx, len(X), conv.in_channels, conv.out_channels, False)['out']
        s = bn.weight.detach().double().cpu().numpy() / np.sqrt(bn.running_var.double().cpu().numpy() + bn.eps)
        sh = bn.bias.detach().double().cpu().numpy() - bn.running_mean.double().cpu().numpy() * s
        t, a = pre * s + sh, A * np.abs(s) + np.abs(sh)                  # the unfused modules on that input, in fp64
        if residual is not None:
            with_residual += 1
            t, a = t + cast(residual), a + np.abs(cast(residual))
        live = (idx['nbr'] >= 0).any(1)
        assert live.all()
        ok, ratio = within_fused_bound(y.float().cpu().numpy(), np.maximum(t, 0.0), a, L, kind)
        worst = max(worst, ratio)
        assert ok, f'{layer}: the fused output misses its bound: worst |ours - o64| / A\' = {ratio:.3e}'
    assert with_residual == len(blocks)
    print(f'fused MlvlSparseEncoder ({block_type}, {kind}) on {dev}: worst |ours - o64| / A\' over the layers {worst:.3e}')


# ---- the tests -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', FUSED_CASES)
def test_fused_twin_within_the_derived_bound_in_every_combination(name, kind):
    check_fused_values(name, 'cpu', kind)


def test_the_fused_cases_hold_what_they_claim():
    assert len(set(FUSED_CASES)) == 14 and c16.case_of(WIDE)['cout'] > 64 and c16.case_of(WIDE)['cout'] % 8 == 0
    assert c16.case_of('s2p011_7x11x13_c3_7')['cout'] % 4 != 0            # element-wise stores and residual loads on both paths
    assert 64 * (27 * 64 + 8) * 2 > 32 << 10                              # subm_7x11x13_c64_64: the 16-bit weight slab is staged in chunks
    for name in DEAD_CASES:
        live = (c16.expected_index(name)['nbr'] >= 0).any(1)
        assert 0 < live.sum() < len(live), name
    assert len(COMBOS) == 8


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', ['subm_9x12x10_c4_16', 's2p011_7x11x13_c3_7', 's2p1_channel_tiles_c24_40', 'subm_7x11x13_c64_64'])
def test_shift_alone_and_a_scale_of_ones_give_the_plain_entrys_bits(name, kind):
    check_bit_identity(name, 'cpu', kind)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', DEAD_CASES)
def test_dead_rows_are_exactly_zero_under_a_shift_and_a_nan_residual(name, kind):
    check_dead_rows(name, 'cpu', kind)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', ['subm_channel_tiles_c32_32', 's2p011_7x11x13_c3_7', 's2p1_max_out_above'])
def test_c_entries_between_bands_with_the_residual_aligned_and_shifted(name, kind):
    check_guards(name, 'cpu', kind)


@pytest.mark.parametrize('kind', KINDS)
def test_non_finite_values_pass_and_stay_where_they_are(kind):
    check_nonfinite('cpu', kind)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', ['subm_9x12x10_c4_16', 's2p1_9x12x10_c5_16'])
def test_gradients_follow_the_fp64_chain(name, kind):
    check_gradients(name, 'cpu', kind)


def test_bad_arguments_raise():
    name = 'subm_9x12x10_c4_16'
    X, W, bias, scale, shift, residual = tensors_of(name, 'cpu', 'fp32')
    index = run_index(c16.case_of(name), 'cpu')
    for kw in (dict(scale=scale.clone().requires_grad_(True)), dict(shift=shift.clone().requires_grad_(True))):
        with pytest.raises(RuntimeError, match='must not require grad'):
            amd.sparse_conv(X, W, bias, index, **kw)
    for kw in (dict(scale=scale[:-1]), dict(shift=shift[None]), dict(residual=residual[:-1]), dict(residual=residual[:, :-1]), dict(scale=scale.long())):
        with pytest.raises(RuntimeError, match='shape mismatch'):
            amd.sparse_conv(X, W, bias, index, **kw)
    with pytest.raises(RuntimeError, match='activation'):
        amd.sparse_conv(X, W, bias, index, activation='gelu')
    with pytest.raises(TypeError):
        amd.sparse_conv(X, W, bias, index, None, scale)                   # keyword-only
    lib, out = _lib.load(), torch.zeros_like(residual)
    args = (X.data_ptr(), W.data_ptr(), None, None)
    tail = (index.nbr.data_ptr(), index.num.data_ptr(), len(X), len(X), 27, 4, 16)
    assert lib.gd3d_sparse_conv_forward_fused_cpu(*args, None, *tail, 0, out.data_ptr()) == 0
    assert torch.equal(out, amd.sparse_conv(X, W, None, index))           # nothing given: the plain convolution
    assert lib.gd3d_sparse_conv_forward_fused_cpu(*args, out.data_ptr(), *tail, 1, out.data_ptr()) == 10001        # the residual overlaps out
    assert lib.gd3d_sparse_conv_forward_fused_cpu(*args, out.data_ptr() + 4, *tail, 1, out.data_ptr()) == 10001
    assert lib.gd3d_sparse_conv_forward_fused_cpu(*args, None, *tail, -1, out.data_ptr()) == 10001
    assert lib.gd3d_sparse_conv_forward_fused_16_cpu(*args, None, *tail, 1, 3, out.data_ptr()) == 10001             # dtype
    assert lib.gd3d_sparse_conv_forward_fused_cpu(None, None, None, None, None, None, None, 4, 0, 27, 8, 8, 1, None) == 0       # R == 0
    assert lib.gd3d_sparse_conv_forward_fused_cpu(None, None, None, None, None, None, None, 4, 4, 27, 257, 8, 1, None) == 10002
    for n in ('fuse_sparse_conv_bn', 'FusedSparseConv', 'FusedSparseBasicBlock'):
        assert n in amd.__all__


# form -> (compute_dtype, an epilogue given, the features' dtype, the entries of one forward and one backward in call order,
#          the dtypes of out, grad_features).  Plain: the plain entry, never the fused one with null operands.  fp32 forms return the features'
#          dtype, 16-bit forms compute_dtype; grad_features comes back in the features' dtype, the parameter gradients in the parameters'.
CALL_FORMS = {
    'plain_fp32': (None, False, torch.float64, ('gd3d_sparse_conv_forward', 'gd3d_sparse_conv_backward_input', 'gd3d_sparse_conv_backward_weight'),
                   torch.float64, torch.float64),
    'plain_bf16': (torch.bfloat16, False, torch.float32,
                   ('gd3d_sparse_conv_forward_16', 'gd3d_sparse_conv_backward_input_16', 'gd3d_sparse_conv_backward_weight_16'),
                   torch.bfloat16, torch.float32),
    'fused_fp32': (None, True, torch.float64,
                   ('gd3d_sparse_conv_forward_fused', 'gd3d_sparse_conv_backward_input', 'gd3d_sparse_conv_backward_weight'),
                   torch.float64, torch.float64),
    'fused_bf16': (torch.bfloat16, True, torch.float32,
                   ('gd3d_sparse_conv_forward_fused_16', 'gd3d_sparse_conv_backward_input_16', 'gd3d_sparse_conv_backward_weight_16'),
                   torch.bfloat16, torch.float32),
}


@pytest.mark.parametrize('form', CALL_FORMS)
def test_every_call_form_makes_exactly_its_host_calls(form, monkeypatch):
    """one forward and one backward of `sparse_conv` per form: the entry points in order (one forward call, the input gradient, the weight
    gradient), the output's dtype and the gradients' dtypes"""
    from mmdet3d_gaussian_amd import _host
    compute_dtype, fused, x_dtype, entries, out_dtype, gx_dtype = CALL_FORMS[form]
    name = 'subm_9x12x10_c4_16'
    X, W, bias, scale, shift, residual = tensors_of(name, 'cpu', 'fp32')
    index = run_index(c16.case_of(name), 'cpu')                           # built before the calls are recorded
    seen, real = [], _host.call

    def recording(entry, dev, args, cpu_tail=()):
        seen.append(entry)
        return real(entry, dev, args, cpu_tail)
    monkeypatch.setattr(_host, 'call', recording)
    x, w, b = X.to(x_dtype).requires_grad_(True), W.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    res = residual.clone().requires_grad_(True) if fused else None
    kw = dict(scale=scale, shift=shift, residual=res, activation='relu') if fused else {}
    out = amd.sparse_conv(x, w, b, index, compute_dtype, **kw)
    assert tuple(seen) == entries[:1] and out.dtype == out_dtype
    grads = torch.autograd.grad(out, [x, w, b] + ([res] if fused else []), torch.ones_like(out))
    assert tuple(seen) == entries
    assert grads[0].dtype == gx_dtype and grads[1].dtype == w.dtype == torch.float32 and grads[2].dtype == b.dtype == torch.float32
    assert grads[1].shape == w.shape and (not fused or grads[3].dtype == res.dtype)
    assert all(g.abs().sum() > 0 for g in grads)


@pytest.mark.parametrize('kind', ['fp32', 'bf16'])
@pytest.mark.parametrize('block_type', ['conv_module', 'basicblock'])
def test_fused_encoder_follows_the_unfused_modules_layer_by_layer(block_type, kind, monkeypatch):
    check_fused_encoder('cpu', block_type, kind, monkeypatch)


def test_fuse_raises_on_a_training_batchnorm_and_leaves_a_pre_activation_module():
    seq = amd.make_sparse_convmodule(4, 16, 3, 'k')
    with pytest.raises(RuntimeError, match='training mode'):
        amd.fuse_sparse_conv_bn(seq)                                      # a fresh module is in training mode
    assert [type(m) for m in seq] == [amd.SubMConv3d, torch.nn.BatchNorm1d, torch.nn.ReLU]
    conv = seq[0]
    fused = amd.fuse_sparse_conv_bn(seq.eval())
    assert fused is seq and [type(m) for m in seq] == [amd.FusedSparseConv] and seq[0].conv is conv      # the conv's parameters are shared
    assert list(dict(seq.named_parameters())) == ['0.conv.weight'] and sorted(dict(seq.named_buffers())) == ['0.scale', '0.shift']
    pre = amd.make_sparse_convmodule(4, 16, 3, 'k', order=('norm', 'act', 'conv')).eval()
    assert amd.fuse_sparse_conv_bn(pre) is pre and [type(m) for m in pre] == [torch.nn.BatchNorm1d, torch.nn.ReLU, amd.SubMConv3d]
    with pytest.raises(RuntimeError, match='running statistics'):
        amd.fuse_sparse_conv_bn(amd.SparseSequential(amd.SubMConv3d(4, 8, 3), torch.nn.BatchNorm1d(8, track_running_stats=False)).eval())
    plain = amd.SparseSequential(amd.SubMConv3d(4, 8, 3), torch.nn.BatchNorm1d(8, affine=False), amd.SparseConv3d(8, 8, 3, max_out=9), torch.nn.ReLU()).eval()
    plain[1].running_var.fill_(4.0)
    plain[1].running_mean.fill_(1.0)
    amd.fuse_sparse_conv_bn(plain)
    assert [type(m) for m in plain] == [amd.FusedSparseConv] * 2 and plain[0].activation is None and plain[1].scale is None and plain[1].max_out == 9
    assert torch.allclose(plain[0].scale, torch.full((8,), 4.00001 ** -0.5)) and torch.allclose(plain[0].shift, torch.full((8,), -(4.00001 ** -0.5)))
    block = amd.SparseBasicBlock(8, 8).eval()
    assert isinstance(amd.fuse_sparse_conv_bn(block), amd.FusedSparseBasicBlock)
