"""fp16 / bf16 sparse 3D convolution on the CPU (csrc/sparse_conv_16_cpu.cpp, the `_cpu` twins of csrc/sparse_conv_16.hip): every value
case of tests/sparse_conv_ref.py and the row cases of tests/sparse_conv_16_cases.py in both 16-bit types against the fp64 dense-conv3d
oracle on the rounded operands — the 16-bit outputs within E + u16 (|want| + E) + s, E = 2 (L + 2) 2^-24 A, the fp32 weight and bias
gradients within (L + 2) 2^-24 A (sparse_conv_16_cases.py); `compute_dtype=None` is the call without the keyword, bit for bit; what
'auto' picks; fp32 master weights get fp32 gradients without a 16-bit rounding; dense() of 16-bit features; the keyword reaches every
conv of the encoders; non-finite inputs and sums beyond the type's range; bad arguments.  tests/test_gpu_sparse_conv_16.py runs the same helpers on the device."""
import numpy as np
import pytest
import torch

import mmdet3d_gaussian_amd as amd
import sparse_conv_16_cases as c16
import sparse_conv_ref as ref
from mmdet3d_gaussian_amd import _host, _lib
from test_cpu_sparse_conv import check_nonfinite_containment, run_index

KINDS = ('fp16', 'bf16')


def run_values_16(name, dev, kind, index=None):
    """forward and the three gradients through the autograd function, 16-bit features and grad_out, fp32 parameters (master weights)
    -> dict of numpy arrays: out and gx fp32 views of the 16-bit results (exact), gw and gb as the kernels wrote them"""
    dtype = c16.DTYPES[kind]
    X, W, bias, gY = (None if a is None else torch.from_numpy(a).to(dev) for a in c16.operands(name))
    index = run_index(c16.case_of(name), dev) if index is None else index
    x, w = X.to(dtype).requires_grad_(True), W.clone().requires_grad_(True)
    b = None if bias is None else bias.clone().requires_grad_(True)
    out = amd.sparse_conv(x, w, b, index, compute_dtype=dtype)
    grads = torch.autograd.grad(out, [x, w] + ([] if b is None else [b]), gY.to(dtype))
    assert out.dtype == dtype and grads[0].dtype == dtype and grads[1].dtype == torch.float32 and (b is None or grads[2].dtype == torch.float32)
    return dict(out=out.detach().float().cpu().numpy(), gx=grads[0].float().cpu().numpy(), gw=grads[1].cpu().numpy(),
                gb=None if b is None else grads[2].cpu().numpy())


def check_values_16(name, dev, kind, got=None):
    """the four quantities within their bounds of the fp64 oracle on the rounded operands; returns the worst |ours - o64| / A per quantity"""
    o64, A, L = c16.expected_values(name, kind)
    got = run_values_16(name, dev, kind) if got is None else got
    worst = {}
    for k in ('out', 'gx', 'gw', 'gb'):
        if o64[k] is None:
            assert got[k] is None
            continue
        assert got[k].shape == o64[k].shape, (name, k)
        if k in ('out', 'gx'):
            ok, worst[k] = c16.within_bound_16(got[k], o64[k], A[k], L[k], kind)
        else:
            ok, worst[k] = ref.within_bound(got[k], o64[k], A[k], L[k])
        print(f'{name} {kind} on {dev}: {k}: worst |ours - o64| / A = {worst[k]:.3e} (L up to {int(np.max(L[k], initial=0))})')
        assert ok, f'{name} {kind}: {k} misses its bound on {dev}: worst ratio {worst[k]:.3e}'
    live = (c16.expected_index(name)['nbr'] >= 0).any(1)
    assert not got['out'][~live].any(), f'{name}: a row without neighbours is not zero'
    case = c16.case_of(name)
    dead = ~ref.active_rows(case['coors'], case['shape'], case['B'])
    assert not got['gx'][dead].any(), f'{name}: the input gradient of an inactive row is not zero'
    return worst


def check_range_16(dev, kind):
    """a sum beyond the type's range is inf, never the largest finite value: every feature 60000 (fp16) or 3e38 (bf16), every weight +1,
    then -1, on the 4 x 4 x 4 block (8 .. 27 neighbours of 4 channels a row)"""
    name, dtype = 'subm_dense_block_4x4x4', c16.DTYPES[kind]
    case = ref.CASES[name]
    index = run_index(case, dev)
    assert (ref.expected_index(name)['nbr'] >= 0).any(1).all()
    x = torch.full((len(case['coors']), case['cin']), dict(fp16=60000.0, bf16=3e38)[kind], device=dev).to(dtype)
    assert torch.isfinite(x).all()
    for sign in (1.0, -1.0):
        w = torch.full((27, case['cin'], case['cout']), sign, device=dev)
        out = amd.sparse_conv(x, w, None, index, compute_dtype=dtype)
        assert out.dtype == dtype and torch.equal(out.float(), torch.full_like(out, sign * float('inf'), dtype=torch.float32)), (kind, sign)


def check_dense_16(dev):
    """dense() of fp16 / bf16 features and its gradient equal the upcast - copy - downcast route bit for bit"""
    case = ref.CASES['subm_inactive_rows_scattered_and_tail']
    coors = torch.from_numpy(case['coors']).to(dev)
    torch.manual_seed(15)
    for dtype in c16.DTYPES.values():
        for C in (1, 5, 64):
            feats = torch.randn(len(coors), C, device=dev).to(dtype).requires_grad_(True)
            dense = amd.SparseConvTensor(feats, coors, case['shape'], case['B']).dense()
            up = feats.detach().float().requires_grad_(True)
            want = amd.sparse_to_dense(up, coors, case['shape'], case['B'])
            assert dense.dtype == dtype and dense.shape == want.shape and torch.equal(dense, want.to(dtype))
            g = torch.randn_like(dense)
            (gx,) = torch.autograd.grad(dense, feats, g)
            (wx,) = torch.autograd.grad(want, up, g.float())
            assert gx.dtype == dtype and torch.equal(gx, wx.to(dtype))
    odd = amd.sparse_to_dense(torch.ones(1, 1, device=dev, dtype=torch.bfloat16), torch.zeros(1, 4, dtype=torch.int32, device=dev), (1, 1, 3), 1)
    assert odd.flatten().tolist() == [1.0, 0.0, 0.0]                    # an odd number of 2-byte elements: the last one is cleared too


def check_modules_16(dev):
    """the module form with compute_dtype equals the functional form, bit for bit, forward and gradients"""
    torch.manual_seed(16)
    case = ref.CASES['s2p1_9x12x10_c5_16']
    coors = torch.from_numpy(case['coors']).to(dev)
    feats = torch.randn(len(coors), 5, device=dev)
    for cls, geom, dtype in ((amd.SubMConv3d, 'subm', torch.bfloat16), (amd.SparseConv3d, 's2p1', torch.float16), (amd.SparseConv3d, 'down', 'auto')):
        k, s, p, subm = ref.GEOMS[geom]
        layer = cls(5, 16, k, s, p, bias=True, compute_dtype=dtype).to(dev)
        assert layer.compute_dtype == dtype and 'compute_dtype' in layer.extra_repr() and 'compute_dtype' not in cls(5, 16, k, s, p).extra_repr()
        fin = feats.half() if dtype == 'auto' else feats
        x = amd.SparseConvTensor(fin.clone().requires_grad_(True), coors, case['shape'], case['B'])
        y = layer(x)
        index = amd.sparse_conv_index(coors, case['shape'], case['B'], k, s, p, subm)
        f = fin.clone().requires_grad_(True)
        want = amd.sparse_conv(f, layer.weight, layer.bias, index, compute_dtype=dtype)
        assert y.features.dtype == (torch.float16 if dtype == 'auto' else dtype) and torch.equal(y.features, want)
        g = torch.randn_like(want)
        got = torch.autograd.grad(y.features, [x.features, layer.weight, layer.bias], g)
        exp = torch.autograd.grad(want, [f, layer.weight, layer.bias], g)
        for a, b in zip(got, exp):
            assert a.dtype == b.dtype and torch.equal(a, b)
        assert got[0].dtype == fin.dtype and got[1].dtype == torch.float32 and got[1].shape == layer.weight.shape


def convs_of(module):
    return [m for m in module.modules() if isinstance(m, (amd.SubMConv3d, amd.SparseConv3d))]


# ---- the tests -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', c16.VALUE_CASES)
def test_values_twin_within_the_bounds_of_the_fp64_oracle(name, kind):
    check_values_16(name, 'cpu', kind)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', ['subm_9x12x10_c4_16', 's2p1_9x12x10_c5_16'])
def test_a_non_finite_value_reaches_only_what_reads_it(name, kind):
    check_nonfinite_containment(name, 'cpu', c16.DTYPES[kind])


@pytest.mark.parametrize('kind', KINDS)
def test_a_sum_beyond_the_range_is_inf_not_the_largest_finite_value(kind):
    check_range_16('cpu', kind)


def test_the_row_cases_hold_what_they_claim():
    for n in (0, 1, 15, 16, 17, 127, 128, 129, 257):
        assert sum(len(c['coors']) == n for c in c16.ROW_CASES.values()) == 2, n
    assert all(c['cin'] == 16 and c['cout'] == 16 for c in c16.ROW_CASES.values())
    assert set(c16.GUARD_CASES) <= set(ref.CASES) and len(set(c16.GUARD_CASES)) == 14 and set(c16.DEAD_TILE_CASES) <= set(c16.GUARD_CASES)
    assert ref.CASES['subm_9x12x10_c4_16']['cin'] == 4 and ref.CASES['s2p011_7x11x13_c3_7']['cout'] == 7


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16, torch.float32])
def test_compute_dtype_none_is_the_call_without_the_keyword(dtype):
    name = 'subm_rows_tile_plus_1'
    X, W, bias, gY = (torch.from_numpy(a).to(dtype) for a in ref.operands(name))
    index = run_index(ref.CASES[name], 'cpu')
    res = []
    for kw in (dict(), dict(compute_dtype=None)):
        x, w, b = X.clone().requires_grad_(True), W.clone().requires_grad_(True), bias.clone().requires_grad_(True)
        out = amd.sparse_conv(x, w, b, index, **kw)
        res.append((out,) + torch.autograd.grad(out, [x, w, b], gY))
    for a, b in zip(*res):
        assert a.dtype == dtype and torch.equal(a, b)
    if dtype != torch.float32:                                           # and that call is the fp32 evaluation cast back, not the 16-bit path
        assert torch.equal(res[0][0], amd.sparse_conv(X.float(), W.float(), bias.float(), index).to(dtype))


def test_auto_picks_the_features_dtype_then_the_autocast_dtype_then_fp32(monkeypatch):
    name = 'subm_rows_tile_plus_1'
    X, W, bias, _ = (torch.from_numpy(a) for a in ref.operands(name))
    index = run_index(ref.CASES[name], 'cpu')
    seen = []
    real = _host.call
    monkeypatch.setattr(_host, 'call', lambda n, dev, args, cpu_tail=(): (seen.append((n, args)), real(n, dev, args, cpu_tail))[1])
    for dtype, code in ((torch.float16, 1), (torch.bfloat16, 2)):
        out = amd.sparse_conv(X.to(dtype), W, bias, index, compute_dtype='auto')
        assert out.dtype == dtype and seen[-1][0] == 'gd3d_sparse_conv_forward_16' and seen[-1][1][10] == code
        assert torch.equal(out, amd.sparse_conv(X.to(dtype), W, bias, index, compute_dtype=dtype))
    with torch.autocast('cpu', dtype=torch.bfloat16):
        out = amd.sparse_conv(X, W, bias, index, compute_dtype='auto')
    assert out.dtype == torch.bfloat16 and seen[-1][0] == 'gd3d_sparse_conv_forward_16' and seen[-1][1][10] == 2
    out = amd.sparse_conv(X, W, bias, index, compute_dtype='auto')       # fp32 features, no autocast: the fp32 path
    assert out.dtype == torch.float32 and seen[-1][0] == 'gd3d_sparse_conv_forward' and torch.equal(out, amd.sparse_conv(X, W, bias, index))
    out = amd.sparse_conv(X.double(), W.double(), bias.double(), index, compute_dtype='auto')
    assert out.dtype == torch.float64 and seen[-1][0] == 'gd3d_sparse_conv_forward'


def test_fp32_master_weights_get_fp32_gradients_without_a_16_bit_rounding():
    name = 's2p1_9x12x10_c5_16'
    X, W, bias, gY = (torch.from_numpy(a) for a in ref.operands(name))
    index = run_index(ref.CASES[name], 'cpu')
    x, w, b = X.clone().requires_grad_(True), W.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    out = amd.sparse_conv(x, w, b, index, compute_dtype=torch.bfloat16)
    gx, gw, gb = torch.autograd.grad(out, [x, w, b], gY)
    assert out.dtype == torch.bfloat16 and gx.dtype == torch.float32 and gw.dtype == torch.float32 and gb.dtype == torch.float32
    # the fp32 twin on the rounded operands: the same loops on the same (exactly representable) values
    x16, g16 = X.bfloat16().float().requires_grad_(True), gY.bfloat16().float()
    w32, b32 = W.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    _, want_w, want_b = torch.autograd.grad(amd.sparse_conv(x16, w32, b32, index), [x16, w32, b32], g16)
    assert torch.equal(gw, want_w) and torch.equal(gb, want_b)
    assert not torch.equal(gw, gw.bfloat16().float()), 'the weight gradient carries more than 8 bits'
    assert torch.equal(gx, gx.bfloat16().float()), 'grad_features is the 16-bit result, returned in the features dtype'


def test_dense_of_16_bit_features_equals_the_upcast_route():
    check_dense_16('cpu')


def test_modules_equal_the_functional_form():
    check_modules_16('cpu')


@pytest.mark.parametrize('block_type', ['conv_module', 'basicblock'])
def test_the_keyword_reaches_every_conv_of_the_encoders(block_type):
    kw = dict(block_type=block_type)
    if block_type == 'basicblock':
        kw.update(encoder_channels=((16, 16, 32), (32, 32, 64), (64, 64, 128), (128, 128)), encoder_paddings=((0, 0, 1), (0, 0, 1), (0, 0, (0, 1, 1)), (0, 0)))
    for cls in (amd.SparseEncoder, amd.MlvlSparseEncoder):
        enc = cls(4, [9, 48, 40], compute_dtype=torch.bfloat16, **kw)
        convs = convs_of(enc)
        assert len(convs) == dict(conv_module=12, basicblock=21)[block_type] and all(m.compute_dtype == torch.bfloat16 for m in convs) and enc.compute_dtype == torch.bfloat16
        assert enc.fp16_enabled is False
        plain = cls(4, [9, 48, 40], **kw)
        assert len(convs_of(plain)) == len(convs) and all(m.compute_dtype is None for m in convs_of(plain)) and plain.compute_dtype is None
    block = amd.SparseBasicBlock(16, 16, compute_dtype='auto')
    assert block.conv1.compute_dtype == 'auto' and block.conv2.compute_dtype == 'auto'
    seq = amd.make_sparse_convmodule(4, 16, 3, 'k', conv_type='SparseConv3d', compute_dtype=torch.float16)
    assert seq[0].compute_dtype == torch.float16


def test_bad_arguments_raise():
    name = 'subm_rows_tile'
    case = ref.CASES[name]
    index = run_index(case, 'cpu')
    x, w = torch.zeros(len(case['coors']), 16), torch.zeros(27, 16, 16)
    for bad in (torch.float64, torch.float32, torch.int32, 'fp16', 'AUTO', 1):
        with pytest.raises(RuntimeError, match='compute_dtype'):
            amd.sparse_conv(x, w, None, index, compute_dtype=bad)
        with pytest.raises(RuntimeError, match='compute_dtype'):
            amd.SubMConv3d(4, 8, 3, compute_dtype=bad)
        with pytest.raises(RuntimeError, match='compute_dtype'):
            amd.SparseEncoder(4, [9, 48, 40], compute_dtype=bad)
    with pytest.raises(TypeError):
        amd.SubMConv3d(4, 8, 3, 1, 0, 1, True, None, torch.float16)        # keyword-only
    lib = _lib.load()                                                      # the C entry points' own codes: nothing is touched
    n = len(x)
    x16, w16, o16 = x.half(), w.half(), torch.zeros(n, 16, dtype=torch.float16)
    num = index.num
    for code in (0, 3, -1):
        assert lib.gd3d_sparse_conv_forward_16_cpu(x16.data_ptr(), w16.data_ptr(), None, index.nbr.data_ptr(), num.data_ptr(), n, n, 27, 16, 16, code,
                                                   o16.data_ptr()) == 10001
        assert lib.gd3d_sparse_conv_backward_input_16_cpu(o16.data_ptr(), w16.data_ptr(), index.nbr.data_ptr(), 1, n, n, 27, 16, 16, code, x16.data_ptr()) == 10001
        assert lib.gd3d_sparse_conv_backward_weight_16_cpu(x16.data_ptr(), o16.data_ptr(), index.nbr.data_ptr(), num.data_ptr(), n, n, 27, 16, 16, code, None,
                                                           torch.zeros(27, 16, 16).data_ptr(), None) == 10001
    assert lib.gd3d_sparse_conv_forward_16_cpu(x16.data_ptr(), w16.data_ptr(), None, index.nbr.data_ptr(), num.data_ptr(), n, n, 27, 16, 16, 1, o16.data_ptr()) == 0
    assert lib.gd3d_sparse_conv_forward_16_cpu(None, None, None, None, None, 4, 4, 27, 0, 8, 1, None) == 10001
    assert lib.gd3d_sparse_conv_forward_16_cpu(None, None, None, None, None, 4, 4, 27, 257, 8, 1, None) == 10002
    assert lib.gd3d_sparse_conv_forward_16_cpu(None, None, None, None, None, 4, 0, 27, 8, 8, 2, None) == 0        # R == 0: nothing to do
    assert lib.gd3d_sparse_conv_forward_16_cpu(x16.data_ptr() + 1, w16.data_ptr(), None, index.nbr.data_ptr(), None, n, n, 27, 16, 16, 1, o16.data_ptr()) == 10001
    assert lib.gd3d_sparse_conv_backward_input_16_cpu(None, None, None, 1, 4, 5, 27, 8, 8, 1, None) == 10001         # flip needs N == R
    assert lib.gd3d_sparse_conv_backward_weight_16_cpu(None, None, None, None, 4, 4, 27, 8, 8, 2, None, None, None) == 10001   # no grad_weight
    assert lib.gd3d_sparse_to_dense_16_cpu(None, None, 4, 0, 2, 3, 3, 3, None) == 10001
    assert lib.gd3d_sparse_to_dense_backward_16_cpu(None, None, 4, 300, 2, 3, 3, 3, None) == 10002
