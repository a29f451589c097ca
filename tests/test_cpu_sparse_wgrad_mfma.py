"""The opt-in matrix-core weight gradient of the 16-bit sparse convolution, what holds without a device: the
`weight_grad` keyword on the two functions, the four layer classes, `FusedSparseConv` and the tree-walking `set_weight_grad`; that it is
inert on CPU tensors and in fp32 (the entries called and the gradients' bits are those of `None`); which entry a device tensor would take;
the exported symbol and its argument errors, code for code those of gd3d_sparse_conv_backward_weight_16.
tests/test_gpu_sparse_wgrad_mfma.py holds the values."""
import ctypes

import pytest
import torch

import mmdet3d_gaussian_amd as amd
import sparse_conv_16_cases as c16
import sparse_conv_ref as ref
from mmdet3d_gaussian_amd import _host, _lib, sparse_encoder
from mmdet3d_gaussian_amd.sparse_conv import SparseConvolution, _weight_entry
from test_cpu_sparse_conv import run_index
from test_cpu_sparse_conv_16 import convs_of

BASIC = dict(block_type='basicblock', encoder_channels=((16, 16, 32), (32, 32, 64), (64, 64, 128), (128, 128)),
             encoder_paddings=((0, 0, 1), (0, 0, 1), (0, 0, (0, 1, 1)), (0, 0)))
BAD_MODES = ('MFMA', 'fma', True, 1, torch.bfloat16, '')


def test_the_keyword_is_accepted_everywhere_and_a_bad_value_raises():
    case = ref.CASES['s2p1_9x12x10_c5_16']
    index = run_index(case, 'cpu')
    x, w = torch.randn(len(case['coors']), 5), torch.randn(27, 5, 16)
    for mode in (None, 'mfma'):
        y = amd.sparse_conv(x, w, None, index, weight_grad=mode)
        assert amd.sparse_inverse_conv(y, torch.randn(27, 16, 5), None, index, weight_grad=mode).shape == x.shape
        layers = (SparseConvolution(4, 8, 3, weight_grad=mode), amd.SubMConv3d(4, 8, 3, weight_grad=mode),
                  amd.SparseConv3d(4, 8, 3, 2, 1, weight_grad=mode), amd.SparseInverseConv3d(4, 8, 3, 'k', weight_grad=mode))
        for layer in layers:
            assert layer.weight_grad == mode and ('weight_grad' in layer.extra_repr()) == (mode is not None)
            assert (f"weight_grad={mode!r}" in repr(layer)) == (mode is not None)
            fused = amd.FusedSparseConv(layer, None, 'relu')
            assert fused.weight_grad == mode and ('weight_grad' in fused.extra_repr()) == (mode is not None)
    with pytest.raises(TypeError):
        amd.sparse_conv(x, w, None, index, None, None, None, None, None, 'mfma')          # keyword-only
    for bad in BAD_MODES:
        with pytest.raises(RuntimeError, match='weight_grad'):
            amd.sparse_conv(x, w, None, index, weight_grad=bad)
        with pytest.raises(RuntimeError, match='weight_grad'):
            amd.sparse_inverse_conv(torch.randn(index.nbr.size(0), 16), torch.randn(27, 16, 5), None, index, weight_grad=bad)
        for cls, args in ((amd.SubMConv3d, (4, 8, 3)), (amd.SparseConv3d, (4, 8, 3)), (amd.SparseInverseConv3d, (4, 8, 3, 'k')),
                          (SparseConvolution, (4, 8, 3))):
            with pytest.raises(RuntimeError, match='weight_grad'):
                cls(*args, weight_grad=bad)
        with pytest.raises(RuntimeError, match='weight_grad'):
            sparse_encoder.set_weight_grad(amd.SubMConv3d(4, 8, 3), bad)
        with pytest.raises(RuntimeError, match='weight_grad'):
            amd.SparseEncoder(4, [9, 48, 40]).set_weight_grad(bad)
    assert 'set_weight_grad' not in amd.__all__ and 'check_weight_grad' not in amd.__all__


def encoders():
    yield 'SparseEncoder conv_module', lambda: amd.SparseEncoder(4, [9, 48, 40])
    yield 'SparseEncoder basicblock', lambda: amd.SparseEncoder(4, [9, 48, 40], **BASIC)
    yield 'MlvlSparseEncoder', lambda: amd.MlvlSparseEncoder(4, [9, 48, 40])
    yield 'SparseUNet', lambda: amd.SparseUNet(4, [9, 48, 40])


@pytest.mark.parametrize('which', [n for n, _ in encoders()])
def test_the_setter_reaches_every_conv_before_and_after_convert_norm_and_fuse(which):
    make = dict(encoders())[which]
    plain = make()
    every_conv = lambda module: [m for m in module.modules() if isinstance(m, SparseConvolution)]     # the inverse layers of the U-Net included
    keys, n_convs = list(plain.state_dict()), len(every_conv(plain))
    assert n_convs >= len(convs_of(plain)) >= 12 and all(m.weight_grad is None for m in every_conv(plain))

    def check(enc, mode):
        convs = every_conv(enc)
        assert len(convs) == n_convs and all(m.weight_grad == mode for m in convs), which
        assert all(m.weight_grad == mode for m in enc.modules() if isinstance(m, amd.FusedSparseConv))

    enc = make()
    assert enc.set_weight_grad('mfma') is enc                     # before either rewrite
    check(enc, 'mfma')
    assert list(enc.state_dict()) == keys, 'the switch is an attribute, never a buffer or a parameter'
    assert enc.convert_norm() is enc
    check(enc, 'mfma')                                            # it survives convert_norm() ...
    enc.eval().fuse()
    check(enc, 'mfma')                                            # ... and eval().fuse()
    assert sum(isinstance(m, amd.FusedSparseConv) for m in enc.modules()) > 0
    fused_keys = list(enc.state_dict())
    enc.set_weight_grad(None)                                     # after both
    check(enc, None)
    enc.set_weight_grad('mfma')
    check(enc, 'mfma')
    assert list(enc.state_dict()) == fused_keys
    late = make().convert_norm()                                  # set after convert_norm() alone
    late.set_weight_grad('mfma')
    check(late, 'mfma')
    assert list(late.state_dict()) == keys
    seq = sparse_encoder.set_weight_grad(amd.make_sparse_convmodule(4, 16, 3, 'k'), 'mfma')   # the free function, on any module tree
    assert seq[0].weight_grad == 'mfma'


FORMS = {   # compute_dtype, the features' dtype -> the entries of one forward and one backward on CPU tensors
    'fp32': (None, torch.float32, ('gd3d_sparse_conv_forward', 'gd3d_sparse_conv_backward_input', 'gd3d_sparse_conv_backward_weight')),
    'fp16': (torch.float16, torch.float16, ('gd3d_sparse_conv_forward_16', 'gd3d_sparse_conv_backward_input_16', 'gd3d_sparse_conv_backward_weight_16')),
    'bf16': (torch.bfloat16, torch.bfloat16, ('gd3d_sparse_conv_forward_16', 'gd3d_sparse_conv_backward_input_16', 'gd3d_sparse_conv_backward_weight_16')),
    'auto': ('auto', torch.bfloat16, ('gd3d_sparse_conv_forward_16', 'gd3d_sparse_conv_backward_input_16', 'gd3d_sparse_conv_backward_weight_16')),
}


@pytest.mark.parametrize('form', list(FORMS))
def test_mfma_is_inert_on_cpu_tensors_and_in_fp32(form, monkeypatch):
    """recording `_host.call`: with 'mfma' the entries are exactly those of None, and every gradient is bit-equal"""
    compute_dtype, x_dtype, entries = FORMS[form]
    name = 'subm_9x12x10_c4_16'
    X, W, bias, gY = (torch.from_numpy(a) for a in c16.operands(name))
    index = run_index(c16.case_of(name), 'cpu')
    seen, real = [], _host.call

    def recording(entry, dev, args, cpu_tail=()):
        seen.append(entry)
        return real(entry, dev, args, cpu_tail)
    monkeypatch.setattr(_host, 'call', recording)
    results = {}
    for mode in (None, 'mfma'):
        del seen[:]
        x, w, b = X.to(x_dtype).requires_grad_(True), W.clone().requires_grad_(True), bias.clone().requires_grad_(True)
        out = amd.sparse_conv(x, w, b, index, compute_dtype, weight_grad=mode)
        grads = torch.autograd.grad(out, [x, w, b], gY.to(out.dtype))
        assert tuple(seen) == entries, (form, mode, seen)
        results[mode] = [out.detach()] + list(grads)
    for a, b in zip(results[None], results['mfma']):
        assert a.dtype == b.dtype and torch.equal(a, b)
    assert all(g.abs().sum() > 0 for g in results['mfma'])


def test_the_entry_a_device_tensor_takes():
    """`_weight_entry` is what `_backward_entries` hands to `_host.call`: the device type alone is read, so no device is needed"""
    cuda, cpu = torch.device('cuda:0'), torch.device('cpu')
    for dtype in (torch.float16, torch.bfloat16):
        assert _weight_entry(dtype, cuda, None) == 'gd3d_sparse_conv_backward_weight_16'
        assert _weight_entry(dtype, cuda, 'mfma') == 'gd3d_sparse_conv_backward_weight_16_mfma'
        assert _weight_entry(dtype, cpu, 'mfma') == 'gd3d_sparse_conv_backward_weight_16'
    for mode in (None, 'mfma'):
        assert _weight_entry(None, cuda, mode) == 'gd3d_sparse_conv_backward_weight'
        assert _weight_entry(None, cpu, mode) == 'gd3d_sparse_conv_backward_weight'
    assert _lib.SYMBOLS['gd3d_sparse_conv_backward_weight_16_mfma'] == _lib.SYMBOLS['gd3d_sparse_conv_backward_weight_16']
    assert hasattr(_lib.load(), 'gd3d_sparse_conv_backward_weight_16_mfma')


def test_the_new_entry_returns_the_old_entrys_codes_before_any_launch():
    """argument errors that return before a launch, so no device is touched: null pointers, K = 0, 257 channels, a bad dtype, a misaligned
    workspace, an odd 16-bit pointer — the same code from both entries for the same arguments"""
    lib = _lib.load()
    new, old = lib.gd3d_sparse_conv_backward_weight_16_mfma, lib.gd3d_sparse_conv_backward_weight_16
    buf = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(buf) + 255) & ~255                   # host memory: only its ADDRESS is checked, nothing is read or written
    x, g, nbr, num, work, gw, gb = base, base + 512, base + 1024, base + 1536, base + 2048, base + 2560, base + 3072
    calls = {                                                     # features, grad_out, nbr, num, N, R, K, Cin, Cout, dtype, workspace, gw, gb
        'K = 0': ((x, g, nbr, num, 4, 4, 0, 8, 8, 1, work, gw, gb), 10001),
        'Cin = 0': ((x, g, nbr, num, 4, 4, 27, 0, 8, 1, work, gw, gb), 10001),
        'K = 28': ((x, g, nbr, num, 4, 4, 28, 8, 8, 1, work, gw, gb), 10002),
        'Cin = 257': ((x, g, nbr, num, 4, 4, 27, 257, 8, 1, work, gw, gb), 10002),
        'Cout = 257': ((x, g, nbr, num, 4, 4, 27, 8, 257, 2, work, gw, gb), 10002),
        'dtype 0': ((x, g, nbr, num, 4, 4, 27, 8, 8, 0, work, gw, gb), 10001),
        'dtype 3': ((x, g, nbr, num, 4, 4, 27, 8, 8, 3, work, gw, gb), 10001),
        'dtype -1': ((x, g, nbr, num, 4, 4, 27, 8, 8, -1, work, gw, gb), 10001),
        'N < 0': ((x, g, nbr, num, -1, 4, 27, 8, 8, 1, work, gw, gb), 10001),
        'R < 0': ((x, g, nbr, num, 4, -1, 27, 8, 8, 1, work, gw, gb), 10001),
        'no grad_weight': ((x, g, nbr, num, 4, 4, 27, 8, 8, 2, work, None, gb), 10001),
        'no grad_weight, R = 0': ((x, g, nbr, num, 4, 0, 27, 8, 8, 2, work, None, gb), 10001),
        'R beyond int32': ((x, g, nbr, num, 4, 1 << 31, 27, 8, 8, 1, work, gw, gb), 10002),
        'R K beyond int32': ((x, g, nbr, num, 4, 1 << 27, 27, 8, 8, 1, work, gw, gb), 10002),
        'no features': ((None, g, nbr, num, 4, 4, 27, 8, 8, 1, work, gw, gb), 10001),
        'no grad_out': ((x, None, nbr, num, 4, 4, 27, 8, 8, 1, work, gw, gb), 10001),
        'no nbr': ((x, g, None, num, 4, 4, 27, 8, 8, 2, work, gw, gb), 10001),
        'no workspace': ((x, g, nbr, num, 4, 4, 27, 8, 8, 2, None, gw, gb), 10001),
        'workspace off 256': ((x, g, nbr, num, 4, 4, 27, 8, 8, 2, work + 128, gw, gb), 10001),
        'odd features': ((x + 1, g, nbr, num, 4, 4, 27, 8, 8, 1, work, gw, gb), 10001),
        'odd grad_out': ((x, g + 1, nbr, num, 4, 4, 27, 8, 8, 2, work, gw, None), 10001),
    }
    for what, (args, code) in calls.items():
        assert new(*args, None) == old(*args, None) == code, what
    assert bytes(buf) == bytes(4096), 'nothing is touched'
