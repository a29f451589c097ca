"""The sparse inverse convolution and SparseUNet on the `_cpu` twins: `sparse_inverse_conv` is `sparse_conv` over the
swapped tables of the forward layer's index, so it is held to `sparse_conv`'s own bounds against an oracle of its own — the fp64
`conv_transpose3d` of the densified features read at the forward layer's input sites (tests/sparse_decoder_ref.py).  fp32: |got - o64| <=
(L + 2) 2^-24 A; 16-bit outputs: E + u16 (|want| + E) with E = 2 (L + 2) 2^-24 A on the operands after rounding; fused: L + 4 and A'.
The check functions take the device: tests/test_gpu_sparse_decoder.py runs them on cuda:0."""
import copy
import functools

import numpy as np
import pytest
import torch

import mmdet3d_gaussian_amd as amd
import sparse_conv_16_cases as c16
import sparse_conv_ref as ref
import sparse_decoder_ref as dref
from mmdet3d_gaussian_amd.sparse_conv import SparseConvolution
from test_cpu_sparse_conv import count_calls
from test_cpu_sparse_conv_fused import randomise_batchnorms, within_fused_bound

B = 2
# name -> (shape, kernel, stride, padding)
GEOMS = {
    'k3s2p1_divides': ((7, 11, 9), (3, 3, 3), (2, 2, 2), (1, 1, 1)),             # (n + 2p - k) % s == 0 on every axis
    'k3s2p1_remainder': ((8, 10, 12), (3, 3, 3), (2, 2, 2), (1, 1, 1)),
    'k2s2p0_remainder': ((9, 11, 9), (2, 2, 2), (2, 2, 2), (0, 0, 0)),           # the last plane of every axis feeds no output: rows without a neighbour
    'k311s211': ((9, 11, 12), (3, 1, 1), (2, 1, 1), (0, 0, 0)),
    'k2s3': ((8, 10, 12), (2, 2, 2), (3, 3, 3), (0, 0, 0)),                      # stride above the kernel: every third plane is never read
}
PAIRS = ((16, 32), (5, 4), (64, 64))
KINDS = ('fp32', 'fp16', 'bf16')
N_ROWS = 300


@functools.lru_cache(maxsize=None)
def case_of(geom, max_out=None, inactive=False):
    """-> (coors (N, 4) int32, the restated index of the FORWARD layer); inactive: rows of -1 and out-of-range rows inside the tensor"""
    shape, kernel, stride, padding = GEOMS[geom]
    rng = np.random.default_rng(700 + sorted(GEOMS).index(geom))
    coors = ref.random_coors(rng, N_ROWS, shape, B)
    if inactive:
        coors = coors.copy()
        coors[rng.choice(N_ROWS, 40, replace=False)] = -1
        coors[5] = [B, 1, 1, 1]
    if isinstance(max_out, str):                                         # 'above' / 'below' the true count
        total = int(ref.index_ref(coors, shape, B, kernel, stride, padding, False)['num'][1])
        max_out = total + 9 if max_out == 'above' else total - 11
    return coors, ref.index_ref(coors, shape, B, kernel, stride, padding, False, max_out), max_out


@functools.lru_cache(maxsize=None)
def expected(geom, cin, cout, bias, kind, max_out=None, inactive=False):
    """-> (operands fp32, o64, A, L): computed once and shared, never modified.  X (R, Cin) lies on the forward layer's OUTPUT rows"""
    shape, kernel, stride, padding = GEOMS[geom]
    coors, idx, _ = case_of(geom, max_out, inactive)
    rng = np.random.default_rng(900 + cin + 3 * cout)
    K, R = idx['nbr'].shape[1], len(idx['nbr'])
    X = rng.standard_normal((R, cin)).astype(np.float32)
    W = (rng.standard_normal((K, cin, cout)) / np.sqrt(K * cin)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32) if bias else None
    gY = rng.standard_normal((len(coors), cout)).astype(np.float32)
    r = (lambda a: np.asarray(a, np.float64)) if kind == 'fp32' else (lambda a: dref.rounded(a, kind))
    run = lambda x, w, bb, g: dref.inverse_oracle(coors, shape, B, kernel, stride, padding, idx, x, w, bb, g)
    o64 = run(r(X), r(W), b, r(gY))
    A = run(np.abs(r(X)), np.abs(r(W)), None if b is None else np.abs(b), np.abs(r(gY)))
    L = ref.term_counts(dref.inverse_tables(idx), R, cin, cout, bias)
    return (X, W, b, gY), o64, A, L


def run_index(geom, dev, max_out=None, inactive=False):
    shape, kernel, stride, padding = GEOMS[geom]
    coors, _, mo = case_of(geom, max_out, inactive)
    return amd.sparse_conv_index(torch.from_numpy(coors).to(dev), shape, B, kernel, stride, padding, False, mo)


def run_inverse(dev, kind, index, X, W, b, gY, dead_fill=None):
    """`sparse_inverse_conv` and its gradients -> dict of fp32 / fp64-exact numpy arrays"""
    dtype = dref.DTYPES[kind]
    x = torch.from_numpy(X).to(dev).to(dtype)
    if dead_fill is not None:
        x[int(index.num[0]):] = dead_fill                                # the rows past the count: nothing may read them
    x.requires_grad_(True)
    w = torch.from_numpy(W).to(dev).requires_grad_(True)                 # fp32 master weights
    bias = None if b is None else torch.from_numpy(b).to(dev).requires_grad_(True)
    out = amd.sparse_inverse_conv(x, w, bias, index, None if kind == 'fp32' else dtype)
    assert out.dtype == dtype and out.shape == (index.in_coors.size(0), W.shape[2])
    grads = torch.autograd.grad(out, [x, w] + ([] if bias is None else [bias]), torch.from_numpy(gY).to(dev).to(dtype))
    f = lambda t: t.detach().float().cpu().numpy()
    return dict(out=f(out), gx=f(grads[0]), gw=f(grads[1]), gb=None if bias is None else f(grads[2]))


def assert_within(got, o64, A, L, kind, what):
    for key in ('out', 'gx', 'gw', 'gb'):
        if o64[key] is None:
            continue
        if kind == 'fp32' or key in ('gw', 'gb'):
            ok, ratio = ref.within_bound(got[key], o64[key], A[key], L[key])
        else:
            ok, ratio = c16.within_bound_16(got[key], o64[key], A[key], L[key], kind)
        print(f'{what} {kind} {key}: worst |ours - o64| / A = {ratio:.3e}')
        assert ok, f'{what} {kind}: {key} misses its bound, worst |ours - o64| / A = {ratio:.3e}'


def check_inverse(dev, kind, geom, cin, cout, bias=True, max_out=None, inactive=False):
    coors, idx, _ = case_of(geom, max_out, inactive)
    (X, W, b, gY), o64, A, L = expected(geom, cin, cout, bias, kind, max_out, inactive)
    index = run_index(geom, dev, max_out, inactive)
    assert np.array_equal(index.nbr_t.cpu().numpy(), idx['nbr_t']) and np.array_equal(index.nbr.cpu().numpy(), idx['nbr'])
    got = run_inverse(dev, kind, index, X, W, b, gY, dead_fill=float('nan') if max_out is not None else None)
    assert_within(got, o64, A, L, kind, f'inverse {geom} {cin}->{cout}')
    lone = ~(idx['nbr_t'] >= 0).any(1)
    assert not got['out'][lone].any(), 'a row without a valid neighbour is exactly zero, bias or not'
    assert np.isfinite(got['out']).all() and np.isfinite(got['gw']).all()
    dead = ~(idx['nbr'] >= 0).any(1)
    assert not got['gx'][dead].any()
    return got, lone


def check_static_against_exact(dev):
    """max_out above the count: the live rows carry the exact form's bits and the tail of the features is never read"""
    geom, cin, cout = 'k3s2p1_remainder', 16, 32
    (X, W, b, gY), _, _, _ = expected(geom, cin, cout, True, 'fp32', 'above')
    _, idx, _ = case_of(geom, 'above')
    kept = int(idx['num'][0])
    exact = run_inverse(dev, 'fp32', run_index(geom, dev), X[:kept], W, b, gY)
    static = run_inverse(dev, 'fp32', run_index(geom, dev, 'above'), X, W, b, gY, dead_fill=float('nan'))
    assert np.array_equal(exact['out'], static['out']) and np.array_equal(exact['gx'], static['gx'][:kept]) and not static['gx'][kept:].any()
    assert np.array_equal(exact['gw'], static['gw']) and np.array_equal(exact['gb'], static['gb'])


def check_modules(dev):
    shape, kernel, stride, padding = GEOMS['k3s2p1_remainder']
    coors, idx, _ = case_of('k3s2p1_remainder')
    torch.manual_seed(3)
    down = amd.SparseConv3d(4, 8, kernel, stride, padding, indice_key='a').to(dev)
    up = amd.SparseInverseConv3d(8, 6, kernel, 'a').to(dev)
    assert up.weight.shape == kernel + (8, 6) and up.bias.shape == (6,) and "indice_key='a'" in repr(up)
    x = amd.SparseConvTensor(torch.randn(len(coors), 4, device=dev), torch.from_numpy(coors).to(dev), shape, B)
    mid = down(x)
    stored = dict(mid.indice_dict)
    y = up(mid)
    assert torch.equal(y.indices, x.indices) and list(y.spatial_shape) == list(shape) and y.features.shape == (len(coors), 6)
    assert y.indice_dict is x.indice_dict and list(y.indice_dict) == ['a'] and all(y.indice_dict[k] is v for k, v in stored.items())
    want = amd.sparse_inverse_conv(mid.features, up.weight, up.bias, stored['a'])
    assert torch.equal(y.features, want)
    inv = amd.sparse_conv_index_inverse(stored['a'])
    assert inv.nbr is stored['a'].nbr_t and inv.nbr_t is stored['a'].nbr and inv.out_coors is stored['a'].in_coors and inv.num is None
    assert tuple(inv.out_shape) == tuple(shape) and inv.num_in == mid.features.size(0) and not inv.subm
    positional = amd.SparseConvIndex(*stored['a'][:6])                   # the record as it was built before the two fields existed
    assert positional.in_coors is None and positional.subm is False and positional.num_in == 0
    subm = amd.SubMConv3d(4, 8, 3, indice_key='s').to(dev)
    z = subm(x)
    bad = [lambda: amd.SparseInverseConv3d(8, 6, kernel, 'missing').to(dev)(mid),
           lambda: amd.SparseInverseConv3d(8, 6, 3, 's').to(dev)(z),                                  # a submanifold key
           lambda: amd.SparseInverseConv3d(8, 6, 2, 'a').to(dev)(mid),                                # wrong K
           lambda: up(x),                                                                             # x lies on the input rows, not the output rows
           lambda: amd.sparse_conv_index_inverse(z.indice_dict['s']), lambda: amd.sparse_conv_index_inverse(positional),
           lambda: amd.sparse_inverse_conv(mid.features[:-1], up.weight, None, stored['a'])]
    for i, call in enumerate(bad):
        with pytest.raises(RuntimeError):
            call()
            pytest.fail(f'call {i} did not raise')
    with pytest.raises(RuntimeError, match="'missing'"):
        amd.SparseInverseConv3d(8, 6, kernel, 'missing').to(dev)(mid)
    seq = amd.make_sparse_inverse_convmodule(8, 6, kernel, 'a')
    assert isinstance(seq[0], amd.SparseInverseConv3d) and seq[0].bias is None and isinstance(seq[1], torch.nn.BatchNorm1d) and isinstance(seq[2], torch.nn.ReLU)
    assert isinstance(amd.ToDense()(mid), torch.Tensor) and amd.ToDense()(mid).shape == (B, 8) + tuple(mid.spatial_shape)


def check_fused_module(dev, kind):
    """conv -> BatchNorm1d -> ReLU around an inverse conv: `fuse_sparse_conv_bn` gives ONE fused launch within the fused bound of the fp64 chain"""
    geom, cin, cout = 'k3s2p1_remainder', 16, 32
    shape, kernel, stride, padding = GEOMS[geom]
    coors, idx, _ = case_of(geom)
    (X, W, _, _), _, _, _ = expected(geom, cin, cout, False, kind)
    dtype = None if kind == 'fp32' else dref.DTYPES[kind]
    seq = amd.make_sparse_inverse_convmodule(cin, cout, kernel, 'a', compute_dtype=dtype)
    with torch.no_grad():
        seq[0].weight.copy_(torch.from_numpy(W).reshape(seq[0].weight.shape))
    seq = randomise_batchnorms(seq, 11).to(dev).eval()
    bn = seq[1]
    keys = list(seq.state_dict())
    converted = amd.convert_sparse_batchnorm(copy.deepcopy(seq))
    assert list(converted.state_dict()) == keys and isinstance(converted[1], amd.SparseBatchNorm1d) and len(converted) == 2
    fused = amd.fuse_sparse_conv_bn(copy.deepcopy(seq))
    assert len(fused) == 1 and isinstance(fused[0], amd.FusedSparseConv) and fused[0].activation == 'relu' and isinstance(fused[0].conv, amd.SparseInverseConv3d)
    x = amd.SparseConvTensor(torch.from_numpy(X).to(dev).to(dtype or torch.float32), torch.from_numpy(idx['out_coors']).to(dev), idx['out_shape'], B)
    x.indice_dict['a'] = run_index(geom, dev)
    with torch.no_grad():
        got, plain, live = fused(x), seq(x), converted(x)
    assert torch.equal(got.indices.cpu(), torch.from_numpy(coors)) and list(got.spatial_shape) == list(shape) and list(x.indice_dict) == ['a']
    r = (lambda a: np.asarray(a, np.float64)) if kind == 'fp32' else (lambda a: dref.rounded(a, kind))
    zeros = np.zeros((len(coors), cout))
    run = lambda xx, ww: dref.inverse_oracle(coors, shape, B, kernel, stride, padding, idx, xx, ww, None, zeros)['out']
    pre, A = run(r(X), r(W)), run(np.abs(r(X)), np.abs(r(W)))
    L = ref.term_counts(dref.inverse_tables(idx), len(X), cin, cout, False)['out']
    s = bn.weight.detach().double().cpu().numpy() / np.sqrt(bn.running_var.double().cpu().numpy() + bn.eps)
    sh = bn.bias.detach().double().cpu().numpy() - bn.running_mean.double().cpu().numpy() * s
    has = (idx['nbr_t'] >= 0).any(1)[:, None]
    want, scale = np.maximum(pre * s + sh, 0.0) * has, (A * np.abs(s) + np.abs(sh)) * has
    ok, ratio = within_fused_bound(got.features.float().cpu().numpy(), want, scale, L, kind)
    assert ok, f'fused inverse module {kind}: worst |ours - o64| / A\' = {ratio:.3e}'
    assert has.all() or not got.features[torch.from_numpy(~has[:, 0]).to(dev)].any()
    # the unfused eval chain is the same function up to its own rounding where every row has a neighbour; the converted norm keeps dead rows zero
    tol = 1e-5 if kind == 'fp32' else 4 * dref.U16[kind]
    rows = torch.from_numpy(has[:, 0]).to(dev)
    assert torch.allclose(got.features[rows].float(), plain.features[rows].float(), rtol=tol, atol=tol * float(np.abs(want).max()))
    assert torch.allclose(got.features.float(), live.features.float(), rtol=tol, atol=tol * float(np.abs(want).max()))


# ---- SparseUNet ------------------------------------------------------------------------------------------------------------------------

UNET_SHAPE, UNET_TALL, UNET_VOXELS = (9, 16, 16), (25, 16, 16), 300       # at D = 9 conv_out's (3, 1, 1) kernel has no output cell; at D = 25 it has
UNET_CFG = dict(base_channels=8, output_channels=16, encoder_channels=((8,), (16, 16, 16), (16, 16, 16), (16, 16, 16)),
                decoder_channels=((16, 16, 16), (16, 16, 16), (16, 16, 8), (8, 8, 8)))


def unet_inputs(shape):
    rng = np.random.default_rng(41)
    return ref.random_coors(rng, UNET_VOXELS, shape, B), rng.standard_normal((UNET_VOXELS, 4)).astype(np.float32)


def build_unet(dev, shape, kind='fp32'):
    torch.manual_seed(8)
    net = amd.SparseUNet(4, list(shape), compute_dtype=None if kind == 'fp32' else dref.DTYPES[kind], **UNET_CFG)
    return randomise_batchnorms(net, 9).to(dev)


def check_unet_shapes_and_index_calls(dev, monkeypatch):
    coors, feats = unet_inputs(UNET_SHAPE)
    net = build_unet(dev, UNET_SHAPE).eval()
    x, c = torch.from_numpy(feats).to(dev), torch.from_numpy(coors).to(dev)
    calls = count_calls(monkeypatch)
    with torch.no_grad():
        out = net(x, c, B)
        enc = amd.SparseEncoder.forward(net, x, c, B)
    keys = {m.indice_key for part in (net.conv_input, net.encoder_layers, net.conv_out) for m in part.modules() if isinstance(m, SparseConvolution)}
    assert keys == {'subm1', 'subm2', 'subm3', 'subm4', 'spconv2', 'spconv3', 'spconv4', 'spconv_down2'}
    assert calls['gd3d_sparse_conv_index'] == 2 * len(keys), calls        # two forwards; the decoder builds none
    assert out['seg_features'].shape == (UNET_VOXELS, UNET_CFG['decoder_channels'][-1][-1]) and torch.isfinite(out['seg_features']).all()
    assert out['spatial_features'].shape == enc.shape and torch.equal(out['spatial_features'], enc)
    # the input's row order: permuting the voxels permutes seg_features the same way (up to the order of the sums inside a layer)
    perm = torch.from_numpy(np.random.default_rng(5).permutation(UNET_VOXELS)).to(dev)
    with torch.no_grad():
        moved = net(x[perm], c[perm], B)['seg_features']
    assert torch.allclose(moved, out['seg_features'][perm], rtol=1e-4, atol=1e-5)
    inverse = [m for m in net.modules() if isinstance(m, amd.SparseInverseConv3d)]
    assert [m.indice_key for m in inverse] == ['spconv4', 'spconv3', 'spconv2']


def check_unet_gradients(dev, shape, skip=()):
    """every parameter receives a finite, non-zero gradient; `skip`: the modules without an output cell on this grid"""
    coors, feats = unet_inputs(shape)
    net = build_unet(dev, shape).train()
    out = net(torch.from_numpy(feats).to(dev), torch.from_numpy(coors).to(dev), B)
    (out['seg_features'].square().sum() + out['spatial_features'].square().sum()).backward()
    for name, p in net.named_parameters():
        if name.startswith(skip) and skip:
            assert p.grad is None or not p.grad.any(), name
        else:
            assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.any(), name


def check_unet_fused(dev, kind):
    """eval().fuse() against the unfused eval model, layer by layer: every fused layer's output on ITS input within the fused bound of the
    fp64 chain conv -> BatchNorm -> (+ identity) -> ReLU over the restated tables (the inverse layers over the swapped ones)"""
    coors, feats = unet_inputs(UNET_SHAPE)
    net = build_unet(dev, UNET_SHAPE, kind).eval()
    fused = copy.deepcopy(net)
    assert fused.fuse() is fused
    layers = [m for m in fused.modules() if isinstance(m, amd.FusedSparseConv)]
    norms = {id(m): None for m in layers}
    plain_convs = [m for m in net.modules() if isinstance(m, SparseConvolution)]
    plain_norms = [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm1d)]
    assert len(layers) == len(plain_convs) == len(plain_norms) == 28 and not any(isinstance(m, (torch.nn.BatchNorm1d, amd.SparseBasicBlock)) for m in fused.modules())
    by_weight = {}
    for conv, bn in zip(plain_convs, plain_norms):                       # modules() lists a conv and then its norm, in every container here
        by_weight[tuple(conv.weight.detach().flatten()[:4].tolist())] = bn
    seen = []
    hooks = [m.register_forward_hook(lambda mod, args, kwargs, out: seen.append((mod, args[0].features.detach(), args[0].indices, list(args[0].spatial_shape), args[0].indice_dict,
                                                                                 kwargs.get('residual'), out.features.detach())), with_kwargs=True)
             for m in layers]
    x, c = torch.from_numpy(feats).to(dev), torch.from_numpy(coors).to(dev)
    with torch.no_grad():
        got, want = fused(x, c, B), net(x, c, B)
    for h in hooks:
        h.remove()
    assert len(seen) == len(norms) and got['seg_features'].shape == want['seg_features'].shape and got['spatial_features'].shape == want['spatial_features'].shape
    cast = (lambda t: t.detach().double().cpu().numpy()) if kind == 'fp32' else (lambda t: t.detach().to(dref.DTYPES[kind]).double().cpu().numpy())
    worst = 0.0
    for layer, xf, xc, xshape, xdict, residual, y in seen:                # the input as it was when the layer ran: the decoder rewrites .features afterwards
        conv = layer.conv
        bn = by_weight[tuple(conv.weight.detach().flatten()[:4].tolist())]
        if isinstance(conv, amd.SparseInverseConv3d):
            stored = xdict[conv.indice_key]
            tables = dict(nbr=stored.nbr_t.cpu().numpy(), nbr_t=stored.nbr.cpu().numpy())
        else:
            tables = ref.index_ref(xc.cpu().numpy(), xshape, B, conv.kernel_size, conv.stride, conv.padding, conv.subm)
        if len(tables['nbr']) == 0:
            assert y.shape[0] == 0
            continue
        X, W = cast(xf), cast(conv.weight).reshape(-1, conv.in_channels, conv.out_channels)
        zeros = np.zeros((len(tables['nbr']), conv.out_channels))
        pre = ref.sparse_oracle(tables, X, W, None, zeros)['out']
        A = ref.sparse_oracle(tables, np.abs(X), np.abs(W), None, zeros)['out']
        L = ref.term_counts(tables, len(X), conv.in_channels, conv.out_channels, False)['out']
        s = bn.weight.detach().double().cpu().numpy() / np.sqrt(bn.running_var.double().cpu().numpy() + bn.eps)
        sh = bn.bias.detach().double().cpu().numpy() - bn.running_mean.double().cpu().numpy() * s
        t, a = pre * s + sh, A * np.abs(s) + np.abs(sh)
        if residual is not None:
            t, a = t + cast(residual), a + np.abs(cast(residual))
        has = (tables['nbr'] >= 0).any(1)[:, None]
        ok, ratio = within_fused_bound(y.float().cpu().numpy(), np.maximum(t, 0.0) * has, a * has, L, kind)
        worst = max(worst, ratio)
        assert ok, f'{layer}: the fused output misses its bound: worst |ours - o64| / A\' = {ratio:.3e}'
    print(f'fused SparseUNet ({kind}) on {dev}: worst |ours - o64| / A\' over {len(seen)} layers {worst:.3e}')


def check_unet_bf16_and_converted(dev):
    coors, feats = unet_inputs(UNET_TALL)                                # the live-row norm takes no empty grid: conv_out needs an output cell
    net = build_unet(dev, UNET_TALL, 'bf16').train()
    keys = list(net.state_dict())
    out = net(torch.from_numpy(feats).to(dev), torch.from_numpy(coors).to(dev), B)
    assert out['seg_features'].dtype == torch.bfloat16 and out['seg_features'].shape == (UNET_VOXELS, 8) and torch.isfinite(out['seg_features'].float()).all()
    out['seg_features'].float().square().sum().backward()
    assert all(p.grad is None or p.grad.dtype == torch.float32 for p in net.parameters())
    assert net.convert_norm() is net and list(net.state_dict()) == keys
    again = net(torch.from_numpy(feats).to(dev), torch.from_numpy(coors).to(dev), B)
    assert again['seg_features'].shape == (UNET_VOXELS, 8) and torch.isfinite(again['seg_features'].float()).all()


# ---- the tests -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('geom', sorted(GEOMS))
def test_every_geometry_against_the_transposed_dense_convolution(geom):
    got, lone = check_inverse('cpu', 'fp32', geom, 16, 32)
    if geom in ('k2s2p0_remainder', 'k2s3'):
        assert lone.sum() > 20, 'this geometry leaves active inputs without an output cell'


def test_the_cases_hold_what_they_claim():
    for geom, (shape, k, s, p) in GEOMS.items():
        rem = [(n + 2 * pa - ka) % sa for n, ka, sa, pa in zip(shape, k, s, p)]
        assert (max(rem) == 0) == (geom in ('k3s2p1_divides', 'k311s211')), (geom, rem)
    _, idx, mo = case_of('k3s2p1_remainder', 'below')
    assert idx['num'][0] == mo < idx['num'][1] and (~(idx['nbr_t'] >= 0).any(1)).any(), 'inputs whose outputs were all dropped'
    _, idx, mo = case_of('k3s2p1_remainder', 'above')
    assert idx['num'][0] == idx['num'][1] < mo


# every pair in every type, and 12 -> 20 (Cin % 8 != 0: the 16-bit kernels' element-wise gather) in the 16-bit types
PAIR_CASES = [(p, k) for k in KINDS for p in PAIRS] + [((12, 20), 'fp16'), ((12, 20), 'bf16')]


@pytest.mark.parametrize('pair,kind', PAIR_CASES, ids=lambda v: v if isinstance(v, str) else f'{v[0]}_{v[1]}')
def test_channel_pairs_in_every_type(pair, kind):
    check_inverse('cpu', kind, 'k3s2p1_remainder', *pair)


@pytest.mark.parametrize('kind', KINDS)
def test_without_bias_and_rows_without_a_neighbour_under_a_bias(kind):
    check_inverse('cpu', kind, 'k2s2p0_remainder', 16, 32, bias=False)
    got, lone = check_inverse('cpu', kind, 'k2s2p0_remainder', 5, 4, bias=True)
    assert lone.sum() > 20 and got['out'][~lone].all()


@pytest.mark.parametrize('max_out', ['above', 'below'])
@pytest.mark.parametrize('kind', ['fp32', 'bf16'])
def test_static_forward_index(kind, max_out):
    check_inverse('cpu', kind, 'k3s2p1_remainder', 16, 32, max_out=max_out)


def test_static_form_carries_the_exact_forms_bits():
    check_static_against_exact('cpu')


@pytest.mark.parametrize('kind', ['fp32', 'fp16'])
def test_inactive_input_rows_inside_the_tensor(kind):
    got, lone = check_inverse('cpu', kind, 'k3s2p1_divides', 16, 32, inactive=True)
    assert lone.sum() >= 41


def test_modules_and_bad_arguments():
    check_modules('cpu')


def test_make_sparse_convmodule_names_the_builder_of_the_inverse_module():
    with pytest.raises(RuntimeError, match='not built here'):
        amd.make_sparse_convmodule(4, 8, 3, 'k', conv_type='SparseConvTranspose3d')
    with pytest.raises(RuntimeError, match='order'):
        amd.make_sparse_inverse_convmodule(4, 8, 3, 'k', order=('conv', 'pool'))


@pytest.mark.parametrize('kind', KINDS)
def test_fused_inverse_module_within_the_fused_bound(kind):
    check_fused_module('cpu', kind)


def test_unet_shapes_row_order_and_index_builds(monkeypatch):
    check_unet_shapes_and_index_calls('cpu', monkeypatch)


def test_unet_every_parameter_gets_a_gradient():
    check_unet_gradients('cpu', UNET_SHAPE, skip=('conv_out',))
    check_unet_gradients('cpu', UNET_TALL)


@pytest.mark.parametrize('kind', ['fp32', 'bf16'])
def test_unet_fused_follows_the_unfused_model_layer_by_layer(kind):
    check_unet_fused('cpu', kind)


def test_unet_bf16_trains_and_converts():
    check_unet_bf16_and_converted('cpu')
