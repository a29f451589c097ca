"""Sparse 3D convolution on the CPU (csrc/sparse_conv_cpu.cpp, the `_cpu` twins): every named case of tests/sparse_conv_ref.py.  The
integer outputs — out_coors, out_shape, nbr, nbr_t, num, out_batch_cnt — EXACTLY equal the numpy restatement; the values — forward, input
gradient, weight gradient, bias gradient — lie within (L + 2) 2^-24 A of the fp64 dense-conv3d oracle, L counted from the restated tables
and A the same convolution of absolute values (a derived bound, sparse_conv_ref.py); the modules equal the functional form, share an
index per `indice_key`, and `MlvlSparseEncoder` at PV-RCNN's constructor values follows a per-layer fp64 oracle.  The index build over
300 samples, at max_out 0 and 1 and at batch size 0; a non-finite input reaches only the outputs that read it.
tests/test_gpu_sparse_conv.py runs the same helpers on the device."""
import ctypes

import numpy as np
import pytest
import torch

import mmdet3d_gaussian_amd as amd
import sparse_conv_ref as ref
from mmdet3d_gaussian_amd import _host, _lib

INT_OUTPUTS = ('out_coors', 'nbr', 'nbr_t', 'num', 'out_batch_cnt')
VALUE_CASES = sorted(n for n, c in ref.CASES.items() if c['values'])
SWEEPS = ('sweep_subm', 'sweep_s2p1')


def run_index(case, dev, max_out='case'):
    """the static call (the dynamic one where the case fixes no max_out) -> the record"""
    coors = torch.from_numpy(case['coors']).to(dev)
    return amd.sparse_conv_index(coors, case['shape'], case['B'], case['kernel'], case['stride'], case['padding'], case['subm'],
                                 case['max_out'] if max_out == 'case' else max_out)


def check_index(name, dev):
    """every integer output equals the restatement exactly; returns the record"""
    case, want = ref.case_of(name), ref.expected_index(name)
    got = run_index(case, dev)
    assert tuple(got.out_shape) == tuple(want['out_shape']), name
    for k in INT_OUTPUTS:
        g, w = getattr(got, k), want[k]
        assert (g is None) == (w is None), (name, k)
        if g is not None:
            assert g.dtype == (torch.int64 if k == 'num' else torch.int32) and np.array_equal(g.cpu().numpy(), w), f'{name}: {k} differs from the restatement on {dev}'
    kept = int(want['num'][0])
    assert (want['out_coors'][kept:] == -1).all() and (want['nbr'][kept:] == -1).all()
    return got


def run_values(name, dev, index=None):
    """forward and the three gradients through the autograd function -> dict of numpy arrays"""
    case = ref.case_of(name)
    X, W, bias, gY = (None if a is None else torch.from_numpy(a).to(dev) for a in ref.operands(name))
    index = run_index(case, dev) if index is None else index
    x, w = X.clone().requires_grad_(True), W.clone().requires_grad_(True)
    b = None if bias is None else bias.clone().requires_grad_(True)
    out = amd.sparse_conv(x, w, b, index)
    grads = torch.autograd.grad(out, [x, w] + ([] if b is None else [b]), gY)
    return dict(out=out.detach().cpu().numpy(), gx=grads[0].cpu().numpy(), gw=grads[1].cpu().numpy(), gb=None if b is None else grads[2].cpu().numpy())


def check_values(name, dev, got=None):
    """the four quantities within the derived bound of the fp64 oracle; returns the worst |ours - o64| / A per quantity"""
    o64, A, L = ref.expected_values(name)
    got = run_values(name, dev) if got is None else got
    worst = {}
    for k in ('out', 'gx', 'gw', 'gb'):
        if o64[k] is None:
            assert got[k] is None
            continue
        assert got[k].shape == o64[k].shape and got[k].dtype == np.float32, (name, k)
        ok, worst[k] = ref.within_bound(got[k], o64[k], A[k], L[k])
        print(f'{name} on {dev}: {k}: worst |ours - o64| / A = {worst[k]:.3e} (L up to {int(np.max(L[k], initial=0))})')
        assert ok, f'{name}: {k} misses (L + 2) 2^-24 A on {dev}: worst ratio {worst[k]:.3e}'
    live = (ref.expected_index(name)['nbr'] >= 0).any(1)
    assert not got['out'][~live].any(), f'{name}: a row without neighbours is not zero'
    case = ref.case_of(name)
    dead = ~ref.active_rows(case['coors'], case['shape'], case['B'])
    assert not got['gx'][dead].any(), f'{name}: the input gradient of an inactive row is not zero'
    return worst


def check_many_samples(geom, dev):
    """B = 300: the counting kernel's loop over the samples takes a second trip; every integer output equals the restatement"""
    case = ref.many_samples_case(geom)
    want = ref.index_ref(case['coors'], case['shape'], case['B'], case['kernel'], case['stride'], case['padding'], case['subm'])
    got = run_index(case, dev)
    assert tuple(got.out_shape) == tuple(want['out_shape'])
    for k in INT_OUTPUTS:
        if want[k] is not None:
            assert np.array_equal(getattr(got, k).cpu().numpy(), want[k]), f'{geom}: {k} differs from the restatement on {dev}'
    cnt = got.out_batch_cnt.cpu().numpy()
    assert cnt.shape == (ref.MANY_B,) and cnt.sum() == int(got.num[0]) > 0 and not cnt[list(ref.MANY_EMPTY)].any()
    assert (cnt[[b for b in range(ref.MANY_B) if b not in ref.MANY_EMPTY and b > 255]] > 0).any(), 'samples of the second trip hold rows'


def check_max_out_0_and_1(dev):
    """the static form at max_out 0 and 1: the tables equal the restatement, num[1] is still the true count, a layer over them returns
    (0, C) / (1, C) in fp32 and in bf16 with finite parameter gradients (zeros at max_out 0)"""
    name = 's2p1_max_out_at'
    case, true = ref.CASES[name], ref.CASES[name]['max_out']
    X, W, bias, gY = (torch.from_numpy(a).to(dev) for a in ref.operands(name))
    for m in (0, 1):
        want = ref.index_ref(case['coors'], case['shape'], case['B'], case['kernel'], case['stride'], case['padding'], case['subm'], m)
        got = run_index(case, dev, max_out=m)
        for k in INT_OUTPUTS:
            assert np.array_equal(getattr(got, k).cpu().numpy(), want[k]), f'max_out {m}: {k} differs from the restatement on {dev}'
        assert want['num'].tolist() == [m, true] and got.nbr_t.max().item() <= m - 1 and got.out_batch_cnt.sum().item() == m
        for dtype in (None, torch.bfloat16):
            x, w, b = X.clone().requires_grad_(True), W.clone().requires_grad_(True), bias.clone().requires_grad_(True)
            out = amd.sparse_conv(x, w, b, got, compute_dtype=dtype)
            assert out.shape == (m, W.shape[2]) and out.dtype == (dtype or torch.float32)
            gx, gw, gb = torch.autograd.grad(out, [x, w, b], gY[:m].to(out.dtype))
            assert gx.shape == x.shape and gw.shape == w.shape and gb.shape == b.shape
            assert all(torch.isfinite(g).all() for g in (gx, gw, gb))
            if m == 0:
                assert not gx.any() and not gw.any() and not gb.any()
            elif dtype is None:                                          # the one row against the gather - matmul oracle, the derived bound
                o64 = ref.sparse_oracle(want, *(a.cpu().numpy() for a in (X, W, bias, gY[:1])))
                A = ref.sparse_oracle(want, *(a.abs().cpu().numpy() for a in (X, W, bias, gY[:1])))
                L = ref.term_counts(want, len(X), W.shape[1], W.shape[2], True)
                for k, g in (('out', out.detach()), ('gx', gx), ('gw', gw), ('gb', gb)):
                    assert ref.within_bound(g.cpu().numpy(), o64[k], A[k], L[k])[0], f'max_out 1: {k} misses the bound on {dev}'
                assert gw.any() and gb.any()


def check_batch_zero(dev):
    """B = 0 with N > 0: every row is inactive, the counts are zero, out_batch_cnt is empty, a layer over the tables gives zeros"""
    base = ref.CASES['s2p1_max_out_at']
    coors = torch.from_numpy(base['coors']).to(dev)
    N = len(coors)
    for geom, max_out in (('subm', None), ('s2p1', None), ('s2p1', 5)):
        k, s, p, subm = ref.GEOMS[geom]
        want = ref.index_ref(base['coors'], base['shape'], 0, k, s, p, subm, max_out)
        got = amd.sparse_conv_index(coors, base['shape'], 0, k, s, p, subm, max_out)
        R = N if subm else (max_out or 0)
        assert tuple(got.out_shape) == tuple(want['out_shape']) and got.nbr.shape == (R, 27) and got.out_batch_cnt.shape == (0,)
        for key in INT_OUTPUTS:
            if want[key] is not None:
                assert np.array_equal(getattr(got, key).cpu().numpy(), want[key]), f'{geom}: {key} differs from the restatement on {dev}'
        assert got.num.tolist() == [R if subm else 0, R if subm else 0] and (got.nbr == -1).all() and (subm or (got.nbr_t == -1).all())
        assert (got.out_coors == (coors if subm else -1)).all()
        x, w, b = (torch.ones(N, 4, device=dev).requires_grad_(True), torch.ones(27, 4, 8, device=dev).requires_grad_(True),
                   torch.ones(8, device=dev).requires_grad_(True))
        out = amd.sparse_conv(x, w, b, got)
        grads = torch.autograd.grad(out, [x, w, b], torch.ones_like(out))
        assert out.shape == (R, 8) and not out.any() and not any(g.any() for g in grads)


def check_nonfinite_containment(name, dev, dtype=None):
    """+inf and NaN in two channels of one input row i, -inf in one channel c of one live grad_out row o, against the same entry point on
    the clean operands: what does not read the poisoned value keeps its bits, what reads it is non-finite (include/gd3d.h: NaN and inf
    pass through).  dtype None: the fp32 path, else the 16-bit path of that type."""
    case, nbr = ref.CASES[name], ref.expected_index(name)['nbr']
    X, W, bias, gY = (torch.from_numpy(a).clone() for a in ref.operands(name))
    live = (nbr >= 0).any(1)
    i, o, c = int(nbr[nbr >= 0][0]), int(np.nonzero(live)[0][-1]), 3
    Xp, gYp = X.clone(), gY.clone()
    Xp[i, 0], Xp[i, 1], gYp[o, c] = float('inf'), float('nan'), float('-inf')
    index = run_index(case, dev)

    def run(x, g):
        x, g = (x if dtype is None else x.to(dtype)).to(dev).requires_grad_(True), (g if dtype is None else g.to(dtype)).to(dev)
        w, b = W.to(dev).requires_grad_(True), bias.to(dev).requires_grad_(True)
        out = amd.sparse_conv(x, w, b, index, compute_dtype=dtype)
        grads = torch.autograd.grad(out, [x, w, b], g)
        return [t.detach().float().cpu().numpy() for t in (out,) + grads]      # exact: the 16-bit values widen without rounding
    clean, dirty = run(X, gY), run(Xp, gYp)
    assert all(np.isfinite(a).all() for a in clean)
    same = lambda a, b: a.tobytes() == b.tobytes()
    reads_i = (nbr == i).any(1)                                          # outputs that read row i
    read_by_o = np.zeros(len(X), bool)
    read_by_o[nbr[o][nbr[o] >= 0]] = True                                # inputs that row o reads
    dirty_j = (nbr == i).any(0) | (nbr[o] >= 0)                          # offsets whose weight gradient sees X[i] or gY[o]
    assert reads_i.any() and not reads_i.all() and read_by_o.any() and not read_by_o.all() and dirty_j.any() and not dirty_j.all()
    who = f'{name} {dtype or "fp32"} on {dev}'
    for k, (a, b), hit in (('out', (clean[0], dirty[0]), reads_i), ('gx', (clean[1], dirty[1]), read_by_o), ('gw', (clean[2], dirty[2]), dirty_j)):
        assert same(a[~hit], b[~hit]), f'{who}: {k}: an entry that does not read the non-finite value changed'
        flat = b[hit].reshape(int(hit.sum()), -1)
        assert (~np.isfinite(flat)).any(1).all(), f'{who}: {k}: an entry that reads the non-finite value is finite'
    col = np.arange(len(bias)) == c
    assert same(clean[3][~col], dirty[3][~col]) and not np.isfinite(dirty[3][c]), f'{who}: gb'


def check_modules_equal_functional(dev):
    """SubMConv3d / SparseConv3d forward and parameter gradients equal sparse_conv over sparse_conv_index, bit for bit"""
    torch.manual_seed(3)
    case = ref.CASES['s2p1_9x12x10_c5_16']
    coors = torch.from_numpy(case['coors']).to(dev)
    feats = torch.randn(len(coors), 5, device=dev)
    for cls, geom in ((amd.SubMConv3d, 'subm'), (amd.SparseConv3d, 's2p1'), (amd.SparseConv3d, 's2p011'), (amd.SparseConv3d, 'down')):
        k, s, p, subm = ref.GEOMS[geom]
        layer = cls(5, 16, k, s, p, bias=True).to(dev)
        assert tuple(layer.weight.shape) == tuple(k) + (5, 16) and layer.bias.shape == (16,)
        x = amd.SparseConvTensor(feats.clone().requires_grad_(True), coors, case['shape'], case['B'])
        y = layer(x)
        index = amd.sparse_conv_index(coors, case['shape'], case['B'], k, s, p, subm)
        f = feats.clone().requires_grad_(True)
        want = amd.sparse_conv(f, layer.weight, layer.bias, index)
        assert torch.equal(y.features, want) and torch.equal(y.indices, index.out_coors) and list(y.spatial_shape) == list(index.out_shape)
        assert y.batch_size == case['B'] and y.indice_dict is x.indice_dict
        g = torch.randn_like(want)
        got = torch.autograd.grad(y.features, [x.features, layer.weight, layer.bias], g)
        exp = torch.autograd.grad(want, [f, layer.weight, layer.bias], g)
        for a, b in zip(got, exp):
            assert torch.equal(a, b)
        assert got[1].shape == layer.weight.shape


def count_calls(monkeypatch):
    """counts the `_host.call`s by entry point"""
    calls, real = {}, _host.call

    def counting(name, dev, args, cpu_tail=()):
        calls[name] = calls.get(name, 0) + 1
        return real(name, dev, args, cpu_tail)
    monkeypatch.setattr(_host, 'call', counting)
    return calls


def check_shared_indice_key(dev, monkeypatch):
    """two layers under one indice_key build ONE index; without a key every layer builds its own"""
    case = ref.CASES['subm_9x12x10_c4_16']
    coors = torch.from_numpy(case['coors']).to(dev)
    torch.manual_seed(4)
    net = amd.SparseSequential(amd.SubMConv3d(4, 16, 3, indice_key='a', bias=False), torch.nn.BatchNorm1d(16), torch.nn.ReLU(),
                               amd.SubMConv3d(16, 16, 3, indice_key='a'), amd.SparseConv3d(16, 32, 3, 2, 1, indice_key='down'),
                               amd.SubMConv3d(32, 32, 3, indice_key='b'), amd.SubMConv3d(32, 32, 3, indice_key='b')).to(dev).eval()
    calls = count_calls(monkeypatch)
    x = amd.SparseConvTensor(torch.randn(len(coors), 4, device=dev), coors, case['shape'], case['B'])
    y = net(x)
    assert calls['gd3d_sparse_conv_index'] == 3 and calls['gd3d_sparse_conv_forward'] == 5, calls
    assert set(y.indice_dict) == {'a', 'down', 'b'} and y.features.shape[1] == 32
    loose = amd.SparseSequential(amd.SubMConv3d(4, 16, 3), amd.SubMConv3d(16, 16, 3)).to(dev)
    calls.clear()
    loose(amd.SparseConvTensor(torch.randn(len(coors), 4, device=dev), coors, case['shape'], case['B']))
    assert calls['gd3d_sparse_conv_index'] == 2


def check_dense(dev):
    """dense() and its gradient equal index_put / gather in torch; inactive rows are skipped and get a zero gradient"""
    case = ref.CASES['subm_inactive_rows_scattered_and_tail']
    coors = torch.from_numpy(case['coors']).to(dev)
    D, H, W = case['shape']
    torch.manual_seed(5)
    for C in (1, 5, 64):
        feats = torch.randn(len(coors), C, device=dev, requires_grad=True)
        dense = amd.SparseConvTensor(feats, coors, case['shape'], case['B']).dense()
        act = torch.from_numpy(ref.active_rows(case['coors'], case['shape'], case['B'])).to(dev)
        c = coors[act].long()
        want = torch.zeros(case['B'], D, H, W, C, device=dev).index_put((c[:, 0], c[:, 1], c[:, 2], c[:, 3]), feats.detach()[act]).permute(0, 4, 1, 2, 3)
        assert dense.shape == (case['B'], C, D, H, W) and torch.equal(dense, want)
        g = torch.randn_like(dense)
        (gx,) = torch.autograd.grad(dense, feats, g)
        wx = torch.zeros_like(gx)
        wx[act] = g.permute(0, 2, 3, 4, 1)[c[:, 0], c[:, 1], c[:, 2], c[:, 3]]
        assert torch.equal(gx, wx)
    assert amd.sparse_to_dense(torch.zeros(0, 3, device=dev), torch.zeros(0, 4, dtype=torch.int32, device=dev), (2, 3, 4), 2).abs().sum() == 0


# ---- MlvlSparseEncoder against a per-layer fp64 oracle ------------------------------------------------------------------------------

ENC_B = 2
ENC_SHAPES = ((9, 48, 40), (25, 24, 20))     # at D = 9 the last stage leaves D = 1 and conv_out's (3, 1, 1) kernel no output cell: an empty map


def encoder_inputs(shape):
    rng = np.random.default_rng(31)
    coors = ref.random_coors(rng, 700, shape, ENC_B)
    coors = coors[np.lexsort((coors[:, 3], coors[:, 2], coors[:, 1], coors[:, 0]))]          # grouped by sample, as voxelization gives them
    feats = rng.standard_normal((len(coors), 4)).astype(np.float32)
    return coors, feats


def build_encoder(dev, shape):
    torch.manual_seed(6)
    enc = amd.MlvlSparseEncoder(in_channels=4, sparse_shape=list(shape), order=('conv', 'norm', 'act'))
    for m in enc.modules():                                              # running statistics a trained model would hold
        if isinstance(m, torch.nn.BatchNorm1d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.normal_(0, 0.1)
    return enc.to(dev).eval()


def conv_bn_relu_64(block, coors, shape, B, x64, e64):
    """One conv -> BatchNorm1d(eval) -> ReLU block in fp64 through the dense oracle, with the bound of the fp32 evaluation's error.

    x64: the fp64 features; e64 >= |fp32 features - x64| elementwise.  The fp32 layer computes conv(x32) with error at most
    (L + 2) u conv(|x32|, |W|), and conv(x32) differs from conv(x64) by at most conv(e, |W|): so
      e_conv = conv(e, |W|) + (L + 2) u conv(|x64| + e, |W|).
    BatchNorm1d in eval is y = (x - mean) * s + beta, s = gamma / sqrt(var + eps): at most 6 fp32 roundings of magnitudes up to
    |s| (|x| + |mean|) + |beta|, so e_bn = |s| e_conv + 8 u (|s| (|x| + e_conv + |mean|) + |beta|).  ReLU does not enlarge an error."""
    conv, bn = block[0], block[1]
    index = ref.index_ref(coors, shape, B, conv.kernel_size, conv.stride, conv.padding, conv.subm)
    W = conv.weight.detach().cpu().double().numpy().reshape(-1, conv.in_channels, conv.out_channels)
    R = len(index['nbr'])
    zeros = np.zeros((R, conv.out_channels))
    if R == 0:                                                           # the kernel does not fit the grid: no output cell (conv3d would raise)
        return index, zeros, zeros
    y = ref.oracle(coors, shape, B, conv.kernel_size, conv.stride, conv.padding, index, x64, W, None, zeros)['out']
    absW = np.abs(W)
    spread = ref.oracle(coors, shape, B, conv.kernel_size, conv.stride, conv.padding, index, e64, absW, None, zeros)['out']
    scale = ref.oracle(coors, shape, B, conv.kernel_size, conv.stride, conv.padding, index, np.abs(x64) + e64, absW, None, zeros)['out']
    L = (index['nbr'] >= 0).sum(1)[:, None] * conv.in_channels
    e_conv = spread + (L + 2) * ref.U * scale
    mean, var = bn.running_mean.cpu().double().numpy(), bn.running_var.cpu().double().numpy()
    gamma, beta = bn.weight.detach().cpu().double().numpy(), bn.bias.detach().cpu().double().numpy()
    s = gamma / np.sqrt(var + bn.eps)
    out = (y - mean) * s + beta
    e_bn = np.abs(s) * e_conv + 8 * ref.U * (np.abs(s) * (np.abs(y) + e_conv + np.abs(mean)) + np.abs(beta))
    return index, np.maximum(out, 0.0), e_bn


def check_encoder(dev, grid):
    coors, feats = encoder_inputs(grid)
    enc = build_encoder(dev, grid)
    with torch.no_grad():
        got = enc(torch.from_numpy(feats).to(dev), torch.from_numpy(coors).to(dev), ENC_B)
    assert set(got) == {'encode_features', 'spatial_features'} and len(got['encode_features']) == 4
    x64, e64, c, shape = feats.astype(np.float64), np.zeros(feats.shape), coors, grid
    _, x64, e64 = conv_bn_relu_64(enc.conv_input, c, shape, ENC_B, x64, e64)
    worst = 0.0
    for k, stage in enumerate(enc.encoder_layers):
        for block in stage:
            index, x64, e64 = conv_bn_relu_64(block, c, shape, ENC_B, x64, e64)
            if not block[0].subm:
                c, shape = index['out_coors'], index['out_shape']
        level = got['encode_features'][k]
        assert level.indices.dtype == torch.int32 and np.array_equal(level.indices.cpu().numpy(), c), f'level {k}: indices differ from the chained restatement'
        assert list(level.spatial_shape) == list(shape) and level.batch_size == ENC_B
        err = np.abs(level.features.cpu().double().numpy() - x64)
        assert (err <= e64).all(), f'level {k}: features miss the chained bound by up to {(err - e64).max():.3e}'
        worst = max(worst, float((err / np.maximum(e64, 1e-300)).max()))
        # a level's indices feed the voxel-centre source of the keypoint encoder as they are
        xyz, cnt = amd.voxel_centers(level.indices, (0.05, 0.05, 0.1), (0, -40, -3, 70.4, 40, 1), 2 ** k, 'half', ENC_B)
        assert xyz.shape == (len(c), 3) and cnt.tolist() == np.bincount(c[:, 0], minlength=ENC_B).tolist()
    if grid == (9, 48, 40):
        assert [list(f.spatial_shape) for f in got['encode_features']] == [[9, 48, 40], [5, 24, 20], [3, 12, 10], [1, 6, 5]]
    index, x64, e64 = conv_bn_relu_64(enc.conv_out, c, shape, ENC_B, x64, e64)
    oc, (D, H, W) = index['out_coors'].astype(np.int64), index['out_shape']
    dense, bound = np.zeros((ENC_B, 128, D, H, W)), np.zeros((ENC_B, 128, D, H, W))
    dense[oc[:, 0], :, oc[:, 1], oc[:, 2], oc[:, 3]] = x64
    bound[oc[:, 0], :, oc[:, 1], oc[:, 2], oc[:, 3]] = e64
    sp = got['spatial_features']
    assert sp.shape == (ENC_B, 128 * D, H, W) and sp.dtype == torch.float32
    err = np.abs(sp.cpu().double().numpy().reshape(dense.shape) - dense)
    assert (err <= bound).all(), f'spatial_features miss the chained bound by up to {(err - bound).max():.3e}'
    print(f'MlvlSparseEncoder on {dev}: worst error / chained bound over the levels {worst:.3f}, spatial_features {float((err / np.maximum(bound, 1e-300)).max(initial=0.0)):.3f}')
    plain = amd.SparseEncoder(4, list(grid), block_type='basicblock', encoder_channels=((16, 16, 32), (32, 32, 64), (64, 64, 128), (128, 128)),
                              encoder_paddings=((0, 0, 1), (0, 0, 1), (0, 0, (0, 1, 1)), (0, 0))).to(dev).eval()
    with torch.no_grad():
        out = plain(torch.from_numpy(feats).to(dev), torch.from_numpy(coors).to(dev), ENC_B)
    assert out.dim() == 4 and out.shape[0] == ENC_B and out.shape[1] % 128 == 0 and torch.isfinite(out).all()


def check_bad_arguments(dev):
    c = torch.from_numpy(ref.CASES['subm_rows_tile']['coors']).to(dev)
    shape = (9, 12, 10)
    idx = amd.sparse_conv_index(c, shape, 2, 3, 1, 1, True)
    x, w = torch.zeros(len(c), 4, device=dev), torch.zeros(27, 4, 8, device=dev)
    bad = [lambda: amd.sparse_conv_index(c, shape, 2, 3, 1, 1, True, dilation=2), lambda: amd.sparse_conv_index(c, shape, 2, 2, 1, 1, True),
           lambda: amd.sparse_conv_index(c, shape, 2, 3, 2, 1, True), lambda: amd.sparse_conv_index(c, shape, 2, 3, 1, 0, True),
           lambda: amd.sparse_conv_index(c, shape, 2, 4, 1, 0, False), lambda: amd.sparse_conv_index(c, shape, 2, 3, 0, 0, False),
           lambda: amd.sparse_conv_index(c, shape, 2, 3, 1, -1, False), lambda: amd.sparse_conv_index(c, (0, 12, 10), 2, 3, 1, 0, False),
           lambda: amd.sparse_conv_index(c[:, :3], shape, 2, 3, 1, 1, True), lambda: amd.sparse_conv_index(c.float(), shape, 2, 3, 1, 1, True),
           lambda: amd.sparse_conv_index(c, shape[:2], 2, 3, 1, 1, True), lambda: amd.sparse_conv_index(c, shape, -1, 3, 1, 1, True),
           lambda: amd.sparse_conv_index(c, shape, 2, 3, 2, 1, False, max_out=-1),
           lambda: amd.sparse_conv(x[:-1], w, None, idx), lambda: amd.sparse_conv(x, w[:9], None, idx), lambda: amd.sparse_conv(x, w, torch.zeros(7, device=dev), idx),
           lambda: amd.sparse_conv(x, torch.zeros(27, 5, 8, device=dev), None, idx), lambda: amd.sparse_conv(x, w, None, (idx.nbr,)),
           lambda: amd.sparse_conv(x.int(), w, None, idx), lambda: amd.sparse_conv(torch.zeros(len(c), 300, device=dev), torch.zeros(27, 300, 8, device=dev), None, idx),
           lambda: amd.sparse_to_dense(x[:-1], c, shape, 2), lambda: amd.sparse_to_dense(x, c, shape, -1),
           lambda: amd.SubMConv3d(4, 8, 3, dilation=2), lambda: amd.SubMConv3d(4, 8, 2), lambda: amd.SparseConv3d(4, 300, 3), lambda: amd.SparseConv3d(4, 8, 4),
           lambda: amd.SubMConv3d(4, 8, 3).to(dev)(x), lambda: amd.make_sparse_convmodule(4, 8, 3, 'k', conv_type='SparseInverseConv3d'),
           lambda: amd.SparseEncoder(4, shape, block_type='other'), lambda: amd.SparseEncoder(4, shape, order=('conv', 'norm'))]
    for i, call in enumerate(bad):
        with pytest.raises(RuntimeError):
            call()
            pytest.fail(f'call {i} did not raise')
    stale = amd.SparseConvTensor(x[:10], c[:10], shape, 2)
    stale.indice_dict['k'] = idx                                        # an index over other rows under the layer's key
    with pytest.raises(RuntimeError, match='indice_key'):
        amd.SubMConv3d(4, 8, 3, indice_key='k').to(dev)(stale)


# ---- the tests -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', sorted(ref.CASES))
def test_index_twin_equals_the_restatement(name):
    check_index(name, 'cpu')


@pytest.mark.parametrize('name', VALUE_CASES)
def test_values_twin_within_the_derived_bound_of_the_fp64_oracle(name):
    check_values(name, 'cpu')


@pytest.mark.parametrize('name', SWEEPS)
def test_sweep_of_20000_rows(name):
    check_index(name, 'cpu')
    check_values(name, 'cpu')


def test_the_cases_hold_what_they_claim():
    e = ref.expected_index
    for geom in ('s2p1', 's2p011', 'down'):                              # the restated active set is conv3d(mask, ones) > 0, exactly
        for shape in ((9, 12, 10), (7, 11, 13)):
            name = [n for n in ref.CASES if n.startswith(f'{geom}_{shape[0]}x')][0]
            c = ref.CASES[name]
            mask = torch.zeros((c['B'], 1) + c['shape'], dtype=torch.float64)
            cc = torch.from_numpy(c['coors']).long()
            mask[cc[:, 0], 0, cc[:, 1], cc[:, 2], cc[:, 3]] = 1
            hit = torch.nn.functional.conv3d(mask, torch.ones((1, 1) + c['kernel'], dtype=torch.float64), stride=c['stride'], padding=c['padding'])[:, 0] > 0
            assert np.array_equal(hit.nonzero().numpy(), e(name)['out_coors']) and e(name)['out_batch_cnt'][1] == 0, name
    assert ref.out_shape_of((7, 11, 13), *ref.GEOMS['s2p011'][:3]) == (3, 6, 7) and ref.out_shape_of((7, 11, 13), *ref.GEOMS['down'][:3]) == (3, 11, 13)
    assert (e('subm_dense_block_4x4x4')['nbr'].reshape(4, 4, 4, 27)[1:3, 1:3, 1:3] >= 0).all()              # the interior: every neighbour valid
    lone = e('subm_isolated')['nbr']
    assert (lone[:, 13] == np.arange(len(lone))).all() and (np.delete(lone, 13, 1) == -1).all()               # only the centre offset
    wraps = ref.CASES['subm_faces_corners_and_wraps']
    n_w = len(wraps['coors'])
    nbr = e('subm_faces_corners_and_wraps')['nbr']
    assert (np.delete(nbr[n_w - 4:], 13, 1) == -1).all(), 'a wrap-around neighbour was found'
    mixed = e('subm_inactive_rows_scattered_and_tail')
    act = ref.active_rows(ref.CASES['subm_inactive_rows_scattered_and_tail']['coors'], (9, 12, 10), 2)
    assert (~act).sum() == 19 and (mixed['nbr'][~act] == -1).all() and not np.isin(mixed['nbr'], np.nonzero(~act)[0]).any()
    big = ref.CASES['subm_keys_past_31_bits']
    assert big['B'] * int(np.prod(big['shape'])) > 2 ** 31 and (e('subm_keys_past_31_bits')['nbr'] >= 0).sum() > 2 * len(big['coors'])
    below, at, above = (e(f's2p1_max_out_{k}') for k in ('below', 'at', 'above'))
    assert below['num'][0] == below['num'][1] - 7 and at['num'][0] == at['num'][1] and len(above['nbr']) == above['num'][0] + 9
    assert below['nbr_t'].max() == below['num'][0] - 1 and np.array_equal(below['out_coors'], at['out_coors'][:len(below['out_coors'])])
    dup = e('subm_duplicates')['nbr']
    assert (dup[40:50, 13] == np.arange(10, 20)).all(), 'a look-up of a duplicated cell finds the lowest row'
    sub = e('subm_9x12x10_c4_16')
    assert np.array_equal(sub['nbr'][sub['nbr'][:, 5].clip(0), 26 - 5][sub['nbr'][:, 5] >= 0], np.nonzero(sub['nbr'][:, 5] >= 0)[0])   # nbr_t[i, j] = nbr[i, K-1-j]
    # the further geometries
    assert len(ref.MORE_GEOMS) == 15 and not set(ref.MORE_GEOMS) & set(ref.GEOMS)
    assert sorted(int(np.prod(g[0])) for g, _, _ in ref.MORE_GEOMS.values()) == [1, 1, 3, 8, 8, 9, 9, 18, 25, 25, 27, 27, 27, 27, 27]
    for geom, (g, cin, cout) in ref.MORE_GEOMS.items():
        name = ref.MORE_GEOM_CASES[geom]
        c, idx = ref.CASES[name], e(name)
        assert (c['kernel'], c['stride'], c['padding'], c['subm'], c['cin'], c['cout']) == g + (cin, cout)
        assert len(np.unique(c['coors'], axis=0)) == 150 and c['B'] == 3 and 1 not in c['coors'][:, 0] and c['shape'] in ((9, 12, 10), (7, 11, 13))
        K = idx['nbr'].shape[1]
        if c['subm']:                                                    # the transpose a submanifold input gradient reads: nbr_t[i, j] = nbr[i, K-1-j]
            o, j = np.nonzero(idx['nbr'] >= 0)
            assert np.array_equal(idx['nbr'][idx['nbr'][o, j], K - 1 - j], o), name
        else:                                                            # the restated active set is conv3d(mask, ones) > 0, exactly
            mask = torch.zeros((c['B'], 1) + c['shape'], dtype=torch.float64)
            cc = torch.from_numpy(c['coors']).long()
            mask[cc[:, 0], 0, cc[:, 1], cc[:, 2], cc[:, 3]] = 1
            hit = torch.nn.functional.conv3d(mask, torch.ones((1, 1) + c['kernel'], dtype=torch.float64), stride=c['stride'], padding=c['padding'])[:, 0] > 0
            assert np.array_equal(hit.nonzero().numpy(), idx['out_coors']) and idx['out_batch_cnt'][1] == 0, name
    far = e(ref.MORE_GEOM_CASES['k3s4p0'])                                # a stride above the kernel: inputs that no output reads
    assert ((far['nbr_t'] == -1).all(1)).any() and (far['nbr'] >= 0).any()
    wide = e(ref.MORE_GEOM_CASES['k3s1p1'])                               # R >> N: more rows gathered from than written in the input gradient
    assert len(wide['nbr']) > 5 * 150
    grown = ref.CASES[ref.MORE_GEOM_CASES['k2s1p1']]
    assert all(o > n for o, n in zip(e(ref.MORE_GEOM_CASES['k2s1p1'])['out_shape'], grown['shape']))
    tiny = ref.CASES[ref.MORE_GEOM_CASES['subm_k1']]                      # K Cr < 32: the whole reduction axis is one padded step of the 16-bit kernel
    assert 1 * tiny['cin'] < 32 and 27 * ref.CASES[ref.MORE_GEOM_CASES['k3s3p2']]['cin'] < 32
    # the channel edges
    lib = _lib.load()
    top = ref.CASES['subm_c256_256_rows_400']
    assert (len(top['coors']), top['cin'], top['cout']) == (400, 256, 256) and (64 << 20) // (27 * 256 * 256 * 4) == 9
    per_part = 27 * 256 * 256 * 4 + 256 * 4                               # 7 chunks of 64 rows (the 64 MiB cap), not 13 of 32
    assert lib.gd3d_sparse_conv_backward_weight_workspace_bytes(400, 27, 256, 256) == 7 * per_part
    assert 9 < 13 < 64 and -(-400 // 64) == 7 and -(-400 // 32) == 13
    assert (ref.CASES['s2p1_c256_256']['cin'], ref.CASES['down_c1_1']['cout']) == (256, 1)
    assert [(ref.CASES[n]['cin'] % 8, ref.CASES[n]['cout'] % 8) for n in ('subm_c16_20', 's2p1_c40_8')] == [(0, 4), (0, 0)]
    # the dead tiles
    lo, hi = ref.DEAD_ROWS
    for geom in ('subm', 's2p1'):
        c = ref.CASES[f'{geom}_inactive_block']
        act = ref.active_rows(c['coors'], c['shape'], c['B'])
        assert len(act) == 300 and (c['coors'][lo:hi] == -1).all() and not act[lo:hi].any() and act[:lo].all() and act[hi:].all()
        assert lo % ref.TILE_M == 0 and hi % 128 == 0 and hi - lo >= 128 + ref.TILE_M          # whole tiles of both kernels, a whole 16-bit workgroup
        assert not np.isin(e(f'{geom}_inactive_block')['nbr'], np.arange(lo, hi)).any()
    far = e('s2p1_max_out_far_above')
    assert len(far['nbr']) == far['num'][1] + 200 and far['num'][0] == far['num'][1] and (far['nbr'][far['num'][0]:] == -1).all()
    assert len(far['nbr']) // 128 > -(-int(far['num'][0]) // 128)         # a 16-bit workgroup (and fp32 tiles) wholly past num[0]
    for geom in ('subm', 's2p1'):
        c, nbr = ref.CASES[f'{geom}_isolated_c64_64'], e(f'{geom}_isolated_c64_64')['nbr']
        assert c['bias'] and (c['cin'], c['cout']) == (64, 64) and 64 * (27 * 64 + 8) * 2 > 32 << 10           # the 16-bit weight is staged in chunks
        assert ((nbr >= 0).sum(1) == 1).all()                             # one offset a row: every other chunk is skipped
    lone = e('subm_isolated_c64_64')['nbr']
    assert (lone[:, 13] == np.arange(len(lone))).all() and (np.delete(lone, 13, 1) == -1).all()               # only the centre offset


def test_dynamic_form_returns_exact_size_views():
    case, want = ref.CASES['s2p1_max_out_at'], ref.expected_index('s2p1_max_out_at')
    got = run_index(case, 'cpu', max_out=None)
    for k in INT_OUTPUTS:
        assert np.array_equal(getattr(got, k).numpy(), want[k]), k


@pytest.mark.parametrize('geom', ['subm', 's2p1'])
def test_index_over_300_samples(geom):
    check_many_samples(geom, 'cpu')


def test_static_form_at_max_out_0_and_1():
    check_max_out_0_and_1('cpu')


def test_batch_size_zero_leaves_every_row_inactive():
    check_batch_zero('cpu')


@pytest.mark.parametrize('name', ['subm_9x12x10_c4_16', 's2p1_9x12x10_c5_16'])
def test_a_non_finite_value_reaches_only_what_reads_it(name):
    check_nonfinite_containment(name, 'cpu')


def test_other_dtypes_are_evaluated_in_fp32_and_cast_back():
    name = 'subm_9x12x10_c4_16'
    X, W, bias, gY = (torch.from_numpy(a) for a in ref.operands(name))
    index = run_index(ref.CASES[name], 'cpu')
    x = X.double().requires_grad_(True)
    out = amd.sparse_conv(x, W.double(), bias.double(), index)
    (gx,) = torch.autograd.grad(out, x, gY.double())
    assert out.dtype == torch.float64 and gx.dtype == torch.float64
    assert torch.equal(out.float(), amd.sparse_conv(X, W, bias, index)) and torch.equal(amd.sparse_conv(X, W.reshape(3, 3, 3, 4, 16), bias, index), out.float())
    long_index = amd.sparse_conv_index(torch.from_numpy(ref.CASES[name]['coors']).long(), (9, 12, 10), 3, 3, 1, 1, True)
    assert torch.equal(long_index.nbr, index.nbr)


def test_modules_equal_the_functional_form():
    check_modules_equal_functional('cpu')


def test_layers_sharing_an_indice_key_build_one_index(monkeypatch):
    check_shared_indice_key('cpu', monkeypatch)


def test_dense_and_its_gradient_equal_index_put_and_gather():
    check_dense('cpu')


@pytest.mark.parametrize('grid', ENC_SHAPES)
def test_mlvl_sparse_encoder_follows_the_per_layer_fp64_oracle(grid):
    check_encoder('cpu', grid)


def test_bad_arguments_raise():
    check_bad_arguments('cpu')
    lib = _lib.load()                                                      # the C entry points' own codes: nothing is touched
    i3 = lambda *v: (ctypes.c_int32 * 3)(*v)
    num, cnt = np.zeros(2, np.int64), np.zeros(2, np.int32)
    tail = (None, None, None, None, num.ctypes.data, cnt.ctypes.data)
    idx = lambda n, shape, k, s, p, subm, mo=0: lib.gd3d_sparse_conv_index_cpu(None, n, 2, i3(*shape), i3(*k), i3(*s), i3(*p), subm, mo, *tail)
    assert idx(0, (9, 12, 10), (3, 3, 3), (1, 1, 1), (1, 1, 1), 1) == 0 and num.tolist() == [0, 0]
    assert idx(0, (9, 12, 10), (3, 3, 3), (2, 1, 1), (1, 1, 1), 1) == 10001 and idx(0, (9, 12, 10), (3, 3, 2), (1, 1, 1), (1, 1, 1), 1) == 10001
    assert idx(0, (9, 12, 10), (3, 3, 4), (1, 1, 1), (0, 0, 0), 0) == 10002                                   # K = 36
    assert idx(1 << 31, (9, 12, 10), (3, 3, 3), (1, 1, 1), (1, 1, 1), 1) == 10002 and idx(1 << 27, (9, 12, 10), (3, 3, 3), (1, 1, 1), (1, 1, 1), 1) == 10002
    assert lib.gd3d_sparse_conv_index_cpu(None, 0, 1 << 30, i3(1 << 24, 1 << 24, 1 << 24), i3(1, 1, 1), i3(1, 1, 1), i3(0, 0, 0), 0, 0, *tail) == 10002
    assert lib.gd3d_sparse_conv_forward_cpu(None, None, None, None, None, 4, 4, 27, 0, 8, None) == 10001
    assert lib.gd3d_sparse_conv_forward_cpu(None, None, None, None, None, 4, 4, 27, 257, 8, None) == 10002
    assert lib.gd3d_sparse_conv_forward_cpu(None, None, None, None, None, 4, 4, 28, 8, 8, None) == 10002
    assert lib.gd3d_sparse_conv_forward_cpu(None, None, None, None, None, 4, 0, 27, 8, 8, None) == 0          # R == 0: nothing to do
    assert lib.gd3d_sparse_conv_backward_input_cpu(None, None, None, 1, 4, 5, 27, 8, 8, None) == 10001         # flip needs N == R
    assert lib.gd3d_sparse_conv_backward_weight_cpu(None, None, None, None, 4, 4, 27, 8, 8, None, None, None) == 10001      # no grad_weight
    assert lib.gd3d_sparse_to_dense_cpu(None, None, 4, 0, 2, 3, 3, 3, None) == 10001
    assert lib.gd3d_sparse_conv_index_workspace_bytes(0, 27, 1) == 256 and lib.gd3d_sparse_conv_index_workspace_bytes(64000, 27, 0) % 256 == 0
    assert lib.gd3d_sparse_conv_backward_weight_workspace_bytes(64000, 27, 128, 128) <= (64 << 20) + 64 * 512 + 512
    for name in ('sparse_conv_index', 'sparse_conv', 'sparse_to_dense', 'SparseConvTensor', 'SubMConv3d', 'SparseConv3d', 'SparseSequential',
                 'SparseBasicBlock', 'make_sparse_convmodule', 'SparseEncoder', 'MlvlSparseEncoder'):
        assert name in amd.__all__
