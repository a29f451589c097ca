"""The fused loss launch walks its tiles in either order: a launch on the same target and row count as the previous fused
launch of its stream runs opposite to it (so that it starts on the target rows still in the Infinity Cache), any other
launch ascends.  The order must change nothing: repeated calls on one target, which alternate direction, return
bit-identical losses and gradients, on every path of the kernel (partial last tile, unaligned rows, (N,7) weights with and
without positives, target gradient, bbox-coder prologues, single-launch finish and two-stage reduce)."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = (1, 255, 256, 16_384, 16_385, 1_000_003)


@pytest.fixture(scope='module')
def amd():
    import mmdet3d_gaussian_amd as m
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    m.load_library()
    return m


def _pairs(n, seed):
    g = torch.Generator().manual_seed(seed)
    lo = torch.tensor([0, -40, -3, 0.5, 0.5, 0.5, -np.pi])
    hi = torch.tensor([70, 40, 1, 2.5, 4.5, 2.0, np.pi])
    t = torch.rand(n, 7, generator=g) * (hi - lo) + lo
    p = t + torch.randn(n, 7, generator=g) * torch.tensor([0.3, 0.3, 0.1, 0.1, 0.1, 0.1, 0.1])
    return p.float().cuda(), t.float().cuda()


def _call(mod, pred, target, grad_target=False, **kw):
    """One forward + backward; returns every output as host arrays (loss values, pred gradient, target gradient)."""
    p = pred.detach().clone().requires_grad_(True)
    t = target
    if grad_target:
        t = target.detach().clone().requires_grad_(True)
    out = mod(p, t, **kw)
    (out.sum() if out.dim() else out).backward()
    torch.cuda.synchronize()
    res = [out.detach().cpu().numpy(), p.grad.cpu().numpy()]
    if grad_target:
        res.append(t.grad.cpu().numpy())
    return res


def _same(runs):
    first = runs[0]
    for r in runs[1:]:
        assert len(r) == len(first)
        for a, b in zip(first, r):
            assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), 'outputs depend on tile order'


def _repeat(fn, k=4):
    return [fn() for _ in range(k)]


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('reduction', ('mean', 'sum', 'none'))
def test_alternating_order_bit_identical(amd, n, reduction):
    pred, target = _pairs(n, seed=n)
    mod = amd.GDLoss('kld3d', fun='log1p', tau=1.0, reduction=reduction, loss_weight=5.0)
    _same(_repeat(lambda: _call(mod, pred, target)))


@pytest.mark.parametrize('n', (255, 16_385, 1_000_003))
def test_unaligned_rows(amd, n):
    # contiguous (n,7) views that start one float into their buffers: 4-byte aligned only, the guarded path of every tile
    pred, target = _pairs(n, seed=7)
    bp = torch.zeros(n * 7 + 4, device='cuda')
    bt = torch.zeros(n * 7 + 4, device='cuda')
    bp[1:1 + n * 7] = pred.reshape(-1)
    bt[1:1 + n * 7] = target.reshape(-1)
    up, ut = bp[1:1 + n * 7].view(n, 7), bt[1:1 + n * 7].view(n, 7)
    for reduction in ('mean', 'none'):
        mod = amd.GDLoss('gwd3d', fun='log1p', tau=1.0, reduction=reduction, loss_weight=2.0)
        _same(_repeat(lambda: _call(mod, up, ut)) + [_call(mod, pred, target)])


@pytest.mark.parametrize('n', (255, 16_384, 1_000_003))
@pytest.mark.parametrize('positives', (True, False))
def test_weight7_select(amd, n, positives):
    pred, target = _pairs(n, seed=3)
    g = torch.Generator().manual_seed(11)
    w = torch.rand(n, 7, generator=g)
    if not positives:
        w = -w
    w = w.cuda()
    for reduction in ('mean', 'sum'):
        mod = amd.GDLoss('bd3d', fun='log1p', tau=1.0, reduction=reduction, loss_weight=1.0)
        _same(_repeat(lambda: _call(mod, pred, target, weight=w)))


@pytest.mark.parametrize('n', (255, 16_385, 1_000_003))
def test_target_requires_grad(amd, n):
    pred, target = _pairs(n, seed=5)
    for reduction in ('mean', 'none'):
        mod = amd.GDLoss('gwd3d', fun='log1p', tau=1.0, reduction=reduction, loss_weight=5.0)
        _same(_repeat(lambda: _call(mod, pred, target, grad_target=True)))


@pytest.mark.parametrize('n', (255, 16_385, 1_000_003))
def test_prologues(amd, n):
    from mmdet3d_gaussian_amd._lib import prologue as _prologue
    g = torch.Generator().manual_seed(13)
    enc_p = (torch.randn(n, 7, generator=g) * 0.2).cuda()
    enc_t = (torch.randn(n, 7, generator=g) * 0.2).cuda()
    anchors = torch.cat([torch.rand(n, 3, generator=g) * 40, torch.rand(n, 3, generator=g) * 2 + 0.5,
                         torch.rand(n, 1, generator=g) * 3], 1).cuda()
    locs = (torch.rand(n, 2, generator=g) * 100).floor().cuda()
    w = torch.rand(n, 7, generator=g).cuda()
    mod = amd.GDLoss('kld3d', fun='log1p', tau=1.0, reduction='mean', loss_weight=2.0)
    pro_a = _prologue(1, anchors)
    _same(_repeat(lambda: _call(mod, enc_p, enc_t, weight=w, avg_factor=float(n), _prologue=pro_a)))
    pro_c = _prologue(2, locs, types.SimpleNamespace(norm_bbox=True, out_size_factor=4.0, voxel_size=(0.1, 0.1), pc_range=(-51.2, -51.2)))
    dims = enc_t.clone()
    dims[:, 3:6] = dims[:, 3:6].exp()
    _same(_repeat(lambda: _call(mod, enc_p, dims, avg_factor=float(n), _prologue=pro_c)))


@pytest.mark.parametrize('n', (16_384, 1_000_003))
def test_two_targets_interleaved(amd, n):
    """A, B, A, B: every launch follows one on the other target and ascends; A, A, B, B: each second launch descends.
    Either way each target's outputs are the same in every call."""
    pa, ta = _pairs(n, seed=21)
    pb, tb = _pairs(n, seed=22)
    mod = amd.GDLoss('bd3d', fun='log1p', tau=1.0, reduction='mean', loss_weight=5.0)
    ra, rb = [], []
    for order in ('abab', 'aabb'):
        for c in order:
            (ra if c == 'a' else rb).append(_call(mod, pa if c == 'a' else pb, ta if c == 'a' else tb))
    _same(ra)
    _same(rb)


# ------------------------------------------------------------------------------------------------------------------------------
# Against the reference.  The tests above hold the tile order to itself; these hold every reuse launch (reversed, uncapped,
# target read with the default cache policy) to the fp64 oracle and to the same call on a fresh target buffer, which ascends
# and keeps the occupancy cap.
MIX = (('gwd3d', dict(fun='log1p', tau=1.0)), ('kld3d', dict(fun='log1p', tau=1.0)), ('bd3d', dict(fun='log1p', tau=1.0)),
       ('jd3d', dict(fun='log1p', tau=1.0)), ('kld3d_symmax', dict(fun='log1p', tau=1.0)),
       ('kld3d_symmin', dict(fun='log1p', tau=1.0)), ('kfiou3d', dict(fun='nlog')))


def _mods(amd, n, losses=MIX):
    # loss_weight n with reduction 'mean': scale 1, so the gradients are the per-pair gradients the bounds are stated for
    return [amd.GDLoss(lt, reduction='mean', loss_weight=float(n), **kw) for lt, kw in losses]


def _dev_call(mod, pred, target, grad_target=False):
    """One forward + backward on the target tensor ITSELF (same pointer every call); outputs stay on the device."""
    p = pred.detach().clone().requires_grad_(True)
    if grad_target:
        target.grad = None
    out = mod(p, target)
    out.backward()
    res = [out.detach().reshape(1), p.grad]
    if grad_target:
        res.append(target.grad)
    return res


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _fresh(target, grad_target):
    return target.detach().clone().requires_grad_(grad_target)


def _check_oracle(name, results, pred, target, lt, kw):
    """each of `results` (outputs of _dev_call at scale 1) within the product's bounds of the fp64 oracle"""
    import oracle
    from gd_golden import check_close, grad_bound
    ref = oracle.gd_loss(pred.cpu().numpy(), target.detach().cpu().numpy(), oracle.make_params(lt, **kw), scale=1.0, nthreads=16)
    bp, bt = grad_bound(ref['grad_pred']), grad_bound(ref['grad_target'])
    for res in results:
        val = res[0].item()
        assert abs(val - ref['loss_sum']) <= 1e-5 * (1 + abs(ref['loss_sum'])), (name, val, ref['loss_sum'])
        check_close(name + '.gp', res[1].cpu().numpy(), ref['grad_pred'], bp)
        if len(res) > 2:
            check_close(name + '.gt', res[2].cpu().numpy(), ref['grad_target'], bt)


@pytest.mark.parametrize('n', (16_384, 16_385, 1_000_003))
def test_mixed_loss_sequence_on_one_target_vs_oracle(amd, n):
    """The bench step's pattern: different loss types back to back on one target.  All seven loss types run twice on one
    target (14 launches: after the first, every launch is a reuse launch and the direction alternates, so each loss runs in
    both directions), with and without the target gradient.  Every output is bit-equal to the same call on a fresh target
    buffer, and those are within the oracle bounds."""
    pred, target = _pairs(n, seed=31)
    mods = _mods(amd, n)
    fresh = {}
    for grad_target in (False, True):
        keep = [_fresh(target, grad_target) for _ in mods]        # distinct live buffers: every fresh call ascends, capped
        fresh[grad_target] = [_dev_call(m, pred, t, grad_target) for m, t in zip(mods, keep)]
        T = _fresh(target, grad_target)
        for rnd in range(2):
            for k, m in enumerate(mods):
                got = _dev_call(m, pred, T, grad_target)
                assert all(_bits(a, b) for a, b in zip(got, fresh[grad_target][k])), (MIX[k][0], rnd, grad_target)
        del keep, T
    for k, (lt, kw) in enumerate(MIX):
        _check_oracle(f'{lt}.{n}', (fresh[False][k], fresh[True][k]), pred, target, lt, kw)


@pytest.mark.parametrize('how', ('device_copy', 'pinned_non_blocking', 'side_stream'))
def test_target_rewritten_in_place_is_read_anew(amd, how):
    """Same pointer, same n, new values between two launches: the next launch (a reuse launch) follows the new values."""
    n = 1_000_003
    pred, target = _pairs(n, seed=41)
    _, target2 = _pairs(n, seed=42)
    lt, kw = MIX[1]
    mod = _mods(amd, n, [MIX[1]])[0]
    T = target.clone()
    first = _dev_call(mod, pred, T)
    _dev_call(mod, pred, T)
    cur = torch.cuda.current_stream()
    host = None
    if how == 'device_copy':
        T.copy_(target2)
    elif how == 'pinned_non_blocking':
        host = target2.cpu().pin_memory()
        T.copy_(host, non_blocking=True)
    else:
        side = torch.cuda.Stream()
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            T.copy_(target2)
        cur.wait_stream(side)
    got = _dev_call(mod, pred, T)
    want = _dev_call(mod, pred, target2.clone())
    torch.cuda.synchronize()
    assert all(_bits(a, b) for a, b in zip(got, want)), how
    assert not _bits(got[0], first[0])
    _check_oracle(f'{lt}.{how}', [want], pred, target2, lt, kw)


@pytest.mark.parametrize('losses', ('bench_step', 'five'))
@pytest.mark.parametrize('n', (16_384, 65_537))
def test_graph_replay_vs_eager_on_fresh_buffers(amd, n, losses):
    """The bench step (gwd3d, kld3d, bd3d on one target, one plain `(l0 + l1 + l2).backward()`) and a five-loss step, both an
    odd number of launches on one target, captured once on static buffers.  Refilled from the host, replayed twice back to
    back: every replay is bit-equal to eager calls on fresh buffers holding the same values."""
    sel = MIX[:3] if losses == 'bench_step' else (MIX[0], MIX[1], MIX[2], MIX[3], MIX[6])
    mods = _mods(amd, n, sel)
    k = len(sel)
    sp = [_pairs(n, seed=51 + j)[0].requires_grad_(True) for j in range(k)]
    st = _pairs(n, seed=50)[1]

    def step():
        for x in sp:
            x.grad = None
        ls = [m(x, st) for m, x in zip(mods, sp)]
        sum(ls[1:], ls[0]).backward()
        return [x.detach() for x in ls], [x.grad for x in sp]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_ls, g_gs = step()
    for it in range(2):
        hp = [_pairs(n, seed=60 + 10 * it + j)[0].cpu() for j in range(k)]
        ht = _pairs(n, seed=59 + 10 * it)[1].cpu()
        with torch.no_grad():
            for x, h in zip(sp, hp):
                x.copy_(h)
            st.copy_(ht)
        reps = []
        for _ in range(2):
            graph.replay()
            reps.append(([x.clone() for x in g_ls], [g.clone() for g in g_gs]))
        torch.cuda.synchronize()
        keep = [ht.cuda() for _ in range(k)]
        eager = [_dev_call(m, h.cuda(), t) for m, h, t in zip(mods, hp, keep)]
        for r_ls, r_gs in reps:
            for j in range(k):
                assert _bits(r_ls[j].reshape(1), eager[j][0]) and _bits(r_gs[j], eager[j][1]), (losses, it, sel[j][0])
    lt, kw = sel[0]
    _check_oracle(f'{losses}.{lt}', [eager[0]], hp[0], ht, lt, kw)


@pytest.mark.parametrize('weight', ('none', 'w7'))
def test_c_abi_tile_partials_identical_in_both_orders_and_vs_oracle(amd, weight):
    """include/gd3d.h: the fp32 per-tile partials gd3d_loss_fused leaves at the start of the workspace are bit-identical in
    either tile order, and agree with fp64 per-tile sums of the oracle's per-row losses within the loss bound."""
    import ctypes
    import oracle
    from gd_golden import check_close, loss_bound
    from mmdet3d_gaussian_amd import gd_loss
    lib = amd.load_library()
    n = 100_003
    nb = (n + 255) // 256
    pred, target = _pairs(n, seed=61)
    g = torch.Generator().manual_seed(62)
    w7 = torch.rand(n, 7, generator=g).cuda() if weight == 'w7' else None
    prm = gd_loss.make_params('bd3d', 'log1p', 1.0, 1.0, (0, 0, 0.5), {})
    ws = torch.empty(lib.gd3d_loss_workspace_bytes(n) // 4, device='cuda')
    loss_sum = torch.empty(1, device='cuda')
    gp = torch.empty_like(pred)
    stream = torch.cuda.current_stream().cuda_stream
    parts = []
    for _ in range(2):           # same target, same n: the second launch walks the tiles in the other direction
        ws.fill_(float('nan'))
        if w7 is None:
            rc = lib.gd3d_loss_fused(ctypes.byref(prm), pred.data_ptr(), target.data_ptr(), None, n, 1.0, None,
                                     loss_sum.data_ptr(), gp.data_ptr(), None, ws.data_ptr(), stream)
        else:
            rc = lib.gd3d_loss_fused_w7(ctypes.byref(prm), pred.data_ptr(), target.data_ptr(), None, w7.data_ptr(), n, 1.0,
                                        None, loss_sum.data_ptr(), gp.data_ptr(), None, ws.data_ptr(), stream)
        assert rc == 0
        torch.cuda.synchronize()
        parts.append(ws[:nb].cpu().numpy())
    assert np.array_equal(parts[0].view(np.uint32), parts[1].view(np.uint32))
    rw = None if w7 is None else w7.cpu().numpy().astype(np.float64).mean(-1)
    ref = oracle.gd_loss(pred.cpu().numpy(), target.cpu().numpy(), oracle.make_params('bd3d', fun='log1p', tau=1.0),
                         row_weight=rw, scale=1.0, nthreads=16)
    tiles = np.add.reduceat(ref['loss'], np.arange(0, n, 256))
    check_close(f'partials.{weight}', parts[0], tiles, loss_bound(tiles))


def test_c_abi_select_partials_identical_in_both_orders_and_vs_oracle(amd):
    """gd3d_loss_fused_select's three partial arrays (loss | sum(pred * weight7) | some weight > 0), tiles with and without a
    positive weight: bit-identical in either order, and equal to fp64 per-tile sums within the loss bound."""
    import ctypes
    import oracle
    from gd_golden import check_close, loss_bound
    from mmdet3d_gaussian_amd import gd_loss
    lib = amd.load_library()
    n = 100_003
    nb = (n + 255) // 256
    nbp = (nb + 3) & ~3
    pred, target = _pairs(n, seed=63)
    g = torch.Generator().manual_seed(64)
    w = torch.rand(n, 7, generator=g)
    tile = torch.arange(n) // 256
    w[tile % 3 == 0] *= -1                                         # every third tile has no weight > 0
    w7 = w.cuda()
    prm = gd_loss.make_params('kld3d', 'log1p', 1.0, 1.0, (0, 0, 0.5), {})
    ws = torch.empty(lib.gd3d_loss_workspace_bytes(n) // 4, device='cuda')
    loss_sum = torch.empty(1, device='cuda')
    anyp = torch.empty(1, dtype=torch.int32, device='cuda')
    gp = torch.empty_like(pred)
    stream = torch.cuda.current_stream().cuda_stream
    parts = []
    for _ in range(2):
        ws.fill_(float('nan'))
        rc = lib.gd3d_loss_fused_select(ctypes.byref(prm), None, pred.data_ptr(), target.data_ptr(), w7.data_ptr(), n, 1.0,
                                        loss_sum.data_ptr(), anyp.data_ptr(), gp.data_ptr(), None, ws.data_ptr(), stream,
                                        None, None)
        assert rc == 0
        torch.cuda.synchronize()
        h = ws.cpu().numpy()
        parts.append([h[k * nbp:k * nbp + nb] for k in range(3)])
    for a, b in zip(*parts):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    wn = w.numpy().astype(np.float64)
    ref = oracle.gd_loss(pred.cpu().numpy(), target.cpu().numpy(), oracle.make_params('kld3d', fun='log1p', tau=1.0),
                         row_weight=wn.mean(-1), scale=1.0, nthreads=16)
    starts = np.arange(0, n, 256)
    want = [np.add.reduceat(ref['loss'], starts), np.add.reduceat((pred.cpu().numpy().astype(np.float64) * wn).sum(-1), starts),
            np.maximum.reduceat((wn > 0).any(-1).astype(np.float64), starts)]
    for k, name in enumerate(('loss', 'pred_w')):
        check_close(f'select.{name}', parts[0][k], want[k], loss_bound(want[k]))
    # the third array counts the tile's waves that saw a weight > 0: the contract is "> 0 iff some weight of the tile is > 0"
    assert np.array_equal(parts[0][2] > 0, want[2] > 0) and ((parts[0][2] >= 0) & (parts[0][2] <= 4)).all()
    assert anyp.item() == 1
