"""Several GD losses on one target in one fused launch (gd3d_loss_fused_multi) and the deferral that feeds it.

Kernel, through the C ABI: every loss scalar and gradient bit-equal to the single-loss entry point (gd3d_loss_fused, unchanged
code) on the same inputs, and inside the product's flat gate (gd_golden.py) of the fp64 oracle; guard rows untouched; a
misaligned pred takes the guarded path.  Sizes: one row, one row short of a tile, a tile, one row over, two tiles and a row,
and 64 tiles and a row (past the single-launch form).
Semantics, through GDLoss with the C++ node: queued forwards give values and gradients bit-equal to GD3D_DEFER=0 in every
flush situation the node distinguishes.
"""
import ctypes

import numpy as np
import pytest
import torch

import oracle
from gd_golden import LOSS_TOL, check_close, oracle32_bounds

pytestmark = pytest.mark.gpu

LT = {'gwd3d': 0, 'kld3d': 1, 'bd3d': 2}
SIZES = [1, 255, 256, 257, 513, 16385]
TUPLES = [('gwd3d', 'kld3d', 'bd3d'), ('bd3d', 'gwd3d', 'kld3d'), ('kld3d', 'gwd3d'), ('gwd3d', 'bd3d')]
GUARD = 64          # guard rows on each side of a gradient buffer
SENTINEL = 7.5


def _synthetic(n, seed, npred=3):
    """SURVEY.md §8d recipe (as tests/test_cpu_gd_loss.py), one target and `npred` predictions."""
    g = torch.Generator().manual_seed(seed)
    lo = torch.tensor([0, -40, -3, 0.5, 0.5, 0.5, -np.pi])
    hi = torch.tensor([70, 40, 1, 2.5, 4.5, 2.0, np.pi])
    tgt = torch.rand(n, 7, generator=g) * (hi - lo) + lo
    sig = torch.tensor([0.3, 0.3, 0.1, 0.1, 0.1, 0.1, 0.1])
    preds = [(tgt + torch.randn(n, 7, generator=g) * sig).float().contiguous() for _ in range(npred)]
    return preds, tgt.float().contiguous()


_inputs, _refs = {}, {}


def _case(n):
    if n not in _inputs:
        _inputs[n] = _synthetic(n, seed=n)
    return _inputs[n]


def _oracle(n, lt, k, scale):
    """fp64 oracle of loss `lt` on prediction k of size n's inputs (computed once, shared)."""
    key = (n, lt, k, scale)
    if key not in _refs:
        preds, tgt = _case(n)
        prm = oracle.make_params(lt, fun='log1p', tau=1.0)
        ref = oracle.gd_loss(preds[k].numpy(), tgt.numpy(), prm, scale=scale)
        _refs[key] = (ref, oracle32_bounds(preds[k].numpy(), tgt.numpy(), prm, ref, scale)[1])
    return _refs[key]


def _lib_and_params():
    import mmdet3d_gaussian_amd as amd
    from mmdet3d_gaussian_amd import _lib
    return amd.load_library(), _lib


def _params(_lib, lt):
    p = _lib.Params()
    p.loss_type, p.fun, p.tau, p.alpha, p.flag = LT[lt], 1, 1.0, 1.0, 1
    p.center_offset = (ctypes.c_float * 3)(0.0, 0.0, 0.5)
    return p


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _single(L, _lib, lt, pred, tgt, n, scale):
    out = torch.zeros(4, device='cuda')
    grad = torch.full((n + 2 * GUARD, 7), SENTINEL, device='cuda')
    ws = torch.empty(L.gd3d_loss_workspace_bytes(n) // 4 + 4, device='cuda')
    rc = L.gd3d_loss_fused(_params(_lib, lt), pred.data_ptr(), tgt.data_ptr(), None, n, scale, None, out.data_ptr(),
                           grad[GUARD:GUARD + n].data_ptr(), None, ws.data_ptr(), _stream())
    assert rc == 0
    return out, grad


def _multi(L, _lib, lts, preds, tgt, n, scales):
    k = len(lts)
    outs = [torch.zeros(4, device='cuda') for _ in lts]
    grads = [torch.full((n + 2 * GUARD, 7), SENTINEL, device='cuda') for _ in lts]
    ws = torch.empty(L.gd3d_loss_fused_multi_workspace_bytes(k, n) // 4 + 4, device='cuda')
    vp = ctypes.c_void_p * k
    rc = L.gd3d_loss_fused_multi(k, (_lib.Params * k)(*[_params(_lib, lt) for lt in lts]), vp(*[p.data_ptr() for p in preds]),
                                 tgt.data_ptr(), n, (ctypes.c_float * k)(*scales), vp(*[o.data_ptr() for o in outs]),
                                 vp(*[g[GUARD:GUARD + n].data_ptr() for g in grads]), ws.data_ptr(), _stream())
    assert rc == 0
    return outs, grads


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize('lts', TUPLES, ids='-'.join)
@pytest.mark.parametrize('n', SIZES)
def test_multi_launch_bit_equal_to_single_launches_and_inside_the_gate(n, lts):
    L, _lib = _lib_and_params()
    preds, tgt = _case(n)
    dp, dt = [p.cuda() for p in preds[:len(lts)]], tgt.cuda()
    scales = [5.0, 3.0, 1.0][:len(lts)]
    outs, grads = _multi(L, _lib, lts, dp, dt, n, scales)
    for k, lt in enumerate(lts):
        o1, g1 = _single(L, _lib, lt, dp[k], dt, n, scales[k])
        torch.cuda.synchronize()
        assert torch.equal(_bits(outs[k]), _bits(o1)), (lt, outs[k][0].item(), o1[0].item())
        assert torch.equal(_bits(grads[k]), _bits(g1)), lt                 # gradient rows AND both guard bands
        band = torch.cat([grads[k][:GUARD], grads[k][GUARD + n:]])
        assert torch.equal(band, torch.full_like(band, SENTINEL)), lt      # ... which nobody wrote
        ref, gb = _oracle(n, lt, k, scales[k])
        assert abs(outs[k][0].item() - ref['loss_sum']) <= LOSS_TOL * (1 + abs(ref['loss_sum']))
        check_close(f'{lt}.{n}.gp', grads[k][GUARD:GUARD + n].cpu().numpy(), ref['grad_pred'], gb)


@pytest.mark.parametrize('n', [257, 16385])
def test_misaligned_pred_takes_the_guarded_path(n):
    L, _lib = _lib_and_params()
    lts = ('gwd3d', 'kld3d', 'bd3d')
    preds, tgt = _case(n)
    dp, dt = [p.cuda() for p in preds], tgt.cuda()
    flat = torch.empty(n * 7 + 1, device='cuda')
    flat[1:].copy_(dp[1].reshape(-1))
    shifted = flat[1:].view(n, 7)
    assert shifted.data_ptr() % 16 == 4
    outs, grads = _multi(L, _lib, lts, [dp[0], shifted, dp[2]], dt, n, [5.0, 3.0, 1.0])
    for k, lt in enumerate(lts):
        o1, g1 = _single(L, _lib, lt, dp[k], dt, n, [5.0, 3.0, 1.0][k])
        torch.cuda.synchronize()
        assert torch.equal(_bits(outs[k]), _bits(o1)) and torch.equal(_bits(grads[k]), _bits(g1)), lt


def test_arguments_the_multi_launch_refuses():
    L, _lib = _lib_and_params()
    n = 257
    preds, tgt = _case(n)
    dp, dt = [p.cuda() for p in preds], tgt.cuda()
    bad = _params(_lib, 'gwd3d')
    bad.fun = 0                                      # an instance the kernel is not compiled for
    assert L.gd3d_loss_fused_multi_eligible(bad) == 0 and L.gd3d_loss_fused_multi_eligible(_params(_lib, 'bd3d')) == 1
    out = torch.zeros(4, device='cuda')
    ws = torch.empty(L.gd3d_loss_workspace_bytes(n) // 4 + 4, device='cuda')
    vp = ctypes.c_void_p * 2
    args = (vp(dp[0].data_ptr(), dp[1].data_ptr()), dt.data_ptr(), 257, (ctypes.c_float * 2)(1.0, 1.0),
            vp(out.data_ptr(), out.data_ptr() + 4), vp(None, None), ws.data_ptr(), _stream())
    assert L.gd3d_loss_fused_multi(2, (_lib.Params * 2)(bad, _params(_lib, 'kld3d')), *args) == 10001
    assert L.gd3d_loss_fused_multi(1, (_lib.Params * 2)(_params(_lib, 'gwd3d'), _params(_lib, 'kld3d')), *args) == 10001
    assert L.gd3d_loss_fused_multi_workspace_bytes(3, 10_000_000) <= L.gd3d_loss_workspace_bytes(10_000_000)


# ---- deferral through GDLoss ------------------------------------------------------------------------------------------------

N_SEM = 16640   # 65 tiles: past gd3d_one_launch_max_n(), whose calls are never queued


@pytest.fixture
def cpp(monkeypatch):
    """The C++ node, the queueing threshold patched down to 257 rows; yields (gd_loss module, stats function)."""
    from mmdet3d_gaussian_amd import _lib, gd_loss
    _lib.set_host_glue('cpp')
    node = _lib.load_node()
    monkeypatch.setattr(gd_loss, 'DEFER_MIN_N', 257)
    monkeypatch.setattr(gd_loss, '_DEFER', True)
    gd_loss.flush()
    yield gd_loss, node.pending_stats
    gd_loss.flush()
    _lib.set_host_glue(None)


def _mods():
    import mmdet3d_gaussian_amd as amd
    return [amd.GDLoss(lt, fun='log1p', tau=1.0, reduction='mean', loss_weight=5.0) for lt in ('gwd3d', 'kld3d', 'bd3d')]


def _leaves(n=N_SEM, npred=3, seed=3):
    preds, tgt = _synthetic(n, seed, npred)
    return [p.cuda().requires_grad_(True) for p in preds], tgt.cuda()


def _eager(gd_loss, fn):
    keep = gd_loss._DEFER
    gd_loss._DEFER = False
    try:
        return fn()
    finally:
        gd_loss._DEFER = keep


def _step():
    ps, t = _leaves()
    ls = [m(p, t) for m, p in zip(_mods(), ps)]
    (ls[0] + ls[1] + ls[2]).backward()
    return [l.detach().clone() for l in ls], [p.grad.clone() for p in ps]


def _same(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def test_three_forwards_leave_in_one_launch_bit_equal_to_eager(cpp):
    gd_loss, stats = cpp
    want_l, want_g = _eager(gd_loss, _step)
    s0 = stats()
    got_l, got_g = _step()
    s1 = stats()
    assert (s1[0] - s0[0], s1[1] - s0[1]) == (1, 0)       # one multi-loss launch, no single one
    assert _same(got_l, want_l) and _same(got_g, want_g)


def test_python_glue_stays_eager_and_bit_equal(cpp):
    gd_loss, stats = cpp
    from mmdet3d_gaussian_amd import _lib
    want_l, want_g = _step()
    _lib.set_host_glue('python')
    s0 = stats()
    got_l, got_g = _step()
    assert stats() == s0
    assert _same(got_l, want_l) and _same(got_g, want_g)


def test_one_forward_alone_takes_the_single_launch(cpp):
    gd_loss, stats = cpp

    def one():
        ps, t = _leaves()
        return _mods()[1](ps[1], t).item()
    want = _eager(gd_loss, one)
    s0 = stats()
    got = one()
    s1 = stats()
    assert (s1[0] - s0[0], s1[1] - s0[1]) == (0, 1) and got == want


def test_two_targets_interleaved(cpp):
    gd_loss, stats = cpp

    def run():
        ps, ta = _leaves(npred=3)
        qs, tb = _leaves(npred=3, seed=4)
        m = _mods()
        ls = [m[0](ps[0], ta), m[1](qs[0], tb), m[2](ps[1], ta), m[0](qs[1], tb)]
        torch.stack(ls).sum().backward()
        return [l.detach().clone() for l in ls], [x.grad.clone() for x in (ps[0], qs[0], ps[1], qs[1])]
    want = _eager(gd_loss, run)
    got = run()
    assert _same(got[0], want[0]) and _same(got[1], want[1])


def test_same_pred_twice(cpp):
    gd_loss, stats = cpp

    def run():
        ps, t = _leaves()
        m = _mods()
        la, lb = m[0](ps[0], t), m[1](ps[0], t)
        (la + lb).backward()
        return [la.detach().clone(), lb.detach().clone()], [ps[0].grad.clone()]
    want = _eager(gd_loss, run)
    s0 = stats()
    got = run()
    s1 = stats()
    assert s1[0] == s0[0] and s1[1] - s0[1] == 2          # the second forward flushed the first: two single launches
    assert _same(got[0], want[0]) and _same(got[1], want[1])


def test_inplace_edit_before_use_raises(cpp):
    gd_loss, stats = cpp
    ps, t = _leaves()
    m = _mods()
    la, lb = m[0](ps[0], t), m[1](ps[1], t)
    with torch.no_grad():
        ps[1].add_(1.0)
    with pytest.raises(RuntimeError, match='modified by an inplace operation'):
        la.item()
    assert torch.isnan(lb).item()                          # never computed on the changed input
    with pytest.raises(RuntimeError):
        lb.backward()
    want = _eager(gd_loss, lambda: m[0](ps[0].detach(), t).item())
    assert la.item() == want                               # the untouched neighbour was evaluated
    assert _same(_step()[0], _eager(gd_loss, _step)[0])    # and nothing stays poisoned


def test_loss_dropped_before_use_launches_nothing(cpp):
    gd_loss, stats = cpp
    ps, t = _leaves()
    s0 = stats()
    loss = _mods()[0](ps[0], t)
    del loss
    gd_loss.flush()
    s1 = stats()
    assert (s1[0] - s0[0], s1[1] - s0[1], s1[2] - s0[2]) == (0, 0, 1)
    assert ps[0].grad is None
    want_l, want_g = _eager(gd_loss, _step)
    got_l, got_g = _step()
    assert _same(got_l, want_l) and _same(got_g, want_g)


def test_forward_under_graph_capture_is_eager_and_replays(cpp):
    gd_loss, stats = cpp
    ps, t = _leaves()
    mod = _mods()[2]
    static = ps[2].detach().clone()
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                mod(static, t).item()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        s0 = stats()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = mod(static, t)
        assert stats() == s0                               # captured as the launches themselves: nothing was queued
        static.copy_(ps[0].detach())
        graph.replay()
        torch.cuda.synchronize()
        got = out.detach().clone()
        want = _eager(gd_loss, lambda: mod(ps[0].detach(), t).detach().clone())
    assert torch.equal(_bits(got), _bits(want))


def test_profile_events_keep_the_launches_single(cpp):
    gd_loss, stats = cpp
    ps, t = _leaves()
    s0 = stats()
    sink = []
    gd_loss.PROFILE_EVENTS = sink
    try:
        ls = [m(p, t) for m, p in zip(_mods(), ps)]
    finally:
        gd_loss.PROFILE_EVENTS = None
    torch.cuda.synchronize()
    assert len(sink) == 3 and all(tm.elapsed_ms() > 0 for tm in sink) and stats() == s0
    want = _eager(gd_loss, lambda: [m(p.detach(), t).detach().clone() for m, p in zip(_mods(), ps)])
    assert _same([l.detach() for l in ls], want)
