"""The fused loss launch walks its tiles in either order: a launch on the same target and row count as the previous fused
launch of its stream runs opposite to it (so that it starts on the target rows still in the Infinity Cache), any other
launch ascends.  The order must change nothing: repeated calls on one target, which alternate direction, return
bit-identical losses and gradients, on every path of the kernel (partial last tile, unaligned rows, (N,7) weights with and
without positives, target gradient, bbox-coder prologues, single-launch finish and two-stage reduce)."""
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
    from mmdet3d_gaussian_amd.head_loss import _prologue
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
    pro_c = _prologue(2, locs, norm_bbox=True, out_size_factor=4.0, voxel_size=(0.1, 0.1), pc_range=(-51.2, -51.2))
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
