"""Every compiled instance of the GD-loss kernels against the fp64 oracles (tests/gd_instances.py lists them).

`head_anchor_kernel` (csrc/gd3d_anchor_head.hip), `head_center_kernel` (csrc/gd3d_center_head.hip) and `fused_kernel`
(csrc/gd3d_loss.hip) are compiled per (loss type, fun, flag) of the table in csrc/gd3d_instances.h, and `fused_kernel` also
per target gradient, with an option-free gwd3d form besides.  Each instance runs here with the
reference defaults and with seeded non-default hyper-parameters (alpha, tau, center_offset reach the head launchers through
their own argument structs), at positive counts on both sides of the 256-thread tile.  References and bounds are the
suite's own:
  * decode-fused rows vs oracle.gd_loss_decoded (fp64): flat 2e-5 (test_gpu_head_loss.test_anchor_decoded_loss_vs_oracle
    says why: the decode's fp32 inputs);
  * head slices vs oracle/head_torch.py in fp64 / fp32: 1e-5 + 3 |r32 - r64|, relative to 1 + |r64|
    (test_gpu_head_loss.test_center_head_losses_all_tasks_one_launch);
  * plain rows vs oracle.gd_loss (fp64): gd_golden.loss_bound / grad_bound."""
import numpy as np
import pytest
import torch

import oracle
from gd_golden import _flat, check_close, grad_bound, loss_bound
from gd_instances import INSTANCES, count, hyper, ident

pytestmark = pytest.mark.gpu
IDS = [ident(x) for x in INSTANCES]
KINDS = ('default', 'drawn')
DW = [1.0, 1.0, 0.5, 1.0, 2.0, 1.0, 1.0]
SL1 = dict(type='SmoothL1Loss', beta=1.0 / 9.0, loss_weight=2.0)
CW = [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.5]


@pytest.fixture(scope='module')
def amd():
    import mmdet3d_gaussian_amd as m
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    m.load_library()
    return m


def _tol_check(name, got, r64, r32):
    """1e-5 + 3 x the reference's own fp32 error, relative to 1 + max |r64| (the head-slice rule of this suite)"""
    got, r64, r32 = (np.asarray(x, np.float64) for x in (got, r64, r32))
    sc = np.abs(r64).max() if r64.size else 0.0
    tol = 1e-5 + 3 * (np.abs(r32 - r64).max() if r64.size else 0.0) / (1 + sc)
    err = np.abs(got - r64).max() if r64.size else 0.0
    assert err <= tol * (1 + sc), (name, err, tol * (1 + sc))


# ------------------------------------------------------------------------------------------------- head_anchor_kernel
def _anchor_inputs(seed, P, B=2, A=2, H=40, W=36, C=3):
    """an NCHW anchor head with exactly P positive anchors (labels in [0, C)); the rest are negatives (C) or ignored (-1)"""
    g = torch.Generator().manual_seed(seed)
    n_per = H * W * A
    M = B * n_per
    assert P <= M
    anchors = torch.rand(n_per, 7, generator=g) * torch.tensor([70, 80, 1, 1.5, 3, 0.5, 1.5]) + \
        torch.tensor([0, -40, -2, .6, .9, 1.4, 0])
    bbox_pred = torch.randn(B, A * 7, H, W, generator=g) * 0.15
    bbox_targets = torch.randn(B, n_per, 7, generator=g) * 0.2
    bbox_weights = torch.rand(B, n_per, 7, generator=g)
    labels = torch.full((M,), C, dtype=torch.int64)
    labels[torch.randperm(M, generator=g)[:M // 4]] = -1
    labels[torch.randperm(M, generator=g)[:P]] = torch.randint(0, C, (P,), generator=g)
    return anchors, bbox_pred, bbox_targets, bbox_weights, labels.reshape(B, n_per), C


def _anchor_oracle(lt, kw, anchors, bbox_pred, bbox_targets, bbox_weights, labels, C, scale):
    nz = ((labels.reshape(-1) >= 0) & (labels.reshape(-1) < C)).numpy()
    pos = np.flatnonzero(nz)
    bp = bbox_pred.permute(0, 2, 3, 1).reshape(-1, 7).numpy()[pos]
    bt = bbox_targets.reshape(-1, 7).numpy()[pos]
    an = anchors.numpy()[pos % anchors.shape[0]]
    w = (bbox_weights.reshape(-1, 7).numpy()[pos].astype(np.float64) * np.array(DW)).mean(-1)
    ref = oracle.gd_loss_decoded(bp, bt, oracle.make_params(lt, **kw), oracle.PRO_ANCHOR_DELTA, an, row_weight=w, scale=scale)
    return nz, ref


def _check_anchor_grad(name, grad, nz, ref):
    gflat = grad.permute(0, 2, 3, 1).reshape(-1, 7).cpu().numpy()
    check_close(name + '.gp', gflat[nz], ref['grad_pred'], _flat(ref['grad_pred'], True, 2e-5))
    assert np.abs(gflat[~nz]).max(initial=0.0) == 0.0, name + ': gradient written outside the positives'


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('i', range(len(INSTANCES)), ids=IDS)
def test_head_anchor_kernel_instance(amd, i, kind):
    """anchor_head_decoded_loss_fused (dense and list forms) vs the fp64 oracle on the gathered rows, and anchor_head_bbox_loss
    (GD + SmoothL1 on the encoded rows) vs head_torch.loss_single_bbox in fp64 / fp32; value and NCHW gradient."""
    from oracle import head_torch
    lt = INSTANCES[i][0]
    kw = hyper(i, kind)
    P = count(i)
    anchors, bbox_pred, bt, bw, labels, C = _anchor_inputs(100 + i, P)
    avg = 37.0
    mod = amd.GDLoss(lt, loss_weight=5.0, **kw)
    bt_d, bw_d, lab_d, an_d = bt.cuda(), bw.cuda(), labels.cuda(), anchors.cuda()
    nz, ref = _anchor_oracle(lt, kw, anchors, bbox_pred, bt, bw, labels, C, 5.0 / avg)
    assert nz.sum() == P
    for dense in (True, False):
        p = bbox_pred.cuda().requires_grad_(True)
        out = amd.anchor_head_decoded_loss_fused(mod, p, bt_d, bw_d, lab_d, an_d, C, avg, DW, dense=dense)
        out.backward()
        name = f'{ident(INSTANCES[i])}.{kind}.dense={dense}'
        assert abs(out.item() - ref['loss_sum']) <= 2e-5 * (1 + abs(ref['loss_sum'])), (name, out.item(), ref['loss_sum'])
        _check_anchor_grad(name, p.grad, nz, ref)

    dense = i % 2 == 0
    p = bbox_pred.cuda().requires_grad_(True)
    out = amd.anchor_head_bbox_loss(mod, SL1, p, bt_d, bw_d, lab_d, an_d, C, avg, code_weight=CW, decode_weight=DW,
                                    diff_rad_by_sin=True, dense=dense)
    out.backward()

    def ref_torch(dtype):
        q = bbox_pred.to(dtype).requires_grad_(True)
        r = head_torch.loss_single_bbox(q, bt.to(dtype), bw.to(dtype), labels, anchors.to(dtype), C, avg,
                                        gd=dict(loss_type=lt, loss_weight=5.0, **kw),
                                        sl1=dict(beta=SL1['beta'], loss_weight=SL1['loss_weight']), code_weight=CW,
                                        decode_weight=DW, diff_rad_by_sin=True)
        r.backward()
        return r.item(), q.grad.numpy()
    l64, g64 = ref_torch(torch.float64)
    l32, g32 = ref_torch(torch.float32)
    name = f'{ident(INSTANCES[i])}.{kind}.sl1'
    _tol_check(name + '.loss', out.item(), l64, l32)
    _tol_check(name + '.grad', p.grad.cpu().numpy(), g64, g32)


@pytest.mark.parametrize('i', [0, 21, 24], ids=[IDS[k] for k in (0, 21, 24)])
def test_head_anchor_kernel_more_partials_than_reduce_threads(amd, i):
    """one list-form call with more than 1024 x 256 positives: reduce_partials_kernel adds several partials per thread"""
    lt = INSTANCES[i][0]
    kw = hyper(i, 'drawn')
    P = 1024 * 256 + 1000
    anchors, bbox_pred, bt, bw, labels, C = _anchor_inputs(300 + i, P, B=1, A=2, H=380, W=350)
    avg = 1000.0
    nz, ref = _anchor_oracle(lt, kw, anchors, bbox_pred, bt, bw, labels, C, 5.0 / avg)
    mod = amd.GDLoss(lt, loss_weight=5.0, **kw)
    p = bbox_pred.cuda().requires_grad_(True)
    out = amd.anchor_head_decoded_loss_fused(mod, p, bt.cuda(), bw.cuda(), labels.cuda(), anchors.cuda(), C, avg, DW, dense=False)
    out.backward()
    assert abs(out.item() - ref['loss_sum']) <= 2e-5 * (1 + abs(ref['loss_sum'])), (out.item(), ref['loss_sum'])
    _check_anchor_grad(ident(INSTANCES[i]), p.grad, nz, ref)


# ------------------------------------------------------------------------------------------------- head_center_kernel
def _center_tasks(seed, ns, vel, B=2, H=48, W=40):
    g = torch.Generator().manual_seed(seed)
    tasks = []
    for n in ns:
        d = {'reg': torch.rand(B, 2, H, W, generator=g), 'height': torch.randn(B, 1, H, W, generator=g) * 0.5,
             'dim': torch.randn(B, 3, H, W, generator=g) * 0.3, 'yaw': torch.randn(B, 1, H, W, generator=g),
             'dir': torch.randn(B, 2, H, W, generator=g)}
        if vel:
            d['vel'] = torch.randn(B, 2, H, W, generator=g)
        pi = torch.stack([torch.randint(0, B, (n,), generator=g), torch.randint(0, W, (n,), generator=g),
                          torch.randint(0, H, (n,), generator=g)], -1)
        if n > 10:
            pi[5] = pi[2]
            pi[7] = pi[2]                                   # three objects in one cell (and more at random when n is large)
        cx = (pi[:, 1].float() + 0.5) * 0.8 - 51.2
        cy = (pi[:, 2].float() + 0.5) * 0.8 - 51.2
        an = torch.stack([cx + torch.randn(n, generator=g) * 0.2, cy + torch.randn(n, generator=g) * 0.2,
                          torch.randn(n, generator=g), torch.rand(n, generator=g) * 2 + 0.5, torch.rand(n, generator=g) * 4 + 0.5,
                          torch.rand(n, generator=g) + 0.8, (torch.rand(n, generator=g) - 0.5) * 6.28] +
                         ([torch.randn(n, generator=g), torch.randn(n, generator=g)] if vel else []), -1)
        tasks.append((d, pi, an))
    return tasks


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('i', range(len(INSTANCES)), ids=IDS)
def test_head_center_kernel_instance(amd, i, kind):
    """center_head_losses over three tasks (one without positives, duplicate cells, object counts on both sides of 256) vs
    head_torch.center_head_task_losses in fp64 / fp32: both losses of every task and the gradient of every head map."""
    from oracle import head_torch
    lt = INSTANCES[i][0]
    kw = hyper(i, kind)
    vel = i % 2 == 0
    ns = [count(i), 0, (255, 256, 257)[i % 3]]
    tasks = _center_tasks(200 + i, ns, vel)
    cfg = dict(pc_range=[-51.2, -51.2], out_size_factor=4, voxel_size=[0.2, 0.2], norm_bbox=True)
    coder = amd.CenterPointBBoxYawCoder(pc_range=cfg['pc_range'], out_size_factor=4, voxel_size=cfg['voxel_size'], norm_bbox=True)
    cw = [1.0, 1.0, 0.2, 0.2] if vel else [1.0, 0.5]
    up = [(1.0, 1.0), (1.0, 1.0), (0.5, 3.0)]
    mod = amd.GDLoss(lt, loss_weight=5.0, **kw)
    dev_tasks = [{k: v.cuda().requires_grad_(True) for k, v in d.items()} for d, _, _ in tasks]
    out = amd.center_head_losses(mod, dict(type='L1Loss', reduction='mean', loss_weight=0.25), coder, dev_tasks,
                                 [pi.cuda() for _, pi, _ in tasks], [an.cuda() for _, _, an in tasks], ns, cw)
    sum(u[0] * o[0] + u[1] * o[1] for u, o in zip(up, out)).backward()

    def ref(dtype):
        res, grads = [], []
        for (d, pi, an), n, u in zip(tasks, ns, up):
            dd = {k: v.to(dtype).requires_grad_(True) for k, v in d.items()}
            l1, gd = head_torch.center_head_task_losses(dd, pi, an.to(dtype), n, cfg, dict(loss_type=lt, loss_weight=5.0, **kw),
                                                        0.25, cw)
            tot = u[0] * l1.sum() + u[1] * gd.sum()
            if tot.requires_grad:
                tot.backward()
            res.append((float(l1.sum().detach()), float(gd.sum().detach())))
            grads.append({k: (v.grad.numpy() if v.grad is not None else np.zeros(v.shape)) for k, v in dd.items()})
        return res, grads
    r64, g64 = ref(torch.float64)
    r32, g32 = ref(torch.float32)
    name = f'{ident(INSTANCES[i])}.{kind}'
    for t in range(len(ns)):
        for j in range(2):
            _tol_check(f'{name}.task{t}.loss{j}', out[t][j].item(), r64[t][j], r32[t][j])
        for k, v in dev_tasks[t].items():
            got = v.grad.cpu().numpy() if v.grad is not None else np.zeros(v.shape)
            _tol_check(f'{name}.task{t}.{k}', got, g64[t][k], g32[t][k])
    assert out[1][0].item() == 0.0 and out[1][1].item() == 0.0


# ------------------------------------------------------------------------------------------------- fused_kernel
def _rows(seed, n):
    """tests/test_param_sweep.py's `_case` rows at n pairs"""
    rng = np.random.default_rng(seed)
    t = np.stack([rng.uniform(-50, 50, n), rng.uniform(-50, 50, n), rng.uniform(-3, 1, n), rng.uniform(.3, 6, n),
                  rng.uniform(.3, 12, n), rng.uniform(.3, 4, n), rng.uniform(-6, 6, n)], -1)
    p = t + rng.normal(0, 1, (n, 7)) * np.array([.4, .4, .2, .15, .15, .1, .2])
    p[:, 3:6] = np.abs(p[:, 3:6]) + 0.05
    w = rng.uniform(0, 2, n)
    return p.astype(np.float32), t.astype(np.float32), w.astype(np.float32)


N_FAST = 2307      # nine full 256-row tiles on the 16-byte-aligned LDS-DMA path, and a 3-row tail


@pytest.mark.parametrize('i', range(len(INSTANCES)), ids=IDS)
def test_fused_kernel_instance_fast_path(amd, i):
    """per-row loss (forward launch: no gradient outputs), grad_pred and grad_target (backward launches with and without the
    target gradient) with row weights and non-default hyper-parameters, against the fp64 oracle"""
    lt = INSTANCES[i][0]
    kw = hyper(i, 'drawn')
    p, t, w = _rows(400 + i, N_FAST)
    prm = oracle.make_params(lt, **kw)
    ref = oracle.gd_loss(p, t, prm, row_weight=w.astype(np.float64), scale=2.0)
    bl, bp, bt = loss_bound(ref['loss']), grad_bound(ref['grad_pred']), grad_bound(ref['grad_target'])
    if lt == 'kfiou3d':
        # kfiou3d is ill-conditioned in fp32 on thin, long boxes at close angles (w 0.3-0.6 m, l 6-11 m here): the 2x2 determinant
        # of the summed covariances cancels.  On these 2307 rows the `_cpu` twin (the kernel's own math) exceeds the flat 1e-5 on
        # 4 / 1 / 1 rows (nlog / expm1 / none; loss worst 2.1e-5 / 1.8e-5 / 1.2e-5, gradient worst 2.8e-5 / 1.0e-5 / 4.9e-5) and
        # the fp32 oracle, a plain port of the reference's arithmetic, errs as much on the same inputs (loss 2.2e-5 / 8.7e-6 /
        # 3.6e-5, gradient 2.3e-5 / 1.5e-5 / 3.0e-5): the rows of the other six losses stay under 4.1e-7.  gd_golden's
        # policy for such inputs applies: 1e-5 + 3 x the fp32 oracle's own worst error on the case.
        from gd_golden import policy_grad_bound, policy_loss_bound
        r32 = oracle.gd_loss(p, t, prm, row_weight=w, scale=2.0, dtype=np.float32)
        bl = policy_loss_bound(ref['loss'], r32['loss'])
        bp = policy_grad_bound(ref['grad_pred'], r32['grad_pred'])
        bt = policy_grad_bound(ref['grad_target'], r32['grad_target'])
    mod = amd.GDLoss(lt, reduction='none', loss_weight=2.0, **kw)
    wd = torch.from_numpy(w).cuda()
    for grad_target in (False, True):
        pp = torch.from_numpy(p).cuda().requires_grad_(True)
        tt = torch.from_numpy(t).cuda().requires_grad_(grad_target)
        out = mod(pp, tt, wd)
        out.sum().backward()
        name = f'{ident(INSTANCES[i])}.gt={grad_target}'
        check_close(name + '.loss', out.detach().cpu().numpy(), ref['loss'], bl)
        check_close(name + '.gp', pp.grad.cpu().numpy(), ref['grad_pred'], bp)
        if grad_target:
            check_close(name + '.gt', tt.grad.cpu().numpy(), ref['grad_target'], bt)


@pytest.mark.parametrize('fun', ('log1p', 'none'))
@pytest.mark.parametrize('normalize', (True, False))
def test_fused_kernel_option_free_gwd3d(amd, fun, normalize):
    """the option-free gwd3d instantiation: reduced 'sum', no weights, no target gradient, past the one-launch size"""
    n = int(amd.load_library().gd3d_one_launch_max_n()) + N_FAST
    p, t, _ = _rows(450 + int(normalize) + 2 * (fun == 'none'), n)
    kw = dict(fun=fun, tau=1.0, alpha=1.0, normalize=normalize)
    ref = oracle.gd_loss(p, t, oracle.make_params('gwd3d', **kw), scale=3.0, want_grad_target=False, nthreads=8)
    pp = torch.from_numpy(p).cuda().requires_grad_(True)
    out = amd.GDLoss('gwd3d', reduction='sum', loss_weight=3.0, **kw)(pp, torch.from_numpy(t).cuda())
    out.backward()
    assert abs(out.item() - ref['loss_sum']) <= 1e-5 * (1 + abs(ref['loss_sum'])), (out.item(), ref['loss_sum'])
    check_close('gwd3d.plain.gp', pp.grad.cpu().numpy(), ref['grad_pred'], grad_bound(ref['grad_pred']))
