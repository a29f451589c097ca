"""CenterPoint target assignment on the MI355X (csrc/center_targets.hip, center_targets.py) against the CPU restatement of
gd_centerpoint_head.py:65-156 with mmdet3d's Gaussian helpers (oracle/center_targets_torch.py; third-party parts unpinned).
Positions, boxes and their order bit for bit; heat maps bit for bit (the window is evaluated in fp64 and rounded once, as numpy
does — a device exp that differed by an fp64 ulp exactly at an fp32 rounding boundary would show as one ulp: not seen)."""
import functools

import numpy as np
import pytest
import torch

import mmdet3d_gaussian_amd as amd
from oracle import center_targets_torch as ct

pytestmark = pytest.mark.extras   # frozen extras outside SURVEY.md §8: `pytest -m extras` on a GPU box (conftest.py), not part of `-m gpu`
NUS = dict(grid_size=[512, 512, 1], point_cloud_range=[-51.2, -51.2, -5.0, 51.2, 51.2, 3.0], voxel_size=[0.2, 0.2, 8],
           out_size_factor=4, gaussian_overlap=0.1, min_radius=2)
TASKS = [['car'], ['truck', 'construction_vehicle'], ['bus', 'trailer'], ['barrier'], ['motorcycle', 'bicycle'],
         ['pedestrian', 'traffic_cone']]


def scene(g, n, spread=58.0, ignore=0.1):
    xy = torch.rand(n, 2, generator=g) * 2 * spread - spread          # some centres fall outside the 51.2 m range
    dims = torch.rand(n, 3, generator=g) * torch.tensor([3.0, 9.0, 3.0]) + torch.tensor([0.3, 0.4, 0.5])
    box = torch.cat([xy, torch.rand(n, 1, generator=g) * 4 - 3, dims, torch.rand(n, 1, generator=g) * 6.28 - 3.14,
                     torch.randn(n, 2, generator=g)], 1)
    lab = torch.randint(0, 10, (n,), generator=g)
    lab[torch.rand(n, generator=g) < ignore] = -1
    return box, lab


def check(boxes, labels, tasks, cfg, objects=False):
    counts = [len(t) for t in tasks]

    class Obj:                       # what the head receives: bottom-centred rows behind `.tensor`
        def __init__(self, t):
            self.tensor = t
    if objects:
        gpu_boxes = [Obj(b.cuda()) for b in boxes]
        grav = [torch.cat([b[:, :2], (b[:, 2] + b[:, 5] * 0.5).unsqueeze(1), b[:, 3:]], 1) for b in boxes]
    else:
        gpu_boxes, grav = [b.cuda() for b in boxes], boxes
    hm, an, pi = amd.extras.center_head_get_targets(gpu_boxes, [l.cuda() for l in labels], tasks, cfg)
    hw, aw, pw = ct.get_targets(grav, labels, counts, cfg)
    assert len(hm) == len(hw) == len(tasks)
    for t in range(len(tasks)):
        assert pi[t].dtype == torch.int64 and torch.equal(pi[t].cpu(), pw[t]), t
        assert torch.equal(an[t].cpu(), aw[t]), t
        assert hm[t].shape == hw[t].shape
        assert torch.equal(hm[t].cpu(), hw[t]), (t, float((hm[t].cpu() - hw[t]).abs().max()))
    return hm, an, pi


def test_targets_nuscenes_geometry():
    g = torch.Generator().manual_seed(31)
    data = [scene(g, n) for n in (140, 3, 260, 75)]
    hm, an, pi = check([d[0] for d in data], [d[1] for d in data], TASKS, NUS)
    assert sum(a.shape[0] for a in an) > 250 and all(float(h.max()) == 1.0 for h in hm)
    check([d[0] for d in data], [d[1] for d in data], TASKS, NUS, objects=True)


def test_targets_edge_cases():
    g = torch.Generator().manual_seed(32)
    b0, l0 = scene(g, 60)
    b0[:5, 3] = 0.0                         # zero width: invalid (:124)
    b0[5:8, 4] = -1.0                       # negative length
    b0[8, 0], b0[8, 1] = -51.3, 10.0        # just left of the range: `.long()` truncates -0.125 to cell 0 -> still valid
    b0[9, 0], b0[9, 1] = 51.19, -51.19      # last / first cell
    b0[10, 0] = 51.2                        # first cell outside
    b0[11:14, :2] = torch.tensor([[-51.0, -51.0], [51.0, 51.0], [0.0, 51.0]])   # Gaussians clipped at corners / an edge
    b0[11:14, 3:5] = torch.tensor([[8.0, 20.0], [10.0, 25.0], [6.0, 14.0]])     # big boxes: radius well above min_radius
    l0[11:14] = torch.tensor([3, 3, 4])
    b0[14:20, :2] = torch.tensor([1.0, 2.0])                                     # six boxes of one class in ONE cell
    l0[14:20] = 0
    b1, l1 = scene(g, 0)                    # a sample without boxes
    b2, l2 = scene(g, 30)
    l2[:] = 9                               # one class only: five tasks get nothing from this sample
    check([b0, b1, b2], [l0, l1, l2], TASKS, NUS)
    # nothing valid at all
    hm, an, pi = check([b1, b1], [l1, l1], TASKS, NUS)
    assert all(a.shape[0] == 0 for a in an) and all(float(h.abs().max()) == 0.0 for h in hm)
    # other geometry: one task of three classes, rectangular... the reference mixes the two map extents only for non-square
    # grids (rows = grid_size[0] // osf); keep it square but change every other setting
    cfg = dict(grid_size=[1440, 1440, 40], point_cloud_range=[-54.0, -54.0, -5.0, 54.0, 54.0, 3.0], voxel_size=[0.075, 0.075, 0.2],
               out_size_factor=8, gaussian_overlap=0.35, min_radius=1)
    data = [scene(g, n, spread=56.0) for n in (90, 41)]
    for d in data:
        d[1].clamp_(max=2)
    check([d[0] for d in data], [d[1] for d in data], [['a', 'b', 'c']], cfg)
    # the reference's KITTI CenterPoint geometry (configs/_base_/models/pillarmvf_centerpoint_016pillar_second_secfpn_kitti.py):
    # grid_size = [496, 432, 1] -> maps of 248 rows x 216 columns, tasks Pedestrian | Cyclist | Car
    kitti = dict(grid_size=[496, 432, 1], point_cloud_range=[0, -39.68, -3, 69.12, 39.68, 1], voxel_size=[0.16, 0.16, 4],
                 out_size_factor=2, gaussian_overlap=0.1, min_radius=2)
    data = []
    for n in (40, 25):
        b, l = scene(g, n)
        b[:, 0] = torch.rand(n, generator=g) * 75 - 3           # x in [-3, 72): a few outside [0, 69.12)
        b[:, 1] = torch.rand(n, generator=g) * 84 - 42
        data.append((b, l.clamp(min=-1, max=2)))
    hm, an, pi = check([d[0] for d in data], [d[1] for d in data], [['Pedestrian'], ['Cyclist'], ['Car']], kitti)
    assert hm[0].shape == (2, 1, 248, 216) and int(torch.cat(pi)[:, 1].max()) < 216 and int(torch.cat(pi)[:, 2].max()) > 216


def test_targets_feed_the_head_losses():
    """the outputs are what center_head_losses takes: boxes (n, 9) and [batch, x, y] rows on the device"""
    g = torch.Generator().manual_seed(33)
    data = [scene(g, n, spread=50.0, ignore=0.0) for n in (50, 60)]
    hm, an, pi = amd.extras.center_head_get_targets([d[0].cuda() for d in data], [d[1].cuda() for d in data], TASKS, NUS)
    coder = amd.CenterPointBBoxYawCoder(pc_range=[-51.2, -51.2], out_size_factor=4, voxel_size=[0.2, 0.2], norm_bbox=True)
    maps = [{k: (torch.randn(2, c, 128, 128, generator=g) * 0.3).cuda().requires_grad_(True)
             for k, c in (('reg', 2), ('height', 1), ('dim', 3), ('yaw', 1), ('dir', 2), ('vel', 2))} for _ in TASKS]
    out = amd.center_head_losses(amd.GDLoss('bd3d', fun='log1p', tau=0.0, loss_weight=5.0), dict(type='L1Loss', reduction='mean', loss_weight=0.25),
                                 coder, maps, pi, an, [max(a.shape[0], 1) for a in an], [1.0, 1.0, 0.2, 0.2])
    total = sum(a + b for a, b in out)
    total.backward()
    assert torch.isfinite(total) and all(torch.isfinite(m['dim'].grad).all() for m in maps)


def test_targets_errors():
    g = torch.Generator().manual_seed(34)
    b, l = scene(g, 10)
    with pytest.raises(RuntimeError, match='no CPU path'):
        amd.extras.center_head_get_targets([b], [l], TASKS, NUS)
    with pytest.raises(RuntimeError, match='one label each'):
        amd.extras.center_head_get_targets([b.cuda()], [l[:5].cuda()], TASKS, NUS)
    big = scene(g, 9000)
    with pytest.raises(RuntimeError, match='sorts at most'):
        amd.extras.center_head_get_targets([big[0].cuda()], [big[1].cuda()], TASKS, NUS)


def test_targets_random_batches():
    """25 random batches (sample counts, box counts incl. empty samples, task layouts, geometries, overlaps): everything bit for bit"""
    g = torch.Generator().manual_seed(88)
    rng = np.random.default_rng(88)
    for it in range(25):
        B = int(rng.integers(1, 6))
        layout = [['c'] * int(rng.integers(1, 4)) for _ in range(int(rng.integers(1, 7)))]
        ncls = sum(len(t) for t in layout)
        osf = int(rng.choice([1, 2, 4, 8]))
        vs = float(rng.choice([0.1, 0.16, 0.2, 0.32]))
        nx, ny = int(rng.integers(4, 40)) * osf * 4, int(rng.integers(4, 40)) * osf * 4
        cfg = dict(grid_size=[ny, nx, 1], point_cloud_range=[-nx * vs / 2, -ny * vs / 3, -5.0, nx * vs / 2, ny * vs * 2 / 3, 3.0],
                   voxel_size=[vs, vs, 8], out_size_factor=osf, gaussian_overlap=float(rng.choice([0.1, 0.3, 0.5])),
                   min_radius=int(rng.integers(0, 4)))
        boxes, labels = [], []
        for b in range(B):
            n = int(rng.integers(0, 120))
            bx, _ = scene(g, n)
            bx[:, 0] = (torch.rand(n, generator=g) * 1.2 - 0.1) * nx * vs - nx * vs / 2
            bx[:, 1] = (torch.rand(n, generator=g) * 1.2 - 0.1) * ny * vs - ny * vs / 3
            boxes.append(bx)
            labels.append(torch.randint(-1, ncls + 1, (n,), generator=g))     # -1 and ncls belong to no task
        check(boxes, labels, layout, cfg, objects=bool(it % 2))


# ---------------------------------------------------------------------------------------------------------------------------
# Past one pass of the 1024-thread sort.  assign_kernel sorts P = pow2 >= total keys in LDS: above 1024 boxes the key loop, the
# compare-exchange chunks (lds_sort.h, `t += T`) and, above 1024 VALID boxes, the output loops stride.
def split(total, fractions):
    """sample sizes: uneven, one sample empty"""
    sizes = [int(total * f) for f in fractions]
    sizes[-1] = total - sum(sizes[:-1])
    assert sum(sizes) == total and 0 in sizes and len(set(sizes)) == len(sizes)
    return sizes


SPLITS = {1024: (0.25, 0.0, 0.75), 1025: (0.0, 0.7, 0.3), 2048: (0.3, 0.6, 0.0, 0.1), 2049: (0.45, 0.0, 0.55),
          4096: (0.6, 0.0, 0.3, 0.1), 4097: (0.2, 0.0, 0.8), 8192: (0.4, 0.0, 0.35, 0.25)}


@functools.lru_cache(maxsize=None)
def big_batch(total):
    """`scene()` boxes at nuScenes geometry: labels include -1 and about a fifth of the centres lie outside the range, so valid
    boxes and sunk keys interleave in the list that is sorted"""
    g = torch.Generator().manual_seed(9000 + total)
    data = [scene(g, n) for n in split(total, SPLITS[total])]
    return [d[0] for d in data], [d[1] for d in data]


@pytest.mark.parametrize('total', sorted(SPLITS))
def test_targets_past_one_sort_pass(total):
    """P = 1024 (the last single pass), 2048, 4096, 8192.  total = 8192 needs 73 792 bytes of dynamic LDS: the
    hipFuncSetAttribute opt-in branch of center_targets_build; it runs twice in this process (the second call skips the
    attribute set) with equal results."""
    boxes, labels = big_batch(total)
    hm, an, pi = check(boxes, labels, TASKS, NUS)
    nvalid = sum(a.shape[0] for a in an)
    if total >= 2048:
        assert nvalid > 1024          # the output loops stride too
    elif total == 1025:
        assert total > 1024 > nvalid  # the key loop and the sort stride, the output loops do not
    else:
        assert total == 1024          # exactly one key per thread
    if total == 8192:
        hm2, an2, pi2 = amd.extras.center_head_get_targets([b.cuda() for b in boxes], [l.cuda() for l in labels], TASKS, NUS)
        for t in range(len(TASKS)):
            assert torch.equal(hm2[t], hm[t]) and torch.equal(an2[t], an[t]) and torch.equal(pi2[t], pi[t])


def test_targets_keep_input_order_inside_a_class():
    """1500 boxes of one class in one sample on 100 distinct centres (15 per cell): the sort key ends in the box index, so anno rows
    come out in input order — the marker column says so directly"""
    g = torch.Generator().manual_seed(9100)
    n = 1500
    b, l = scene(g, n, spread=50.0, ignore=0.0)
    centres = torch.rand(100, 2, generator=g) * 90 - 45
    b[:, :2] = centres[torch.randint(0, 100, (n,), generator=g)]
    b[:, 7] = torch.arange(n, dtype=torch.float32)                 # marker
    l[:] = 0
    b2, l2 = scene(g, 40)
    hm, an, pi = check([b, b2], [l, l2], TASKS, NUS)
    first = an[0][:n, 7].cpu()
    assert an[0].shape[0] >= n and torch.equal(first, torch.arange(n, dtype=torch.float32)), first[:20]
    assert int(pi[0][:n, 0].max()) == 0 and len({tuple(r) for r in pi[0][:n].tolist()}) <= 100


def test_targets_at_the_limits_of_the_key_fields():
    """the key (task * B + sample) * 64 + class at 40 tasks, 64 samples and a task of 64 classes (103 classes in all), with boxes
    in the last class of the wide task and in the last task, both in the last sample"""
    g = torch.Generator().manual_seed(9200)
    wide = 20
    layout = [['c'] * (64 if t == wide else 1) for t in range(40)]
    ncls = sum(len(t) for t in layout)
    assert ncls == 103
    cfg = dict(grid_size=[16, 16, 1], point_cloud_range=[-8.0, -8.0, -5.0, 8.0, 8.0, 3.0], voxel_size=[1.0, 1.0, 8], out_size_factor=1,
               gaussian_overlap=0.1, min_radius=1)
    boxes, labels = [], []
    for s in range(64):
        n = 17 + s % 7
        b, _ = scene(g, n, spread=9.0)
        lab = torch.randint(-1, ncls + 1, (n,), generator=g)
        boxes.append(b)
        labels.append(lab)
    boxes[63][:4, :2] = torch.tensor([[0.5, 0.5], [-3.2, 4.1], [7.9, -7.9], [2.0, 2.0]])
    labels[63][:4] = torch.tensor([wide + 63, wide + 63, ncls - 1, wide])
    boxes[0][:2, :2] = torch.tensor([[1.5, -2.5], [-6.0, 6.0]])
    labels[0][:2] = torch.tensor([0, ncls - 1])
    hm, an, pi = check(boxes, labels, layout, cfg)
    assert sum(b.shape[0] for b in boxes) > 1024
    assert hm[wide].shape == (64, 64, 16, 16) and float(hm[wide][63, 63].max()) == 1.0 and float(hm[39][63, 0].max()) == 1.0
    assert int(pi[wide][-1, 0]) == 63 and int(pi[39][-1, 0]) == 63 and int(pi[0][0, 0]) == 0


def test_targets_window_larger_than_the_map():
    """a box whose Gaussian radius exceeds both extents of a 24 x 20 map: the window is the whole map (480 cells, two passes of
    draw_kernel's 256 threads), clipped on all four sides; one box in a corner cell"""
    cfg = dict(grid_size=[24, 20, 1], point_cloud_range=[0.0, 0.0, -5.0, 20.0, 24.0, 3.0], voxel_size=[1.0, 1.0, 8], out_size_factor=1,
               gaussian_overlap=0.1, min_radius=2)
    b = torch.zeros(3, 9)
    b[:, 2:7] = torch.tensor([0.0, 1.0, 1.0, 1.5, 0.3])
    b[0, :2], b[0, 3:5] = torch.tensor([10.5, 12.5]), torch.tensor([70.0, 70.0])        # radius ~0.43 * 70 = 30 cells
    b[1, :2], b[1, 3:5] = torch.tensor([19.5, 23.5]), torch.tensor([9.0, 12.0])         # last cell of the last row
    b[2, :2], b[2, 3:5] = torch.tensor([0.2, 0.3]), torch.tensor([70.0, 60.0])          # first cell, radius past the far corner
    lab = torch.tensor([0, 0, 1])
    hm, an, pi = check([b], [lab], [['a', 'b']], cfg)
    assert hm[0].shape == (1, 2, 24, 20) and pi[0].tolist() == [[0, 10, 12], [0, 19, 23], [0, 0, 0]]
    assert float(hm[0][0, 0].min()) > 0.0 and float(hm[0][0, 1].min()) > 0.0       # both windows reach every cell of their plane
    assert float(hm[0][0, 0, 12, 10]) == 1.0 and float(hm[0][0, 0, 23, 19]) == 1.0 and float(hm[0][0, 1, 0, 0]) == 1.0


@functools.lru_cache(maxsize=None)
def small_batch():
    g = torch.Generator().manual_seed(9300)
    data = [scene(g, n) for n in (130, 0, 170)]
    return [d[0] for d in data], [d[1] for d in data]


@pytest.mark.parametrize('total', (300, 2049))
def test_padded_form_equals_the_plain_form(total):
    """padded=True (task_start stays on the device) against the lists of the plain form"""
    boxes, labels = small_batch() if total == 300 else big_batch(total)
    assert sum(b.shape[0] for b in boxes) == total
    gb, gl = [b.cuda() for b in boxes], [l.cuda() for l in labels]
    hm, an, pi = amd.extras.center_head_get_targets(gb, gl, TASKS, NUS)
    hp, ap, pp, start = amd.extras.center_head_get_targets(gb, gl, TASKS, NUS, padded=True)
    assert start.dtype == torch.int64 and start.is_cuda and ap.shape == (total, 9) and pp.shape == (total, 3) and pp.dtype == torch.int64
    counts = [a.shape[0] for a in an]
    assert start.tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
    end = int(start[-1])
    assert 0 < end < total
    assert torch.equal(ap[:end], torch.cat(an)) and torch.equal(pp[:end], torch.cat(pi))
    assert len(hp) == len(hm) and all(torch.equal(a, b) for a, b in zip(hp, hm))


def test_padded_targets_feed_the_device_resident_head_losses():
    """the chain at a multi-pass size (2049 boxes): center_head_get_targets(padded=True) -> center_head_losses(rows=task_start,
    num_pos = a device tensor) against plain targets -> host-form losses: equal losses and gradients, bit for bit"""
    boxes, labels = big_batch(2049)
    gb, gl = [b.cuda() for b in boxes], [l.cuda() for l in labels]
    B = len(boxes)
    coder = amd.CenterPointBBoxYawCoder(pc_range=[-51.2, -51.2], out_size_factor=4, voxel_size=[0.2, 0.2], norm_bbox=True)
    mod = amd.GDLoss('bd3d', fun='log1p', tau=0.0, loss_weight=5.0)
    l1 = dict(type='L1Loss', reduction='mean', loss_weight=0.25)
    cw = [1.0, 1.0, 0.2, 0.2]

    def maps():
        g = torch.Generator().manual_seed(9400)
        return [{k: (torch.randn(B, c, 128, 128, generator=g) * 0.3).cuda().requires_grad_(True)
                 for k, c in (('reg', 2), ('height', 1), ('dim', 3), ('yaw', 1), ('dir', 2), ('vel', 2))} for _ in TASKS]
    up = [(1.0, 1.0), (0.5, 3.0)] * 3
    _, an, pi = amd.extras.center_head_get_targets(gb, gl, TASKS, NUS)
    host = maps()
    out_h = amd.center_head_losses(mod, l1, coder, host, pi, an, [float(a.shape[0]) for a in an], cw)
    sum(u[0] * o[0] + u[1] * o[1] for u, o in zip(up, out_h)).backward()
    _, ap, pp, start = amd.extras.center_head_get_targets(gb, gl, TASKS, NUS, padded=True)
    num_pos = (start[1:] - start[:-1]).float()
    dev = maps()
    out_d = amd.center_head_losses(mod, l1, coder, dev, pp, ap, num_pos, cw, rows=start)
    sum(u[0] * o[0] + u[1] * o[1] for u, o in zip(up, out_d)).backward()
    assert max(a.shape[0] for a in an) > 256 and ap.shape[0] == 2049
    for t in range(len(TASKS)):
        assert torch.equal(out_d[t][0], out_h[t][0]) and torch.equal(out_d[t][1], out_h[t][1]), t
        assert float(out_h[t][0].detach()) > 0.0 and bool(torch.isfinite(out_h[t][1]))
        for k in host[t]:
            assert torch.equal(dev[t][k].grad, host[t][k].grad) and float(host[t][k].grad.abs().max()) > 0.0, (t, k)
