"""Seeded inputs of the device-resident centre-head tests (tests/test_center_rows_cases.py, tests/test_gpu_center_head_rows.py)
and their oracle results, computed once per process and never modified.

`center_head_losses(..., rows=...)` reads every task's slice [rows[t], rows[t+1]) of ONE shared pos_inds (N, 3) / anno_boxes (N, C)
pair and divides by max(num_pos[t], 1) on the device (csrc/gd3d_center_head.hip: `center_dyn`, `row = D.row0 + i`).  A case holds
both forms of one problem: the per-task lists (what oracle/head_torch.py and the host form take) and the shared arrays.  Every
shared row outside [rows[0], rows[T]) is POISON — a position outside the head map and NaN box values: the kernel range-checks the
position, so a row read by mistake turns that task's losses into NaN without touching memory.  rows[T] <= N in every case.

Geometry and coder settings are those of test_gpu_head_loss.test_center_head_losses_all_tasks_one_launch; HEAD_T = 256 objects per
workgroup, 64 keys per scan step."""
import functools

import numpy as np
import torch

from oracle import head_torch

B, H, W = 2, 16, 12
HEAD_T, WAVE = 256, 64
CODER = dict(pc_range=[-51.2, -51.2], out_size_factor=4, voxel_size=[0.2, 0.2], norm_bbox=True)
L1_WEIGHT = 0.25
GD = {'gwd3d': dict(loss_type='gwd3d', loss_weight=5.0, fun='log1p', tau=0.0),
      'bd3d': dict(loss_type='bd3d', loss_weight=5.0, fun='log1p', tau=1.0),
      'kld3d': dict(loss_type='kld3d', loss_weight=5.0, fun='none', tau=0.0)}
POISON_POS = (B, W, H)                   # every coordinate one past its extent
HEADS = ('reg', 'height', 'dim', 'yaw', 'dir', 'vel')
CHANNELS = dict(reg=2, height=1, dim=3, yaw=1, dir=2, vel=2)

BLOCK_SIZES = (37, 0, 300, 255, 256, 257, 1, 0)
# `shared`: objects of task 0 that are put into one cell each
TRIPLE, PAIR, CROWD = (2, 5, 7), (10, 300), tuple(range(21, 21 + 8 * 70, 8))
NUMPOS = (0.0, 0.5, 1.0, 37.0, 1000.0)
NUMPOS_ROWS = (3, 10, 5, 20, 300)
NAMES = ('blocks', 'lead', 'shared', 'numpos', 'heads-reg-vel', 'heads-reg-novel7', 'heads-noreg-vel', 'heads-noreg-novel9', 'frozen')
GRAPH_N = 1024


class Case:
    """maps[t]: head name -> (B, c, H, W) fp32;  frozen[t]: names of the maps of task t that take no gradient;
    pos[t] (n, 3) int64 [b, x, y], anno[t] (n, C);  shared_pos (N, 3), shared_anno (N, C), rows (T+1,) int64, num_pos (T,) fp32;
    up[t] = upstream gradient of (loss_l1, loss_gd);  gd: the GDLoss settings as oracle/head_torch.py takes them."""

    def __init__(self, name, maps, pos, anno, lead, tail, gd, num_pos=None, frozen=None, up=None):
        self.name, self.maps, self.pos, self.anno, self.gd = name, maps, pos, anno, dict(gd)
        self.T = len(maps)
        self.vel, self.reg = 'vel' in maps[0], 'reg' in maps[0]
        self.code_weights = [1.0, 1.0, 0.2, 0.2] if self.vel else [1.0, 0.5]
        self.frozen = frozen if frozen is not None else [frozenset()] * self.T
        self.up = up if up is not None else [(1.0, 1.0)] * self.T
        sizes = [p.shape[0] for p in pos]
        self.num_pos = torch.tensor([float(n) for n in sizes] if num_pos is None else num_pos, dtype=torch.float32)
        self.shared_pos, self.shared_anno, self.rows = share(pos, anno, lead, tail)
        self.N = self.shared_pos.shape[0]

    def oracle_anno(self, t):
        """what oracle/head_torch.py takes: its encode() appends every column past the seventh to the L1 target, so a task
        without 'vel' hands it seven columns whatever the width of the stored rows"""
        return self.anno[t][:, :7 + (2 if self.vel else 0)]

    def cells(self, t):
        """bool (B, H, W): the cells named in task t's slice"""
        m = torch.zeros(B, H, W, dtype=torch.bool)
        p = self.pos[t]
        m[p[:, 0], p[:, 2], p[:, 1]] = True
        return m


def share(pos, anno, lead, tail, gap_before=None):
    """per-task lists -> shared (N, 3) / (N, C) arrays with `lead` poison rows in front and `tail` behind, and rows (T+1,).
    gap_before = k inserts ONE more poison row between the data of task k - 1 and task k; rows[k] stays in front of it (so task
    k - 1 is clean and the row is the first of task k's slice) and rows[k+1:] move up by one."""
    cols = anno[0].shape[1]
    sizes = [p.shape[0] for p in pos]
    rows = [lead]
    for n in sizes:
        rows.append(rows[-1] + n)
    parts_p, parts_a = [], []

    def poison(n):
        parts_p.append(torch.tensor([POISON_POS] * n, dtype=torch.int64).reshape(n, 3))
        parts_a.append(torch.full((n, cols), float('nan')))
    poison(lead)
    for t, (p, a) in enumerate(zip(pos, anno)):
        if gap_before == t:
            poison(1)
        parts_p.append(p)
        parts_a.append(a)
    poison(tail)
    rows = torch.tensor(rows, dtype=torch.int64)
    if gap_before is not None:
        rows[gap_before + 1:] += 1
    return torch.cat(parts_p), torch.cat(parts_a), rows


def with_gap(case, k, owner):
    """`case` with one poison row between the data of tasks k - 1 and k: -> (shared_pos, shared_anno, rows, task that reads it).
    rows is a list of contiguous boundaries, so a row between two tasks always belongs to one of them: owner = 'next' leaves
    rows[k] in front of the gap (task k reads it), owner = 'prev' moves rows[k] one row into the gap (task k - 1 reads it).
    Every other task's slice holds exactly its own rows."""
    lead, tail = int(case.rows[0]), case.N - int(case.rows[-1])
    sp, sa, rows = share(case.pos, case.anno, lead, tail, gap_before=k)
    if owner == 'prev':
        rows[k] += 1
        return sp, sa, rows, k - 1
    assert owner == 'next'
    return sp, sa, rows, k


def _maps(g, reg, vel):
    d = {'height': torch.randn(B, 1, H, W, generator=g) * 0.5, 'dim': torch.randn(B, 3, H, W, generator=g) * 0.3,
         'yaw': torch.randn(B, 1, H, W, generator=g), 'dir': torch.randn(B, 2, H, W, generator=g)}
    if reg:
        d['reg'] = torch.rand(B, 2, H, W, generator=g)
    if vel:
        d['vel'] = torch.randn(B, 2, H, W, generator=g)
    return d


def _anno(g, pi, cols):
    """boxes near their cells (as a trained head sees them), `cols` columns: 7 + whatever follows the yaw"""
    n = pi.shape[0]
    cx = (pi[:, 1].float() + 0.5) * 0.8 - 51.2
    cy = (pi[:, 2].float() + 0.5) * 0.8 - 51.2
    return torch.stack([cx + torch.randn(n, generator=g) * 0.2, cy + torch.randn(n, generator=g) * 0.2, torch.randn(n, generator=g),
                        torch.rand(n, generator=g) * 2 + 0.5, torch.rand(n, generator=g) * 4 + 0.5, torch.rand(n, generator=g) + 0.8,
                        (torch.rand(n, generator=g) - 0.5) * 6.28] + [torch.randn(n, generator=g) for _ in range(cols - 7)], -1)


def _objects(g, n, cols, avoid=()):
    """n random cells, none of them in `avoid` (a list of (b, x, y))"""
    pi = torch.stack([torch.randint(0, B, (n,), generator=g), torch.randint(0, W, (n,), generator=g),
                      torch.randint(0, H, (n,), generator=g)], -1)
    banned = {tuple(c) for c in avoid}
    for i in range(n):
        while tuple(pi[i].tolist()) in banned:
            pi[i] = torch.tensor([int(torch.randint(0, B, (1,), generator=g)), int(torch.randint(0, W, (1,), generator=g)),
                                  int(torch.randint(0, H, (1,), generator=g))])
    return pi, _anno(g, pi, cols)


def _tasks(g, sizes, reg=True, vel=True, cols=9):
    maps, pos, anno = [], [], []
    for n in sizes:
        maps.append(_maps(g, reg, vel))
        p, a = _objects(g, n, cols)
        if n > 10:
            p[5] = p[2]
            p[7] = p[2]                     # three objects in one cell
            a = _anno(g, p, cols)
        pos.append(p)
        anno.append(a)
    return maps, pos, anno


@functools.lru_cache(maxsize=None)
def build(name):
    g = torch.Generator().manual_seed(7000 + sum(map(ord, name)))
    if name == 'blocks':
        maps, pos, anno = _tasks(g, BLOCK_SIZES)
        up = [(1.0, 1.0)] * 8
        up[2], up[5] = (0.5, 3.0), (2.0, 0.25)
        return Case(name, maps, pos, anno, 0, 0, GD['gwd3d'], up=up)
    if name == 'lead':
        maps, pos, anno = _tasks(g, (0, 40, 260, 3))
        return Case(name, maps, pos, anno, 5, 9, GD['bd3d'], up=[(1.0, 1.0), (1.0, 1.0), (0.5, 3.0), (1.0, 1.0)])
    if name == 'shared':
        cells = [(0, 3, 4), (1, 7, 9), (1, 11, 15)]                        # of the triple, the pair, the crowd
        p0, _ = _objects(g, 600, 9, avoid=cells)
        for group, c in zip((TRIPLE, PAIR, CROWD), cells):
            p0[list(group)] = torch.tensor(c)
        p1, _ = _objects(g, 50, 9, avoid=cells)
        p1[3] = p1[44] = torch.tensor(cells[2])                            # the crowd's cell, in another task
        p1[20] = torch.tensor(cells[1])
        maps = [_maps(g, True, True), _maps(g, True, True)]
        return Case(name, maps, [p0, p1], [_anno(g, p0, 9), _anno(g, p1, 9)], 0, 3, GD['kld3d'], up=[(0.5, 3.0), (1.0, 1.0)])
    if name == 'numpos':
        maps, pos, anno = _tasks(g, NUMPOS_ROWS)
        return Case(name, maps, pos, anno, 2, 2, GD['gwd3d'], num_pos=list(NUMPOS), up=[(1.0, 1.0)] * 4 + [(3.0, 0.5)])
    if name.startswith('heads-'):
        reg, vel = '-reg-' in name, name.endswith('-vel')
        cols = 9 if vel or name.endswith('9') else 7
        maps, pos, anno = _tasks(g, (30, 0, 270), reg=reg, vel=vel, cols=cols)
        return Case(name, maps, pos, anno, 1, 1, GD['bd3d' if reg else 'kld3d'], up=[(1.0, 1.0), (1.0, 1.0), (0.5, 3.0)])
    if name == 'frozen':
        maps, pos, anno = _tasks(g, (30, 40, 50))
        frozen = [frozenset(('reg', 'vel')), frozenset(HEADS), frozenset()]
        return Case(name, maps, pos, anno, 0, 4, GD['gwd3d'], frozen=frozen, up=[(2.0, 0.5), (1.0, 1.0), (1.0, 1.0)])
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def graph_problems():
    """Two problems for one captured graph: same tasks, heads and capacity N = 1024, different split.  From the first to the second
    rows[0] moves from 0 to 7, task 1 grows from 200 to 300 objects (one workgroup -> two), task 2 becomes empty."""
    out = []
    for k, (lead, sizes) in enumerate(((0, (100, 200, 50, 45)), (7, (60, 300, 0, 45)))):
        g = torch.Generator().manual_seed(7700 + k)
        maps, pos, anno = _tasks(g, sizes)
        tail = GRAPH_N - lead - sum(sizes)
        out.append(Case(f'graph{k}', maps, pos, anno, lead, tail, GD['gwd3d'], up=[(1.0, 1.0), (0.5, 3.0), (2.0, 1.0), (1.0, 1.0)]))
    return tuple(out)


def oracle_of(case, dtype):
    """head_torch.center_head_task_losses per task on the per-task slices with avg = num_pos[t] (it clamps to max(., 1) itself),
    upstream gradients case.up -> ([(loss_l1, loss_gd)] as floats, [name -> gradient map as numpy; zeros where none flows])"""
    res, grads = [], []
    for t in range(case.T):
        dd = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in case.maps[t].items()}   # (never the case's own tensor)
        l1, gd = head_torch.center_head_task_losses(dd, case.pos[t], case.oracle_anno(t).to(dtype), float(case.num_pos[t]), CODER,
                                                    case.gd, L1_WEIGHT, case.code_weights)
        tot = case.up[t][0] * l1.sum() + case.up[t][1] * gd.sum()
        if tot.requires_grad:                  # the reference returns plain zeros for a task without objects
            tot.backward()
        res.append((float(l1.sum().detach()), float(gd.sum().detach())))
        grads.append({k: (v.grad.numpy() if v.grad is not None else np.zeros(v.shape)) for k, v in dd.items()})
    return res, grads


@functools.lru_cache(maxsize=None)
def expected(name, dtype):
    """oracle_of a named case, dtype 'float64' | 'float32'"""
    return oracle_of(build(name), getattr(torch, dtype))
