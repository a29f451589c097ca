"""The device-resident form of the centre-head losses, `center_head_losses(..., rows=...)`, on the MI355X: `rows_dev`, `avg_dev` and
`center_dyn()` of csrc/gd3d_center_head.hip with both accumulate forms (the scan, and stage -> stable sort -> sorted finish).

Cases: tests/center_rows_cases.py (their edges are asserted without a GPU in tests/test_center_rows_cases.py).  References:
oracle/head_torch.py on the per-task slices in fp64 / fp32 under the suite's head-slice rule (`_tol_check`: 1e-5 + 3 x the
reference's own fp32 error, relative to 1 + |r64|), and the host form of the same kernels bit for bit.  Before every device-form
call the workspace the call is about to take from the caching allocator is filled with NaN, so a partial sum, key or staged row
read past a task's own objects shows."""
import functools

import pytest
import torch

import center_rows_cases as cc
from test_gpu_kernel_instances import _tol_check

pytestmark = pytest.mark.gpu
L1 = dict(type='L1Loss', reduction='mean', loss_weight=cc.L1_WEIGHT)
FORMS = {'scan': 10 ** 9, 'sorted': 0}       # head_loss.CENTER_SORT_MIN_N that selects the form


@pytest.fixture(scope='module')
def amd():
    import mmdet3d_gaussian_amd as m
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    m.load_library()
    return m


def _modules(amd, case):
    kw = {k: v for k, v in case.gd.items() if k not in ('loss_type', 'loss_weight')}
    mod = amd.GDLoss(case.gd['loss_type'], loss_weight=case.gd['loss_weight'], **kw)
    coder = amd.CenterPointBBoxYawCoder(pc_range=cc.CODER['pc_range'], out_size_factor=cc.CODER['out_size_factor'],
                                        voxel_size=cc.CODER['voxel_size'], norm_bbox=cc.CODER['norm_bbox'])
    return mod, coder


def _leaves(case):
    return [{k: v.detach().cuda().requires_grad_(k not in case.frozen[t]) for k, v in case.maps[t].items()} for t in range(case.T)]


def _finish(case, out, leaves):
    """backward with the case's upstream gradients -> (losses (T, 2) on the host, per task name -> gradient | None)"""
    assert len(out) == case.T and all(o[0].dim() == 0 and o[1].dim() == 0 for o in out)
    total = sum(u[0] * o[0] + u[1] * o[1] for u, o in zip(case.up, out))
    if total.requires_grad:
        total.backward()
    torch.cuda.synchronize()
    losses = torch.stack([torch.stack((o[0], o[1])) for o in out]).detach().cpu()
    return losses, [{k: (None if v.grad is None else v.grad.cpu()) for k, v in d.items()} for d in leaves]


def _dirty_workspace(leaves, N):
    """NaN into the blocks the next device-form call over `leaves` with capacity N takes from the caching allocator: its
    allocations (gradient maps + cell counters, losses, workspace) are made here in the same order and sizes and freed again"""
    from mmdet3d_gaussian_amd import _lib
    T = len(leaves)
    flat = sum(v.numel() for d in leaves for v in d.values() if v.requires_grad)
    flat += sum(cc.B * cc.H * cc.W for d in leaves if any(v.requires_grad for v in d.values()))
    sizes = (flat, 2 * T, _lib.load().gd3d_center_head_workspace_bytes(T, N) // 4)
    blocks = [torch.full((n,), float('nan'), dtype=torch.float32, device='cuda') for n in sizes]
    torch.cuda.synchronize()
    del blocks


def run_rows(amd, case, form, shared=None):
    """the device-resident form; shared = (pos, anno, rows) replaces the case's own shared arrays"""
    from mmdet3d_gaussian_amd import head_loss
    mod, coder = _modules(amd, case)
    sp, sa, rows = shared if shared is not None else (case.shared_pos, case.shared_anno, case.rows)
    leaves = _leaves(case)
    sp, sa, rows, npos = sp.cuda(), sa.cuda(), rows.cuda(), case.num_pos.cuda()
    keep = head_loss.CENTER_SORT_MIN_N
    head_loss.CENTER_SORT_MIN_N = FORMS[form]
    try:
        _dirty_workspace(leaves, sp.shape[0])
        out = amd.center_head_losses(mod, L1, coder, leaves, sp, sa, npos, case.code_weights, rows=rows)
        return _finish(case, out, leaves)
    finally:
        head_loss.CENTER_SORT_MIN_N = keep


def run_host(amd, case):
    """the host form on the per-task slices, num_pos as Python floats"""
    mod, coder = _modules(amd, case)
    leaves = _leaves(case)
    out = amd.center_head_losses(mod, L1, coder, leaves, [p.cuda() for p in case.pos], [a.cuda() for a in case.anno],
                                 [float(v) for v in case.num_pos.tolist()], case.code_weights)
    return _finish(case, out, leaves)


@functools.lru_cache(maxsize=None)
def rows_result(name, form):
    import mmdet3d_gaussian_amd as m
    return run_rows(m, cc.build(name), form)


@functools.lru_cache(maxsize=None)
def host_result(name):
    import mmdet3d_gaussian_amd as m
    return run_host(m, cc.build(name))


def _check_task_vs_oracle(case, t, losses, grads, r64, g64, r32, g32, tag):
    for j in range(2):
        _tol_check(f'{tag}.task{t}.loss{j}', losses[t, j].item(), r64[t][j], r32[t][j])
    for k in case.maps[t]:
        if k in case.frozen[t]:
            assert grads[t][k] is None, (tag, t, k)
            continue
        got = grads[t][k]
        assert got is not None and got.shape == case.maps[t][k].shape, (tag, t, k)
        _tol_check(f'{tag}.task{t}.{k}', got.numpy(), g64[t][k], g32[t][k])
        outside = ~case.cells(t)[:, None].expand_as(got)
        assert not bool(outside.any()) or float(got[outside].abs().max()) == 0.0, (tag, t, k)       # nothing written outside the cells of this task's slice
    if case.pos[t].shape[0] == 0:
        assert losses[t, 0].item() == 0.0 and losses[t, 1].item() == 0.0, (tag, t)
        assert all(float(g.abs().max()) == 0.0 for g in grads[t].values() if g is not None), (tag, t)


@pytest.mark.parametrize('form', tuple(FORMS))
@pytest.mark.parametrize('name', cc.NAMES)
def test_rows_form_vs_oracle(amd, name, form):
    """both losses of every task and the gradient of every head map against head_torch.center_head_task_losses on the per-task
    slices with avg = num_pos[t] (the oracle clamps to max(., 1) itself: tests/test_center_rows_cases.py), upstream gradients
    != 1 on some tasks; empty tasks exactly 0, frozen maps without a gradient, zero outside the slice's cells"""
    case = cc.build(name)
    losses, grads = rows_result(name, form)
    r64, g64 = cc.expected(name, 'float64')
    r32, g32 = cc.expected(name, 'float32')
    assert losses.shape == (case.T, 2) and bool(torch.isfinite(losses).all()), losses
    for t in range(case.T):
        _check_task_vs_oracle(case, t, losses, grads, r64, g64, r32, g32, f'{name}.{form}')


def _same(a, b):
    la, ga = a
    lb, gb = b
    if not torch.equal(la, lb):
        return False
    for da, db in zip(ga, gb):
        for k in da:
            if (da[k] is None) != (db[k] is None) or (da[k] is not None and not torch.equal(da[k], db[k])):
                return False
    return True


@pytest.mark.parametrize('form', tuple(FORMS))
@pytest.mark.parametrize('name', cc.NAMES)
def test_rows_form_equals_the_host_form_bit_for_bit(amd, name, form):
    """the same kernels fed per-task arrays and max(num_pos, 1) divided on the host: equal losses and gradients"""
    assert _same(rows_result(name, form), host_result(name))
    assert float(host_result(name)[0].abs().max()) > 0.0


@pytest.mark.parametrize('name', cc.NAMES)
def test_scan_and_sorted_accumulate_agree_bit_for_bit(amd, name):
    """both add a cell's objects in ascending object index"""
    assert _same(rows_result(name, 'scan'), rows_result(name, 'sorted'))


@pytest.mark.parametrize('form', tuple(FORMS))
@pytest.mark.parametrize('owner', ('prev', 'next'))
def test_a_boundary_moved_into_a_poison_row_turns_exactly_that_task_nan(amd, owner, form):
    """`blocks` with one poison row between the data of tasks 2 and 3.  `rows` are contiguous boundaries, so that row belongs to
    one of the two: with rows[3] moved one row into it ('prev') task 2 reads it, with rows[3] in front of it ('next') task 3
    does.  That task's losses are NaN; every other task still equals the oracle, gradients included."""
    case = cc.build('blocks')
    sp, sa, rows, hit = cc.with_gap(case, 3, owner)
    losses, grads = run_rows(amd, case, form, shared=(sp, sa, rows))
    r64, g64 = cc.expected('blocks', 'float64')
    r32, g32 = cc.expected('blocks', 'float32')
    for t in range(case.T):
        if t == hit:
            assert bool(torch.isnan(losses[t]).all()), (t, losses[t])
        else:
            assert bool(torch.isfinite(losses[t]).all()), (t, losses[t])
            _check_task_vs_oracle(case, t, losses, grads, r64, g64, r32, g32, f'gap.{owner}.{form}')


def test_graph_replay_with_the_split_changed_on_the_device(amd):
    """forward + backward of the scan form captured once over static shared buffers of N = 1024; a second problem is copied in
    place (pos, anno, maps, rows, num_pos: rows[0] moves, one task becomes empty, one grows from 200 to 300 objects and takes a
    second workgroup) and replayed, then the first again: losses and gradients equal an eager host-form call, bit for bit"""
    from mmdet3d_gaussian_amd import head_loss
    first, second = cc.graph_problems()
    mod, coder = _modules(amd, first)
    names = sorted(first.maps[0])
    leaves = [{k: first.maps[t][k].cuda().requires_grad_(True) for k in names} for t in range(first.T)]
    sp, sa = first.shared_pos.cuda(), first.shared_anno.cuda()
    rows, npos = first.rows.cuda(), first.num_pos.cuda()
    up = first.up

    def load(case):
        with torch.no_grad():
            sp.copy_(case.shared_pos)
            sa.copy_(case.shared_anno)
            rows.copy_(case.rows)
            npos.copy_(case.num_pos)
            for t in range(case.T):
                for k in names:
                    leaves[t][k].copy_(case.maps[t][k])

    def step():
        for d in leaves:
            for v in d.values():
                v.grad = None
        out = amd.center_head_losses(mod, L1, coder, leaves, sp, sa, npos, first.code_weights, rows=rows)
        sum(u[0] * o[0] + u[1] * o[1] for u, o in zip(up, out)).backward()
        return torch.stack([torch.stack((o[0], o[1])) for o in out]).detach(), [[d[k].grad for k in names] for d in leaves]
    keep = head_loss.CENTER_SORT_MIN_N
    head_loss.CENTER_SORT_MIN_N = FORMS['scan']
    try:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            l_g, g_g = step()
        for case in (second, first):
            load(case)
            graph.replay()
            torch.cuda.synchronize()
            got = (l_g.cpu(), [{k: g.cpu() for k, g in zip(names, gs)} for gs in g_g])
            want = run_host(amd, case)
            assert _same(got, want), case.name
            assert bool(torch.isfinite(got[0]).all()) and float(got[0][1].abs().min()) > 0.0
            empty = [t for t in range(case.T) if case.pos[t].shape[0] == 0]
            assert all(float(got[0][t].abs().max()) == 0.0 for t in empty) and (case is first or empty == [2])
    finally:
        head_loss.CENTER_SORT_MIN_N = keep
