"""The generator of the device-resident centre-head cases (tests/center_rows_cases.py) keeps the edges its cases are named for, and
the fp64 oracle is finite on all of them: a later edit of the generator cannot quietly lose what tests/test_gpu_center_head_rows.py
relies on.  No GPU."""
import numpy as np
import pytest
import torch

import center_rows_cases as cc
from center_rows_cases import B, H, W, HEAD_T, WAVE


def _is_poison(case, lo, hi, sp=None, sa=None):
    sp = case.shared_pos if sp is None else sp
    sa = case.shared_anno if sa is None else sa
    p, a = sp[lo:hi], sa[lo:hi]
    outside = (p[:, 0] < 0) | (p[:, 0] >= B) | (p[:, 1] < 0) | (p[:, 1] >= W) | (p[:, 2] < 0) | (p[:, 2] >= H)
    return bool(outside.all()) and bool(torch.isnan(a).all())


@pytest.mark.parametrize('name', cc.NAMES)
def test_shared_form_is_the_per_task_lists_with_poison_around(name):
    c = cc.build(name)
    rows = c.rows.tolist()
    assert len(rows) == c.T + 1 and 1 <= c.T <= 8 and c.num_pos.shape == (c.T,) and c.num_pos.dtype == torch.float32
    assert rows[0] >= 0 and rows[-1] <= c.N == c.shared_pos.shape[0] == c.shared_anno.shape[0]
    assert c.shared_pos.dtype == torch.int64 and c.shared_anno.dtype == torch.float32
    for t in range(c.T):
        assert rows[t + 1] - rows[t] == c.pos[t].shape[0] == c.anno[t].shape[0]
        assert torch.equal(c.shared_pos[rows[t]:rows[t + 1]], c.pos[t]) and torch.equal(c.shared_anno[rows[t]:rows[t + 1]], c.anno[t])
        p = c.pos[t]
        assert bool(((p >= 0) & (p < torch.tensor([B, W, H]))).all()) and bool(torch.isfinite(c.anno[t]).all())
        assert c.anno[t].shape[1] == c.shared_anno.shape[1] >= 7 + (2 if c.vel else 0)
        assert set(c.maps[t]) == {'height', 'dim', 'yaw', 'dir'} | ({'reg'} if c.reg else set()) | ({'vel'} if c.vel else set())
        assert all(tuple(m.shape) == (B, cc.CHANNELS[k], H, W) for k, m in c.maps[t].items())
    assert _is_poison(c, 0, rows[0]) and _is_poison(c, rows[-1], c.N)
    assert len(c.code_weights) == (4 if c.vel else 2)
    assert any(u != (1.0, 1.0) for u in c.up)                    # center_scale_kernel has something to do
    # fp32-exact normalisers: the device's division and the host's round alike
    assert all(float(np.float32(v)) == v for v in c.num_pos.double().tolist())


def test_blocks_slices_start_off_block_multiples_and_end_around_one():
    c = cc.build('blocks')
    sizes = [p.shape[0] for p in c.pos]
    assert sizes == [37, 0, 300, 255, 256, 257, 1, 0] and c.T == 8
    rows = c.rows.tolist()
    assert all(rows[t] % HEAD_T != 0 for t in range(1, 8))                         # no slice but the first starts on a block multiple
    assert {n - HEAD_T for n in sizes} >= {-1, 0, 1}                              # one below, at, one above a block of objects
    assert sizes[1] == 0 and sizes[7] == 0 and 0 < sizes[0] < HEAD_T < sizes[2]   # empty in the middle and at the end
    assert max(sizes) > HEAD_T and c.N > 4 * HEAD_T                               # several workgroups per task row
    for owner in ('prev', 'next'):
        sp, sa, r, hit = cc.with_gap(c, 3, owner)
        r = r.tolist()
        assert hit == (2 if owner == 'prev' else 3) and r[-1] <= sp.shape[0] == c.N + 1
        for t in range(8):
            n_poison = sum(_is_poison(c, i, i + 1, sp, sa) for i in range(r[t], r[t + 1]))
            assert n_poison == (1 if t == hit else 0)
            own = sp[r[t]:r[t + 1]]
            own = own[(own[:, 0] < B)]
            assert torch.equal(own, c.pos[t])


def test_lead_starts_past_row_zero_with_an_empty_first_task():
    c = cc.build('lead')
    rows = c.rows.tolist()
    assert rows[0] == 5 and rows[1] == 5 and c.pos[0].shape[0] == 0 and c.N > rows[-1]
    assert _is_poison(c, 0, 5) and _is_poison(c, rows[-1], c.N)
    assert max(p.shape[0] for p in c.pos) > HEAD_T


def test_shared_cells_within_a_task_across_blocks_and_across_tasks():
    c = cc.build('shared')
    p0, p1 = c.pos
    assert p0.shape[0] == 600 and c.T == 2
    key0 = (p0[:, 0] * H + p0[:, 2]) * W + p0[:, 1]
    key1 = (p1[:, 0] * H + p1[:, 2]) * W + p1[:, 1]

    def members(i):
        return tuple(torch.nonzero(key0 == key0[i]).reshape(-1).tolist())
    assert members(2) == (2, 5, 7)
    assert members(10) == (10, 300) and 10 // HEAD_T != 300 // HEAD_T          # owner and contributor in different workgroups
    crowd = members(cc.CROWD[0])
    assert crowd == cc.CROWD and len(crowd) == 70 > WAVE
    assert len({i // HEAD_T for i in crowd}) == 3 and len({i // WAVE for i in crowd}) > 2
    # the crowd's cell and the pair's also appear in task 1, which must keep its own sums
    assert int((key1 == key0[cc.CROWD[0]]).sum()) == 2 and int((key1 == key0[10]).sum()) == 1
    assert len({members(2), members(10), crowd}) == 3


def test_numpos_differs_from_the_row_counts():
    c = cc.build('numpos')
    assert c.num_pos.tolist() == [0.0, 0.5, 1.0, 37.0, 1000.0]
    sizes = [p.shape[0] for p in c.pos]
    assert all(n > 0 and float(n) != v and float(n) != max(v, 1.0) for n, v in zip(sizes, c.num_pos.tolist()))
    assert max(sizes) > HEAD_T


def test_heads_cover_reg_and_vel_both_ways():
    seen = set()
    for name in cc.NAMES:
        if name.startswith('heads-'):
            c = cc.build(name)
            seen.add((c.reg, c.vel, c.shared_anno.shape[1]))
            assert len(c.code_weights) == (4 if c.vel else 2)
    assert seen == {(True, True, 9), (True, False, 7), (False, True, 9), (False, False, 9)}


def test_frozen_masks():
    c = cc.build('frozen')
    assert c.T == 3 and c.frozen[0] == {'reg', 'vel'} and c.frozen[1] >= set(c.maps[1]) and c.frozen[2] == set()
    assert all(p.shape[0] > 0 for p in c.pos)


def test_graph_problems_share_a_capacity_and_differ_in_the_split():
    a, b = cc.graph_problems()
    assert a.N == b.N == cc.GRAPH_N and a.T == b.T and a.rows[-1] <= a.N and b.rows[-1] <= b.N
    sa, sb = [p.shape[0] for p in a.pos], [p.shape[0] for p in b.pos]
    assert int(a.rows[0]) != int(b.rows[0])
    assert sa[1] == 200 and sb[1] == 300 and sa[1] <= HEAD_T < sb[1]          # one workgroup -> two
    assert sa[2] > 0 and sb[2] == 0
    assert a.code_weights == b.code_weights and a.up == b.up and a.gd == b.gd
    for c in (a, b):
        assert _is_poison(c, 0, int(c.rows[0])) and _is_poison(c, int(c.rows[-1]), c.N)


@pytest.mark.parametrize('name', cc.NAMES)
def test_oracle_is_finite_and_zero_on_empty_tasks(name):
    """head_torch.center_head_task_losses in fp64: finite losses and gradients on every case, exactly zero for empty tasks, and
    it clamps the normaliser to max(num_pos, 1) itself (so the GPU tests hand it num_pos unclamped)"""
    from oracle import head_torch
    c = cc.build(name)
    res, grads = cc.expected(name, 'float64')
    cc.expected(name, 'float32')
    assert not any(m.requires_grad for d in c.maps for m in d.values())          # the oracle works on copies: the case stays as built
    for t in range(c.T):
        assert all(np.isfinite(v) for v in res[t]) and all(np.isfinite(g).all() for g in grads[t].values())
        if c.pos[t].shape[0] == 0:
            assert res[t] == (0.0, 0.0) and all((g == 0).all() for g in grads[t].values())
        else:
            assert res[t][0] > 0.0 and res[t][1] != 0.0
            inside = c.cells(t).numpy()
            for k, g in grads[t].items():
                assert (g[np.broadcast_to(~inside[:, None], g.shape)] == 0).all() and np.abs(g).max() > 0, (t, k)
    for t in range(c.T):
        if c.pos[t].shape[0] and float(c.num_pos[t]) < 1.0:
            dd = {k: v.double() for k, v in c.maps[t].items()}
            lo = head_torch.center_head_task_losses(dd, c.pos[t], c.oracle_anno(t).double(), float(c.num_pos[t]), cc.CODER, c.gd,
                                                    cc.L1_WEIGHT, c.code_weights)
            one = head_torch.center_head_task_losses(dd, c.pos[t], c.oracle_anno(t).double(), 1.0, cc.CODER, c.gd, cc.L1_WEIGHT,
                                                     c.code_weights)
            assert float(lo[0]) == float(one[0]) and float(lo[1]) == float(one[1])
