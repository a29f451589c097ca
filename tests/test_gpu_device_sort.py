"""The library's rocPRIM unit (csrc/device_sort.hip) on the MI355X through the three ops that call it, in each regime of the radix sort
of (int64, int32) pairs on gfx950: one block up to 1024 items, the merge sort up to 1 048 576, Onesweep above.  scatter_index against
the ATen statement, hard_voxelize and sparse_conv_index against their `_cpu` twins; a regular 3x3x3 index takes the keys sort and
the exclusive scan past 1 048 576 candidates.  Integer outputs (and copied rows): exact equality."""
import numpy as np
import pytest
import torch

import mmdet3d_gaussian_amd as amd
from mmdet3d_gaussian_amd.scatter import _index_and_grouping, _index_and_grouping_torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROWS = [1000, 5000, 1_100_000]      # one block; merge sort; Onesweep
SHAPE, B = (16, 200, 200), 2        # 1 280 000 cells: room for 1.1 M unique rows


@pytest.mark.parametrize('n', ROWS)
def test_scatter_index_in_every_sort_regime(n):
    rng = np.random.default_rng(n)
    coors = np.stack([rng.integers(0, h, n) for h in (B,) + SHAPE], -1).astype(np.int32)
    coors[n // 2:n // 2 + 100] = coors[:100]                                              # voxels of more than one point
    coors[::97, 3] = -1                                                                   # dropped points
    t = torch.from_numpy(coors).to(DEV)
    got, want = _index_and_grouping(t), _index_and_grouping_torch(t)
    assert 0 < got[0].size(0) < n and (got[1] < 0).any()                                  # shared voxels and dropped points
    for a, b in zip(got[:3] + got[3], want[:3] + want[3]):
        assert a.dtype == b.dtype and torch.equal(a, b)


@pytest.mark.parametrize('n', ROWS)
def test_hard_voxelize_in_every_sort_regime(n):
    """2 slots a voxel and 20 000 voxels a sample keep the twin's walk and the outputs small; every point is still keyed, sorted and scanned"""
    rng = np.random.default_rng(n + 1)
    pts = torch.from_numpy(rng.uniform(-1.0, 41.0, (n, 4)).astype(np.float32))           # about 1 in 7 outside the range
    cnt = torch.tensor([n // 3, n - n // 3], dtype=torch.int32)
    run = lambda dev: amd.hard_voxelize(pts.to(dev), (0.2, 0.2, 2.5), (0, 0, 0, 40, 40, 40), 2, 20000, points_batch_cnt=cnt.to(dev), static=True)
    got, want = run(DEV), run('cpu')
    assert 0 < int(want[3].sum()) <= min(n, 40000)
    for k, a, b in zip(('voxels', 'coors', 'num_points', 'voxel_batch_cnt'), got, want):
        assert a.dtype == b.dtype and torch.equal(a.cpu(), b), k


def unique_rows(n, seed):
    """n distinct active rows [b, z, y, x] in random order, every 50th made inactive"""
    rng = np.random.default_rng(seed)
    cell = rng.permutation(B * SHAPE[0] * SHAPE[1] * SHAPE[2])[:n]
    coors = np.stack(np.unravel_index(cell, (B,) + SHAPE), -1).astype(np.int32)
    coors[::50, 1] = -1
    return torch.from_numpy(coors)


def check_index(coors, **kw):
    got, want = (amd.sparse_conv_index(coors.to(dev), SHAPE, B, **kw) for dev in (DEV, 'cpu'))
    for k in ('out_coors', 'nbr', 'nbr_t', 'num', 'out_batch_cnt'):
        a, b = getattr(got, k), getattr(want, k)
        assert (a is None) == (b is None), k
        if a is not None:
            assert a.dtype == b.dtype and torch.equal(a.cpu(), b), k
    return want


@pytest.mark.parametrize('n', ROWS)
def test_sparse_conv_index_pairs_sort_in_every_regime(n):
    want = check_index(unique_rows(n, n + 2), kernel_size=1, subm=True)
    assert int(want.num[0]) == n and int(want.out_batch_cnt.sum()) == n - (n + 49) // 50


def test_sparse_conv_index_keys_sort_and_scan_past_the_merge_sort_limit():
    """41 000 rows x 27 offsets = 1 107 000 candidates > 1 048 576: the keys sort, the exclusive scan and the compaction over them"""
    want = check_index(unique_rows(41_000, 5), kernel_size=3, stride=2, padding=1, subm=False)
    assert 41_000 * 27 > 1_048_576 and 0 < int(want.num[0]) == want.out_coors.size(0)
