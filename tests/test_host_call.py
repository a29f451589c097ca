"""mmdet3d-gaussian_amd/_host.py — the per-call plumbing every module above the C ABI shares (pointer helpers, the GPU / `_cpu` twin
dispatch, the bounded memo, the count check) — and the group-cut helper of iou3d.py.  No GPU needed."""
import types

import numpy as np
import pytest
import torch

import nms_ref

import mmdet3d_gaussian_amd as amd
from mmdet3d_gaussian_amd import _host, iou3d

CPU = torch.device('cpu')


def test_ptr_maps_none_and_ptr_or_null_also_an_empty_tensor():
    full, empty = torch.zeros(3), torch.zeros((0, 3))
    assert _host.ptr(None) is None and _host.ptr_or_null(None) is None
    assert _host.ptr(full) == full.data_ptr() and _host.ptr_or_null(full) == full.data_ptr()
    assert _host.ptr_or_null(empty) is None
    assert _host.ptr(empty) == empty.data_ptr()      # `ptr` hands an empty tensor's address on as it is


def test_call_on_cpu_tensors_reaches_the_twin():
    """boxes_iou_bev on 3 x 2 boxes goes through `call` to riou_bev_xyxyr_cpu (tail: the thread count) and gives the IoU of
    tests/nms_ref.py's fp64 clipping.  Bound: the twin clips in fp32; with coordinates below 4 a vertex carries at most
    4 * 2^-24 = 2.4e-7 of rounding, an area of ~5 with a perimeter of ~10 therefore ~2.4e-6 absolute = 5e-7 relative, and the IoU
    (a ratio of two such areas) a few times that: 2e-6, the bound of the fixture tests in test_cpu_rbox.py."""
    a = np.array([[0.0, 0.0, 2.0, 3.0, 0.3], [-1.0, 0.5, 1.5, 2.5, -1.1], [1.0, 1.0, 3.5, 2.0, 2.0]], np.float32)
    b = np.array([[0.5, 0.25, 2.5, 2.75, 0.0], [-0.5, -0.5, 2.0, 3.5, 0.7]], np.float32)
    got = amd.boxes_iou_bev(torch.from_numpy(a), torch.from_numpy(b))
    assert got.shape == (3, 2) and got.dtype == torch.float32 and not got.is_cuda
    want = np.array([[nms_ref.exact_iou_xyxyr(x, y) for y in b] for x in a])
    assert want.min() > 0.05                          # every pair overlaps: no entry is trivially 0
    np.testing.assert_allclose(got.numpy(), want, rtol=0, atol=2e-6)


def test_call_passes_the_tail_and_raises_with_the_entry_points_name(monkeypatch):
    seen = []

    def twin(*args):
        seen.append(args)
        return 0

    def failing(*args):
        return 10001
    lib = types.SimpleNamespace(op_cpu=twin, bad_cpu=failing)
    monkeypatch.setattr(_host._lib, 'load', lambda: lib)
    _host.call('op', CPU, (1, 2.5, None), (7,))
    _host.call('op', CPU, (1,), (0,))
    _host.call('op', CPU, (3, 4))
    assert seen == [(1, 2.5, None, 7), (1, 0), (3, 4)]
    with pytest.raises(RuntimeError, match=r'bad_cpu failed with code 10001 \(bad argument\)'):
        _host.call('bad', CPU, (1,), (0,))
    with pytest.raises(AttributeError):               # a GPU-only entry point has no twin: an error, not another path
        _host.call('gpu_only', CPU, ())


@pytest.mark.parametrize('post_max_size', [None, 0, 1, 3, 9, -1])
def test_cut_groups_equals_the_loop_it_replaces(post_max_size):
    G, cap, nums = 3, 5, [0, 5, 2]
    keep = torch.arange(G * cap, dtype=torch.int64).reshape(G, cap) * 3 + 1
    want = []
    for g in range(G):
        k = keep[g, :nums[g]]
        want.append(k if post_max_size is None else k[:post_max_size])
    got = iou3d._cut_groups(keep, nums, post_max_size)
    assert len(got) == G
    for x, y in zip(got, want):
        assert x.dtype == torch.int64 and torch.equal(x, y)
    none = iou3d._no_groups(G, CPU)
    assert len(none) == G and all(k.shape == (0,) and k.dtype == torch.int64 for k in none)
    assert len({id(k) for k in none}) == G            # separate tensors, as the comprehension gave


def test_kept_count_raises_on_the_scan_failure_mark():
    assert _host.kept_count(0, 'nms_gpu') == 0
    assert _host.kept_count(17, 'nms_gpu') == 17
    with pytest.raises(RuntimeError, match='nms_gpu: the device-side NMS scan gave up'):
        _host.kept_count(-1, 'nms_gpu')


def test_memo_returns_the_cached_value_and_empties_itself_past_4096_keys():
    calls = []

    def size(a, b):
        calls.append((a, b))
        return a * 1000 + b
    get = _host.memo(size)
    assert get(3, 4) == 3004 and get(3, 4) == 3004 and calls == [(3, 4)]
    for k in range(4096):                             # 4097 keys now: still all remembered
        get(k, -1)
    assert len(calls) == 4097
    assert get(3, 4) == 3004 and get(0, -1) == -1 and len(calls) == 4097
    get(5000, 0)                                      # the table held more than 4096 keys: emptied, then this one stored
    assert len(calls) == 4098
    assert get(5000, 0) == 5000000 and len(calls) == 4098
    assert get(3, 4) == 3004 and len(calls) == 4099   # forgotten with the rest: asked again


def test_the_workspace_memos_go_through_it():
    """gd_loss._ws_floats keeps its name and signature (tests/test_autograd_node.py uses it)."""
    from mmdet3d_gaussian_amd import gd_loss
    lib = amd.load_library()
    assert gd_loss._ws_floats(64) == lib.gd3d_loss_workspace_bytes(64) // 4 == gd_loss._ws_floats(64)
    assert iou3d._ws_bytes(700) == lib.rnms_workspace_bytes(700)
    assert iou3d._batched_ws_bytes(3, 700, 500) == lib.rnms_batched_scored_workspace_bytes(3, 700, 500)
