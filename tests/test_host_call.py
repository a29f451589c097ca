"""mmdet3d-gaussian_amd/_host.py — the per-call plumbing every module above the C ABI shares (pointer helpers, the GPU / `_cpu` twin
dispatch and its extras counterpart, operand normalisation, the config lookup, the GPU-only refusal, the unit-gradient registry, the
bounded memo, the count check) — and the group-cut helper of iou3d.py.  No GPU needed."""
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


def test_f32c_and_i64c_return_the_operand_itself_when_it_already_is():
    f, i = torch.arange(12, dtype=torch.float32).reshape(3, 4), torch.arange(5)
    assert _host.f32c(f) is f and _host.i64c(i) is i
    for fn, dtype, ops in ((_host.f32c, torch.float32, (f.t(), f[:, ::2], f.half(), torch.arange(6, dtype=torch.int32))),
                           (_host.i64c, torch.int64, (torch.arange(12).reshape(3, 4).t(), torch.arange(6, dtype=torch.int32), f))):
        for t in ops:
            got = fn(t)
            assert got is not t and got.dtype == dtype and got.is_contiguous() and got.shape == t.shape
            assert torch.equal(got, t.to(dtype))


def test_cfg_get_reads_a_dict_or_an_object_and_raises_only_without_a_default():
    d, o = dict(gamma=2.0, alpha=None), types.SimpleNamespace(gamma=3.0, alpha=None)
    assert _host.cfg_get(d, 'gamma', 1.0) == 2.0 and _host.cfg_get(o, 'gamma', 1.0) == 3.0
    assert _host.cfg_get(d, 'alpha', 0.25) is None and _host.cfg_get(o, 'alpha', 0.25) is None   # present: not the default
    assert _host.cfg_get(d, 'beta', 1.0) == 1.0 and _host.cfg_get(o, 'beta', 1.0) == 1.0
    assert _host.cfg_get(d, 'beta', None) is None and _host.cfg_get(o, 'beta', None) is None
    assert _host.cfg_get(d, 'gamma') == 2.0 and _host.cfg_get(o, 'gamma') == 3.0
    with pytest.raises(KeyError):
        _host.cfg_get(d, 'beta')
    with pytest.raises(AttributeError):
        _host.cfg_get(o, 'beta')


def test_gpu_only_refuses_a_cpu_tensor_with_the_one_sentence():
    with pytest.raises(RuntimeError) as e:
        _host.gpu_only(torch.zeros(2), 'select_best')
    assert str(e.value) == 'select_best: the MI355X implementation has no CPU path'
    with pytest.raises(RuntimeError, match='^center_head_heatmap_loss: the MI355X implementation has no CPU path$'):
        amd.extras.center_head_heatmap_loss(dict(type='GaussianFocalLoss'), [torch.zeros(1, 1, 2, 2)], [torch.zeros(1, 1, 2, 2)])


def test_call_extras_appends_the_stream_under_the_guard_and_raises_with_the_entry_points_name(monkeypatch):
    seen, current = [], [0]

    def op(*args):
        seen.append((current[0],) + args)
        return 0
    lib = types.SimpleNamespace(op=op, bad=lambda *args: 10002)
    monkeypatch.setattr(_host._lib, 'load_extras', lambda: lib)
    monkeypatch.setattr(_host, 'get_device', lambda: current[0])
    monkeypatch.setattr(_host, 'set_device', lambda i: current.__setitem__(0, i))
    monkeypatch.setattr(_host, 'raw_stream', lambda i: 0x5000 + i)
    _host.call_extras('op', torch.device('cuda', 1), (1, 2.5, None))
    _host.call_extras('op', torch.device('cuda', 0), ())
    assert seen == [(1, 1, 2.5, None, 0x5001), (0, 0x5000)]     # ran with the tensors' device current, on ITS current stream
    assert current[0] == 0
    with pytest.raises(RuntimeError, match=r'^bad failed with code 10002 \(too large\)$'):
        _host.call_extras('bad', torch.device('cuda', 1), (1,))
    assert current[0] == 0
    with pytest.raises(AttributeError):               # an entry point the library does not have: an error, not another path
        _host.call_extras('missing', torch.device('cuda', 1), ())
    assert current[0] == 0


def test_the_unit_gradient_is_known_by_address_alone():
    from mmdet3d_gaussian_amd import gd_loss
    u = _host.unit_grad('cpu')
    assert gd_loss.unit_grad is _host.unit_grad and gd_loss.unit_grad('cpu') is u and _host.unit_grad(CPU) is u
    assert u.dim() == 0 and u.dtype == torch.float32 and float(u) == 1.0
    assert _host.is_unit_grad(u) and _host.has_unit_grad(torch.zeros(1))
    assert not _host.is_unit_grad(u.clone())
    assert not _host.is_unit_grad(u.reshape(1))                         # the same address, one dimension
    assert not _host.is_unit_grad(torch.ones((), dtype=torch.float64))
    with pytest.raises(RuntimeError, match='unit_grad: no implementation'):
        _host.unit_grad('meta')


@pytest.mark.parametrize('glue', ['python', None])
def test_the_unit_gradient_is_recognised_whichever_glue_is_loaded_after_it(glue):
    """The constant exists BEFORE the glue is (re)loaded — the order the two tables of earlier versions depended on: the same
    tensor is still the unit gradient, and `.backward()` of a CPU GDLoss value (which starts from it: gd_loss.LossValue) gives
    the gradients of an explicit ones gradient bit for bit."""
    from mmdet3d_gaussian_amd import _lib
    u = _host.unit_grad('cpu')
    g = torch.Generator().manual_seed(3)
    tgt = torch.rand(33, 7, generator=g) * torch.tensor([40, 40, 2, 3, 3, 2, 3.0]) + torch.tensor([0, 0, 0, 0.5, 0.5, 0.5, -1.5])
    pred = tgt + 0.1 * torch.randn(33, 7, generator=g)
    mod = amd.build_loss(dict(type='GDLoss', loss_type='kld3d', fun='log1p', tau=1.0, loss_weight=5.0))
    try:
        _lib.set_host_glue(glue)
        _lib.load_node()
        assert _host.unit_grad('cpu') is u and _host.is_unit_grad(u)
        grads = []
        for explicit in (False, True):
            p, t = pred.clone().requires_grad_(True), tgt.clone().requires_grad_(True)
            out = mod(p, t)
            out.backward(gradient=torch.ones(())) if explicit else out.backward()
            grads.append((p.grad, t.grad))
        assert grads[0][0].abs().max() > 0 and grads[0][1].abs().max() > 0
        assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
    finally:
        _lib.set_host_glue(None)
