"""PV-RCNN's keypoint segmentation slice through the `_cpu` twins (csrc/seg_head_cpu.cpp): `pvrcnn_seg_loss` and `keypoint_reweight`
on CPU tensors against the statement-by-statement torch restatement of the reference (tests/pvrcnn_seg_ref.py).

  * n_pos and the winner columns equal the fp32 restatement exactly;
  * the loss value within 1e-5 (relative) of the fp64 restatement;
  * every other tensor — the gradient of seg_preds, the reweighted features, both reweight gradients — within the larger of 4x the fp32
    restatement's own largest deviation from fp64 on the same inputs and one fp32 ulp (2^-23) of the tensor's largest fp64 magnitude
    (printed per case; DESIGN.md §3.12 records the largest ratios);
and the autograd wiring, the dtype rule, the argument checks and the twin under sanitizers as a stand-alone program.

Figures: every case passes, on the `_cpu` twin and on gfx950; the largest |ours - fp64| / bound per tensor is in DESIGN.md §3.12's table."""
import pytest
import torch

import mmdet3d_gaussian_amd as amd
import pvrcnn_seg_ref as ref
from mmdet3d_gaussian_amd import _host, pvrcnn_seg

LOSS_KEYS = ('grad',)
REWEIGHT_KEYS = ('out', 'grad_feats', 'grad_seg')


def run_loss(case, dev='cpu', unit=False):
    """the package's loss, n_pos and gradient of a case on `dev` -> dict like pvrcnn_seg_ref.evaluate_loss's (on the CPU)"""
    x = case['seg_preds'].to(dev).clone().requires_grad_(True)
    t = case['seg_targets'].to(dev)
    loss = amd.pvrcnn_seg_loss(case['cfg'], x, t, ref.NUM_CLASSES, case['class_agnostic'])['loss_seg']
    assert loss.dim() == 0 and loss.dtype == torch.float32
    if unit:
        (grad,) = torch.autograd.grad(loss, x, grad_outputs=_host.unit_grad(loss.device))
    else:
        loss.backward()
        grad = x.grad
    cfg = case['cfg']
    raw, _ = pvrcnn_seg._launch_seg_loss(x.detach(), t, (cfg['gamma'], cfg['alpha'], cfg['loss_weight'], ref.NUM_CLASSES, case['class_agnostic']), False)
    assert torch.equal(raw[0], loss.detach())       # the forward-only form (null gradient pointer): the same loss
    return dict(loss=loss.detach().cpu(), n_pos=raw[1].cpu(), grad=grad.cpu())


def run_reweight(case, dev='cpu', view=lambda t: t):
    f = view(case['feats'].to(dev).clone()).requires_grad_(True)       # never the shared case tensor itself
    x = case['seg_preds'].to(dev).clone().requires_grad_(True)
    out = amd.keypoint_reweight(f, x)
    out.backward(view(case['grad_out'].to(dev)))
    _, win = pvrcnn_seg._launch_reweight(f.detach(), x.detach(), True)
    with torch.no_grad():
        assert torch.equal(amd.keypoint_reweight(f, x), out)       # the forward-only form (no winner array): the same features
    return dict(out=out.detach().cpu(), win=win.cpu().long(), grad_feats=f.grad.cpu(), grad_seg=x.grad.cpu())


def check_loss_case(got, name, what):
    """the assertions the CPU and the GPU file share"""
    case, r32, r64 = ref.loss_reference(name)
    assert float(got['n_pos']) == float(r32['n_pos']), f'{what} {name}: n_pos {float(got["n_pos"])} against {float(r32["n_pos"])}'
    ref.check_loss_value(got['loss'], r64['loss'], f'{what} {name}')
    figures = ref.check_values(got, r32, r64, LOSS_KEYS, f'{what} {name}')
    weightless = ~((case['seg_targets'] >= 0) & (case['seg_targets'] <= ref.NUM_CLASSES))
    assert not got['grad'][weightless].any(), 'an ignored row, or one past background, has a zero gradient row'
    if name.startswith('all_ignored'):
        assert float(got['loss']) == 0.0 and not got['grad'].any()
    if name.startswith('no_positive'):
        assert float(got['n_pos']) == 0.0 and float(got['loss']) > 0.0      # the normaliser clamps to 1
    if name.startswith('targets_past_background'):
        # 2^40, -2^63 and 2^63 - 1 are targets like any other past background: not counted, no gradient (a 32-bit read of the target
        # would see 0, 0 and -1: a positive of class 0 twice)
        t = case['seg_targets']
        rows = torch.tensor(ref.INT64_EXTREME_ROWS)
        assert t[rows].tolist() == list(ref.INT64_EXTREMES) and not got['grad'][rows].any()
        assert float(got['n_pos']) == float(((t >= 0) & (t < ref.NUM_CLASSES)).sum())
    return figures


def check_reweight_case(got, name, what):
    case, r32, r64 = ref.reweight_reference(name)
    assert torch.equal(got['win'], r32['win']), f'{what} {name}: winner columns differ from the fp32 restatement'
    figures = ref.check_values(got, r32, r64, REWEIGHT_KEYS, f'{what} {name}')
    off = torch.ones_like(got['grad_seg'], dtype=torch.bool).scatter_(1, got['win'][:, None], False)
    assert not got['grad_seg'][off].any(), 'the whole gradient goes to the winning column'
    if name == 'exact_ties':
        assert got['win'][0::4].eq(0).all() and got['win'][1::4].eq(1).all() and got['win'][2::4].eq(0).all()    # the lowest tied column
        assert got['grad_seg'][0::4, 0].ne(0).all()
    if name == 'saturated':
        s = case['seg_preds'].sigmoid().reshape(-1)                # the fp32 sigmoid: exactly 1 at 30 and 100, exactly 0 at -100
        flat = (s == 0) | (s == 1)
        assert flat[0] and flat[2] and flat[3] and not flat[1]
        assert not got['grad_seg'].reshape(-1)[flat].any()
    if name == 'n130_c8_k255':
        k = case['seg_preds'].size(1)
        want = torch.tensor(ref.forced_columns(k))[torch.arange(got['win'].numel()) % 4]
        assert ref.forced_columns(k) == (0, 127, 128, 254) and torch.equal(got['win'], want)      # the byte's top bit included
        assert got['grad_seg'].gather(1, want[:, None]).ne(0).all() and r64['grad_seg'].gather(1, want[:, None]).ne(0).all()
    return figures


@pytest.mark.parametrize('name', sorted(ref.LOSS_CASES))
def test_seg_loss_twin_matches_the_restatement(name):
    case = ref.loss_reference(name)[0]
    got = run_loss(case)
    check_loss_case(got, name, 'cpu twin')
    again = run_loss(case, unit=True)                # the same bits on every run, and through the unit-gradient path
    for k in got:
        assert torch.equal(got[k], again[k]), k


@pytest.mark.parametrize('name', ref.ALL_REWEIGHT_CASES)
def test_reweight_twin_matches_the_restatement(name):
    case = ref.reweight_reference(name)[0]
    got = run_reweight(case)
    check_reweight_case(got, name, 'cpu twin')
    again = run_reweight(case)
    for k in got:
        assert torch.equal(got[k], again[k]), k


def test_reweight_misaligned_base_equals_the_aligned_case():
    """C = 128 with every (N, C) operand viewed one float into a larger buffer (4-byte aligned pointers only): the same bits"""
    case = ref.reweight_reference(ref.MISALIGNED_OF)[0]
    aligned, shifted = run_reweight(case), run_reweight(case, view=ref.offset_view)
    for k in aligned:
        assert torch.equal(aligned[k], shifted[k]), k


SENTINEL = -77.0
SINGLE_SHIFTS = ('fwd.feats', 'fwd.out', 'bwd.grad_out', 'bwd.feats', 'bwd.grad_feats')     # every pointer either entry reads as float4


def reweight_entries(case, dev='cpu', shift=(), win=None):
    """`gd3d_keypoint_reweight` and `gd3d_keypoint_reweight_backward` (or their twins) on sentinel-filled outputs with a guard row either
    side.  An operand named in `shift` ('fwd.' / 'bwd.' + feats, out, grad_out, grad_feats) starts one float into a larger buffer: its
    pointer is 4-byte aligned only; every other pointer is 16-byte aligned when C % 4 == 0.  `win`: a byte the backward reads as every
    row's winner instead of the forward's.  Asserts that every output element is written and no guard is -> dict like run_reweight's"""
    N, C = case['feats'].shape
    K = case['seg_preds'].size(1)

    def operand(t, name):
        t = t.to(dev).contiguous()
        t = ref.offset_view(t) if name in shift else t
        assert t.data_ptr() % 16 == (4 if name in shift else 0)
        return t

    def guarded(cols, name):
        off = 1 if name in shift else 0
        buf = torch.full(((N + 2) * cols + 8,), SENTINEL, device=dev)
        rows = buf[off:off + (N + 2) * cols].view(N + 2, cols)
        if cols % 4 == 0:
            assert rows[1:].data_ptr() % 16 == 4 * off
        return rows

    x = case['seg_preds'].to(dev).contiguous()
    out, gf, gx = guarded(C, 'fwd.out'), guarded(C, 'bwd.grad_feats'), guarded(K, 'bwd.grad_seg')
    won = torch.full((N + 2,), 200, dtype=torch.uint8, device=dev)
    f_fwd, f_bwd, g = operand(case['feats'], 'fwd.feats'), operand(case['feats'], 'bwd.feats'), operand(case['grad_out'], 'bwd.grad_out')   # kept alive
    _host.call('gd3d_keypoint_reweight', x.device, (f_fwd.data_ptr(), x.data_ptr(), N, C, K, out[1:].data_ptr(), won[1:].data_ptr()))
    assert won[0] == 200 and won[-1] == 200 and (won[1:-1] < K).all()
    used = won if win is None else torch.full_like(won, win)
    _host.call('gd3d_keypoint_reweight_backward', x.device,
               (g.data_ptr(), f_bwd.data_ptr(), x.data_ptr(), used[1:].data_ptr(), N, C, K, gf[1:].data_ptr(), gx[1:].data_ptr()))
    for buf in (out, gf, gx):
        assert (buf[0] == SENTINEL).all() and (buf[-1] == SENTINEL).all(), 'a guard row was written'
        assert not (buf[1:-1] == SENTINEL).any(), 'an output element was left unwritten'
    return dict(out=out[1:-1].cpu().contiguous(), win=won[1:-1].cpu().long(), grad_feats=gf[1:-1].cpu().contiguous(), grad_seg=gx[1:-1].cpu().contiguous())


def check_entries_equal_the_wrapper(name, dev='cpu'):
    """every element of the four arrays written, the guard rows either side intact, and the wrapper's bits"""
    case = ref.reweight_reference(name)[0]
    got, want = reweight_entries(case, dev), run_reweight(case, dev=dev)
    for k in want:
        assert torch.equal(got[k], want[k]), k


def check_single_misaligned_operand(shift, dev='cpu'):
    """ONE operand one float into a larger buffer, every other pointer 16-byte aligned, C = 128: the launch has to leave the 16-byte
    path on that pointer alone, and gives the all-aligned run's bits (a decision that looked at another pointer only would read or
    write a float4 at an address that is no multiple of 16)"""
    case = ref.reweight_reference(ref.MISALIGNED_OF)[0]
    assert case['feats'].size(1) % 4 == 0 and shift in SINGLE_SHIFTS
    aligned, shifted = reweight_entries(case, dev), reweight_entries(case, dev, shift=(shift,))
    for k in aligned:
        assert torch.equal(aligned[k], shifted[k]), (shift, k)


def check_foreign_winner_bytes(name, dev='cpu'):
    """a winner array from elsewhere holding 200 where K = 3: the backward clamps the byte to K - 1 (the kernel's comment), so the
    gradient lands in the last column, computed with that column's sigmoid, and nothing is accessed past the row (reweight_entries
    asserts the guard rows either side of grad_seg and that every element between them is written)"""
    case = ref.reweight_reference(name)[0]
    K = case['seg_preds'].size(1)
    assert K == 3
    got, last = reweight_entries(case, dev, win=200), reweight_entries(case, dev, win=K - 1)
    for k in got:
        assert torch.equal(got[k], last[k]), k
    assert not got['grad_seg'][:, :K - 1].any() and got['grad_seg'][:, K - 1].ne(0).all()
    want = {}
    for dtype in (torch.float32, torch.float64):            # what "column K - 1 won" means, in plain torch
        f, x, g = (case[k].to(dtype) for k in ('feats', 'seg_preds', 'grad_out'))
        s = x[:, K - 1].sigmoid()
        gx = torch.zeros_like(x)
        gx[:, K - 1] = (g * f).sum(dim=1) * (s * (1 - s))
        want[dtype] = dict(grad_feats=g * s[:, None], grad_seg=gx)
    ref.check_values(got, want[torch.float32], want[torch.float64], ('grad_feats', 'grad_seg'), f'{dev} {name} winner byte 200')


def check_one_sided_backward(name, dev='cpu'):
    """only `feats`, then only `seg_preds`, requires a gradient: the other gradient pointer is null (the kernel skips the dot product,
    or leaves the loop before its shuffles) and the one computed has the two-sided run's bits"""
    case = ref.reweight_reference(name)[0]
    both = run_reweight(case, dev=dev)
    for key, wanted in (('grad_feats', 'feats'), ('grad_seg', 'seg_preds')):
        ops = {k: case[k].to(dev).clone() for k in ('feats', 'seg_preds')}
        ops[wanted].requires_grad_(True)
        amd.keypoint_reweight(ops['feats'], ops['seg_preds']).backward(case['grad_out'].to(dev))
        other = 'seg_preds' if wanted == 'feats' else 'feats'
        assert ops[other].grad is None and torch.equal(ops[wanted].grad.cpu(), both[key]), key


@pytest.mark.parametrize('name', ['n65_c3_k3', 'n67_c260_k3', 'n130_c8_k255'] + list(ref.SWEEP_CASES))
def test_reweight_entry_points_write_every_element_and_nothing_beyond(name):
    check_entries_equal_the_wrapper(name)


@pytest.mark.parametrize('shift', SINGLE_SHIFTS)
def test_reweight_single_misaligned_operand_equals_the_aligned_run(shift):
    check_single_misaligned_operand(shift)


@pytest.mark.parametrize('name', ['n65_c3_k3', 'n130_c128_k3'])
def test_reweight_backward_clamps_a_foreign_winner_byte(name):
    check_foreign_winner_bytes(name)


def test_reweight_one_sided_backward_equals_the_two_sided_run():
    check_one_sided_backward('n130_c128_k3')


def test_sweep_cases_pass_the_grid_cap():
    """the arithmetic the sweep cases stand on, from the shapes themselves: N rows > 8192 workgroups x 4 rows per workgroup"""
    for name in ref.SWEEP_CASES:
        case = ref.reweight_reference(name)[0]
        N, C = case['feats'].shape
        rows = 256 // min(64, 1 << max(0, ((C + 3) // 4 - 1).bit_length()))       # RW_BLOCK / group_lanes(C)
        assert rows == ref.SWEEP_ROWS and N > ref.SWEEP_CAP * rows and N - ref.SWEEP_CAP * rows == 5
    assert ref.reweight_reference('n32773_c256_k3')[0]['feats'].size(1) % 4 == 0      # the 16-byte path
    assert ref.reweight_reference('n32773_c255_k1')[0]['feats'].size(1) % 4 == 3      # the 4-byte path, a clipped last quad


def test_reweight_empty_and_forward_only(monkeypatch):
    f, x = torch.zeros(0, 8, requires_grad=True), torch.zeros(0, 3, requires_grad=True)
    calls = _count_calls(monkeypatch)
    out = amd.keypoint_reweight(f, x)
    assert out.shape == (0, 8) and out.dtype == torch.float32 and calls() == 0        # N = 0: an empty tensor, no launch
    out.sum().backward()
    assert f.grad.shape == (0, 8) and x.grad.shape == (0, 3)
    case = ref.reweight_reference('n65_c3_k3')[0]
    out = amd.keypoint_reweight(case['feats'], case['seg_preds'])                      # nothing requires a gradient
    assert not out.requires_grad and torch.equal(out, run_reweight(case)['out'])
    only_x = case['seg_preds'].clone().requires_grad_(True)                            # one operand: the other gradient is not computed
    amd.keypoint_reweight(case['feats'], only_x).backward(case['grad_out'])
    assert torch.equal(only_x.grad, run_reweight(case)['grad_seg'])


def _count_calls(monkeypatch):
    """counts the entry points reached through _host.call from here on -> a function returning their number"""
    seen = []
    real = _host.call

    def counted(name, dev, args, cpu_tail=()):
        seen.append(name)
        return real(name, dev, args, cpu_tail)
    monkeypatch.setattr(_host, 'call', counted)
    return lambda: len(seen)


def test_seg_loss_autograd_wiring(monkeypatch):
    case, r32, _ = ref.loss_reference('n65_k3')
    x = case['seg_preds'].clone().requires_grad_(True)
    loss = amd.pvrcnn_seg_loss(case['cfg'], x, case['seg_targets'], ref.NUM_CLASSES)['loss_seg']
    stored = loss.grad_fn.state[0]
    n = _count_calls(monkeypatch)
    (g,) = torch.autograd.grad(loss, x, grad_outputs=_host.unit_grad('cpu'), retain_graph=True)
    assert g.data_ptr() == stored.data_ptr() and n() == 0            # the stored buffer itself, nothing launched
    (g3,) = torch.autograd.grad(loss, x, grad_outputs=torch.tensor(3.0), retain_graph=True)
    assert torch.equal(g3, stored * 3.0) and n() == 0                 # a non-unit upstream gradient scales it (an elementwise op, no launch of ours)
    (3.0 * loss).backward()
    assert torch.equal(x.grad, g3)
    # our op is fp32: its gradient is compared with the restatement's (above, per case); finite differences are for the restatement alone
    small = ref.make_loss('n63_k3')
    x64 = small['seg_preds'][:6].double().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda v: ref.seg_loss(v, small['seg_targets'][:6], ref.NUM_CLASSES, False, ref.LOSS_SEG)[0], (x64,))
    x1 = small['seg_preds'][:6, :1].double().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda v: ref.seg_loss(v, small['seg_targets'][:6], ref.NUM_CLASSES, True, ref.LOSS_SEG)[0], (x1,))
    f64, s64 = torch.randn(5, 4, dtype=torch.float64, requires_grad=True), ref.gapped_logits(5, 3, torch.Generator().manual_seed(3)).double().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b: ref.reweight(a, b)[0], (f64, s64))


def test_double_backward_raises():
    case = ref.loss_reference('n63_k1')[0]
    x = case['seg_preds'].clone().requires_grad_(True)
    loss = amd.pvrcnn_seg_loss(case['cfg'], x, case['seg_targets'], ref.NUM_CLASSES, class_agnostic=True)['loss_seg']
    (g,) = torch.autograd.grad(loss, x, create_graph=True)
    with pytest.raises(RuntimeError, match='differentiate twice'):
        g.sum().backward()
    rw = ref.reweight_reference('n65_c4_k1')[0]
    f, s = rw['feats'].clone().requires_grad_(True), rw['seg_preds'].clone().requires_grad_(True)
    gf, gs = torch.autograd.grad(amd.keypoint_reweight(f, s).sum(), (f, s), create_graph=True)
    with pytest.raises(RuntimeError, match='differentiate twice'):
        (gf.sum() + gs.sum()).backward()


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16, torch.float64])
def test_other_dtypes_are_evaluated_in_fp32_and_cast_back(dtype):
    case = ref.loss_reference('n65_k3')[0]
    x = case['seg_preds'].to(dtype).requires_grad_(True)
    x32 = x.detach().float().requires_grad_(True)
    loss = amd.pvrcnn_seg_loss(case['cfg'], x, case['seg_targets'], ref.NUM_CLASSES)['loss_seg']
    loss32 = amd.pvrcnn_seg_loss(case['cfg'], x32, case['seg_targets'], ref.NUM_CLASSES)['loss_seg']
    loss.backward()
    loss32.backward()
    assert loss.dtype == dtype and x.grad.dtype == dtype
    assert torch.equal(loss.detach(), loss32.detach().to(dtype)) and torch.equal(x.grad, x32.grad.to(dtype))
    rw = ref.reweight_reference('n65_c4_k1')[0]
    f, s = rw['feats'].to(dtype).requires_grad_(True), rw['seg_preds'].to(dtype).requires_grad_(True)
    f32, s32 = f.detach().float().requires_grad_(True), s.detach().float().requires_grad_(True)
    out, out32 = amd.keypoint_reweight(f, s), amd.keypoint_reweight(f32, s32)
    out.backward(rw['grad_out'].to(dtype))
    out32.backward(rw['grad_out'].to(dtype).float())
    assert out.dtype == dtype and f.grad.dtype == dtype and s.grad.dtype == dtype
    assert torch.equal(out.detach(), out32.detach().to(dtype))
    assert torch.equal(f.grad, f32.grad.to(dtype)) and torch.equal(s.grad, s32.grad.to(dtype))


class _Module:
    """a loss module stand-in: attributes instead of keys"""
    def __init__(self, **kw):
        self.__dict__.update(kw)


def test_argument_checks():
    case = ref.loss_reference('n63_k3')[0]
    x, t = case['seg_preds'], case['seg_targets']
    focal = type('FocalLoss', (), {})()
    focal.__dict__.update(use_sigmoid=True, reduction='sum', gamma=2.0, alpha=0.25, loss_weight=1.0, activated=False)
    ok = amd.pvrcnn_seg_loss(focal, x, t, 3)                                    # a module, by class name and attributes
    assert torch.equal(ok['loss_seg'], amd.pvrcnn_seg_loss(ref.LOSS_SEG, x, t, 3)['loss_seg']) and list(ok) == ['loss_seg']
    half = amd.pvrcnn_seg_loss(dict(ref.LOSS_SEG, loss_weight=0.5), x, t, 3)['loss_seg']
    assert torch.allclose(half, 0.5 * ok['loss_seg'], rtol=1e-6)                # loss_weight is honoured
    with pytest.raises(RuntimeError, match='shape mismatch'):                   # a wrong K for class_agnostic
        amd.pvrcnn_seg_loss(ref.LOSS_SEG, x, t, 3, class_agnostic=True)
    with pytest.raises(RuntimeError, match='shape mismatch'):
        amd.pvrcnn_seg_loss(ref.LOSS_SEG, x[:, :1], t, 3, class_agnostic=False)
    with pytest.raises(RuntimeError, match='shape mismatch'):
        amd.pvrcnn_seg_loss(ref.LOSS_SEG, x, t[:-1], 3)
    with pytest.raises(RuntimeError, match='integer tensor'):                   # float seg_targets
        amd.pvrcnn_seg_loss(ref.LOSS_SEG, x, t.float(), 3)
    with pytest.raises(RuntimeError, match='floating-point'):
        amd.pvrcnn_seg_loss(ref.LOSS_SEG, x.long(), t, 3)
    meta = torch.device('meta')
    with pytest.raises(RuntimeError, match='is on'):                            # tensors on different devices
        amd.pvrcnn_seg_loss(ref.LOSS_SEG, x, t.to(meta), 3)
    for bad in (dict(ref.LOSS_SEG, type='CrossEntropyLoss'), dict(ref.LOSS_SEG, use_sigmoid=False), dict(ref.LOSS_SEG, activated=True),
                dict(ref.LOSS_SEG, reduction='mean'), dict(ref.LOSS_SEG, gamma=-1.0), dict(ref.LOSS_SEG, alpha=1.5), _Module(reduction='sum')):
        with pytest.raises(RuntimeError, match='loss_seg'):
            amd.pvrcnn_seg_loss(bad, x, t, 3)
    with pytest.raises(RuntimeError, match='at most 255'):
        amd.pvrcnn_seg_loss(ref.LOSS_SEG, torch.zeros(2, 256), torch.zeros(2, dtype=torch.int64), 256)
    f = torch.zeros(4, 8)
    with pytest.raises(RuntimeError, match='1 <= K <= 255'):                    # K = 256
        amd.keypoint_reweight(f, torch.zeros(4, 256))
    with pytest.raises(RuntimeError, match='1 <= K <= 255'):
        amd.keypoint_reweight(f, torch.zeros(4, 0))
    with pytest.raises(RuntimeError, match='C >= 1'):
        amd.keypoint_reweight(torch.zeros(4, 0), torch.zeros(4, 1))
    assert amd.keypoint_reweight(f, torch.zeros(4, 255)).shape == (4, 8)        # K = 255 is the limit
    with pytest.raises(RuntimeError, match='shape mismatch'):
        amd.keypoint_reweight(f, torch.zeros(5, 1))
    with pytest.raises(RuntimeError, match='shape mismatch'):
        amd.keypoint_reweight(f.long(), torch.zeros(4, 1))
    with pytest.raises(RuntimeError, match='is on'):
        amd.keypoint_reweight(f, torch.zeros(4, 1, device=meta))
    assert 'pvrcnn_seg_loss' in amd.__all__ and 'keypoint_reweight' in amd.__all__


def test_host_twin_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """csrc/seg_head_cpu.cpp compiled together with a stand-alone driver (tests/hostmath/seg_head_sanitize.cpp, its own main) under
    -fsanitize=address,undefined and run as a program on the CPU: exactly sized heap buffers on the edge shapes — N = 0, N = 1, null
    gradient pointers, a null winner array, K = 255.  A sanitizer build belongs on a CPU-only machine: with a GPU present the test skips
    before it compiles or starts anything."""
    if torch.cuda.is_available():
        pytest.skip('sanitizer builds run on a CPU-only machine, never where a GPU is present')
    import os
    import subprocess
    from mmdet3d_gaussian_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = _lib._build.host_cxx_path()
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'seg_head_sanitize')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-ffp-contract=off',
           os.path.join(root, 'tests', 'hostmath', 'seg_head_sanitize.cpp'),
           os.path.join(root, 'mmdet3d-gaussian_amd', 'csrc', 'seg_head_cpu.cpp'), '-o', exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.rstrip().endswith('OK') and 'runtime error' not in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
