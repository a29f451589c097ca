"""The per-call plumbing between a torch tensor and an `extern "C"` entry point of libgd3d.so / libgd3d_extras.so, once: raw
stream / device accessors and the device guard, the pointer helpers, the GPU-only refusal, the GPU-or-`_cpu`-twin dispatch and its
extras counterpart, operand normalisation (contiguous fp32 / int64, the stacked point ops, the device-resident normaliser, the
threshold tensors), the dict-or-object config lookup, the bounded memo behind the workspace-size queries, the unit-gradient
registry, the double-backward guard of the autograd nodes, and the pinned count mailbox of the NMS calls.  Imports nothing from
the package but `_lib`; every module above the C ABI takes these from here.
"""
import threading
import time

import torch

from . import _lib

# raw-handle accessors: no Python-level device bookkeeping on the per-call path (`torch.cuda.device` + `current_stream()` was a
# third of nms_gpu's end-to-end time at inference sizes)
raw_stream = torch._C._cuda_getCurrentRawStream
get_device = torch._C._cuda_getDevice
set_device = torch._C._cuda_setDevice


class on_device:
    """Minimal device guard (raw accessors: no Python-level bookkeeping on the per-call path); yields the raw current stream."""
    __slots__ = ('idx', 'prev')

    def __init__(self, dev):
        self.idx = dev.index

    def __enter__(self):
        self.prev = get_device()
        if self.prev != self.idx:
            set_device(self.idx)
        return raw_stream(self.idx)

    def __exit__(self, *exc):
        if self.prev != self.idx:
            set_device(self.prev)
        return False


def ptr(t):
    """Address of t's data; None (a null pointer) for None."""
    return None if t is None else t.data_ptr()


def ptr_or_null(t):
    """As `ptr`, and a null pointer for an EMPTY tensor too (the stacked point ops: the kernels never touch a zero-row operand)."""
    return t.data_ptr() if t is not None and t.numel() > 0 else None


def gpu_only(t, who):
    """The wrappers without a `_cpu` twin refuse a CPU tensor here (a missing kernel is an error, never another path)."""
    if not t.is_cuda:
        raise RuntimeError(f'{who}: the MI355X implementation has no CPU path')


def f32c(t):
    """t as contiguous fp32; t itself when it already is."""
    if t.dtype != torch.float32:
        t = t.float()
    return t if t.is_contiguous() else t.contiguous()


def i64c(t):
    """t as contiguous int64; t itself when it already is."""
    if t.dtype != torch.int64:
        t = t.long()
    return t if t.is_contiguous() else t.contiguous()


_REQUIRED = object()


def cfg_get(cfg, key, default=_REQUIRED):
    """cfg[key] of a config dict or cfg.key of a config object / loss module; without a default a missing key raises."""
    if isinstance(cfg, dict):
        return cfg[key] if default is _REQUIRED else cfg.get(key, default)
    return getattr(cfg, key) if default is _REQUIRED else getattr(cfg, key, default)


def call(name, dev, args, cpu_tail=()):
    """GPU tensors: lib.<name>(*args, current stream of `dev`) under the device guard; CPU tensors: the twin
    lib.<name>_cpu(*args, *cpu_tail) — the twins end differently (a thread count, a reserved 0, nothing), so the caller spells the
    tail out.  A non-zero return code raises with the entry point's name."""
    lib = _lib.load()
    if dev.type == 'cuda':
        with on_device(dev) as stream:
            rc = getattr(lib, name)(*args, stream)
    else:
        name += '_cpu'
        rc = getattr(lib, name)(*args, *cpu_tail)
    _lib.check(rc, name)


def call_extras(name, dev, args):
    """`call` for libgd3d_extras.so: lib.<name>(*args, current stream of `dev`) under the device guard.  GPU tensors only: the
    extras have no `_cpu` twins."""
    lib = _lib.load_extras()
    with on_device(dev) as stream:
        rc = getattr(lib, name)(*args, stream)
    _lib.check(rc, name)


def rows_f32(t, cols, name):
    """A floating-point (rows, cols) operand (cols None: any width) as detached contiguous fp32."""
    if t.dim() != 2 or (cols is not None and t.size(1) != cols):
        raise RuntimeError(f'shape mismatch: {name} must be (rows, {cols if cols is not None else "C"}), got {tuple(t.shape)}')
    if not t.dtype.is_floating_point:
        raise RuntimeError(f'{name} must be a floating-point tensor, got {t.dtype}')
    return t.detach().to(torch.float32).contiguous()


def counts_i32(cnt, like, name):
    """A (batch_size,) integer count operand on `like`'s device as contiguous int32."""
    if cnt.dim() != 1:
        raise RuntimeError(f'{name} must be a (batch_size,) integer tensor, got shape {tuple(cnt.shape)}')
    if cnt.dtype.is_floating_point or cnt.dtype == torch.bool:
        raise RuntimeError(f'{name} must be an integer tensor, got {cnt.dtype}')
    if cnt.device != like.device:
        raise RuntimeError(f'{name} is on {cnt.device}, the points on {like.device}')
    return cnt.to(torch.int32).contiguous()


def avg_tensor(t, dev, who):
    """num_total_samples as a device-resident normaliser: one fp32 value on `dev`, detached"""
    if t.numel() != 1 or t.device != dev:
        raise RuntimeError(f'{who}: a tensor num_total_samples must hold one value on {dev}, got {tuple(t.shape)} on {t.device}')
    t = t.detach().reshape(())
    return t if t.dtype == torch.float32 else t.float()


_THRESH_CACHE = {}


def thresh_tensor(thresh, groups, dev):
    """One threshold, or one per group, as a (groups,) fp32 tensor on `dev`; remembered per (values, device)."""
    vals = tuple(float(t) for t in thresh) if isinstance(thresh, (list, tuple)) else (float(thresh),) * groups
    if len(vals) != groups:
        raise RuntimeError(f'{len(vals)} thresholds for {groups} groups')
    key = (vals, dev)
    t = _THRESH_CACHE.get(key)
    if t is None:
        if len(_THRESH_CACHE) > 64:
            _THRESH_CACHE.clear()
        t = _THRESH_CACHE[key] = torch.tensor(vals, dtype=torch.float32, device=dev)
    return t


def memo(fn, limit=4096):
    """fn(*key) remembered per key (the workspace-size queries: one ctypes call less per launch); the table empties itself once
    it holds more than `limit` keys."""
    table = {}

    def get(*key):
        v = table.get(key)
        if v is None:
            if len(table) > limit:
                table.clear()
            v = table[key] = fn(*key)
        return v
    return get


# ---- the unit gradient ----------------------------------------------------------------------------------------------------------

_UNIT_GRAD = {}     # device index (-1: the CPU) -> (the constant tensor, its address)


def unit_grad(device):
    """The upstream gradient 1.0 as a CONSTANT of this library: one read-only 0-dim fp32 tensor per device.

    `loss.backward()` makes torch fill a fresh ones tensor (one launch) and our backward then has to READ it on the device
    to learn that nothing needs scaling (one more launch, gd3d_grad_finish's early exit).  A training step that passes this
    tensor instead -- `torch.autograd.backward([l0, l1, l2], grad_tensors=[unit_grad(dev)] * 3)` -- is recognised by
    ADDRESS (no read, no sync): the gradients the fused forward launch wrote are already final and backward launches
    nothing.  Never write to the returned tensor."""
    dev = torch.device(device)
    if dev.type == 'cpu':
        idx = -1
    elif dev.type == 'cuda':
        idx = dev.index if dev.index is not None else get_device()
        dev = torch.device('cuda', idx)
    else:
        raise RuntimeError(f'unit_grad: no implementation for device type {dev.type!r}')
    u = _UNIT_GRAD.get(idx)
    if u is None:
        t = torch.ones((), dtype=torch.float32, device=dev)
        u = _UNIT_GRAD[idx] = (t, t.data_ptr())
        _lib.register_unit_grad(idx, u[1])     # the C++ node keeps an address table of its own
    return u[0]


def has_unit_grad(t):
    """Whether the constant of t's device exists yet."""
    return (t.device.index if t.is_cuda else -1) in _UNIT_GRAD


def is_unit_grad(g):
    """Whether g IS `unit_grad` of its device — by address: no read of the tensor."""
    u = _UNIT_GRAD.get(g.device.index if g.is_cuda else -1)
    return u is not None and g.data_ptr() == u[1] and g.dim() == 0 and g.dtype == torch.float32


def guard_double_backward(impl):
    """The backward functions of the package's autograd nodes return gradients that ctypes kernels wrote: no autograd graph hangs
    off them.  Under `create_graph=True` (the only case in which grad mode is ON inside a backward) the results are put behind
    torch's DelayedError node, so differentiating them again RAISES instead of silently treating them as constants.  That is what
    torch.autograd.function.once_differentiable does — except that it only does so when an incoming GRADIENT requires grad,
    which the ones tensor of a plain `autograd.grad(loss, x, create_graph=True)` does not; the gradients here depend on the
    saved INPUTS, so the guard is unconditional (as in the C++ twin).  A plain backward pays one flag test."""
    def backward(ctx, *grads):
        if not torch.is_grad_enabled():
            return impl(ctx, *grads)
        with torch.no_grad():
            outputs = impl(ctx, *grads)
        single = not isinstance(outputs, tuple)
        if single:
            outputs = (outputs,)
        err = torch._C._functions.DelayedError(
            b'trying to differentiate twice a function that was marked with @once_differentiable', len(outputs))
        alias = []
        for v in outputs:
            if v is not None:
                v = v.detach()
                v.requires_grad = True
            alias.append(v)
        res = err(*alias)
        return res[0] if single else res
    return backward


# ---- the count mailbox ----------------------------------------------------------------------------------------------------------
# An NMS result length is data dependent; instead of a blocking 8-byte device-to-host copy (a copy call + a stream
# synchronisation, ~10 us on this stack) the scan kernel writes its count straight into pinned host memory — every NMS entry point
# takes `num_keep` as a plain pointer — and the host polls the word: 55.0 -> 49.8 us per nms_gpu-sized call (n = 4096;
# profiles/r06_nms_batched.txt).  The kept ids stay on the device, stream-ordered as before.  One mailbox per thread, reused by
# every call: a call must not return, by ANY path, while a kernel of its own may still write a word (`launch_counted`).

PENDING = -(1 << 62)
_MAILBOX = threading.local()


def count_mailbox(g):
    """This thread's mailbox: (pinned int64 tensor, its numpy view) of at least g words."""
    cur = getattr(_MAILBOX, 'box', None)
    if cur is None or cur[0].numel() < g:
        t = torch.empty(max(64, g), dtype=torch.int64).pin_memory()
        cur = _MAILBOX.box = (t, t.numpy())
    return cur


def wait_counts(words, g, dev):
    """Poll the first g mailbox words until the kernels have written them all; returns them as ints.  After 0.2 s without them
    the device is synchronised and the words are read once more (a word still pending then raises)."""
    spins, deadline = 0, None
    while True:
        vals = [int(words[i]) for i in range(g)]
        if PENDING not in vals:
            return vals
        spins += 1
        if (spins & 0x3ff) == 0:
            now = time.perf_counter()
            if deadline is None:
                deadline = now + 0.2
            elif now > deadline:
                torch.cuda.synchronize(dev)
                vals = [int(words[i]) for i in range(g)]
                if PENDING in vals:
                    raise RuntimeError('nms_gpu: the NMS kernels finished without reporting a count')
                return vals


def kept_count(k, name):
    """A negative count is the scan kernel's failure mark (a wave of the list scan stopped making progress and its bounded polling
    loop gave up: never observed; a bug must surface as an error, not as a hang or a wrong list)."""
    if k < 0:
        raise RuntimeError(f'{name}: the device-side NMS scan gave up (num_keep = {k}); the result is void')
    return k


def launch_counted(g, dev, name, launch):
    """The whole mailbox protocol: mark g words pending, run `launch(address of the words, stream) -> rc` under the device guard,
    wait for the g counts and return them (each through `kept_count`).  A call that leaves early — a non-zero rc after a partial
    launch, an error or a KeyboardInterrupt while polling — synchronises its stream first: a kernel that wrote late would
    otherwise hit the word after the NEXT call has marked it pending and hand that call a wrong count.  (The pinned block is kept:
    a freed one can be handed out again while the kernel still writes to it.)"""
    box, words = count_mailbox(g)
    words[:g] = PENDING
    try:
        with on_device(dev) as stream:
            rc = launch(box.data_ptr(), stream)
        if rc != 0:
            _lib.check(rc, name)
        return [kept_count(k, name) for k in wait_counts(words, g, dev)]
    except BaseException:
        torch.cuda.current_stream(dev).synchronize()
        raise
