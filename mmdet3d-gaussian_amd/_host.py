"""The per-call plumbing between a torch tensor and an `extern "C"` entry point of libgd3d.so, once: raw stream / device
accessors and the device guard, the pointer helpers, the GPU-or-`_cpu`-twin dispatch, operand normalisation of the stacked point
ops, the bounded memo behind the workspace-size queries, and the pinned count mailbox of the NMS calls.  Imports nothing from the
package but `_lib`; every module above the C ABI takes these from here.
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
