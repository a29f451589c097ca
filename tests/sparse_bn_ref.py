"""Reference side of the live-row batch normalisation tests (include/gd3d.h, gd3d_sparse_bn_*).

* `oracle`   torch's `F.batch_norm`, then the add, then the ReLU, in fp64 on the LIVE rows only (gathered with `sparse_conv_ref.active_rows`),
             on operands already rounded to the kernel's type; the gradients by fp64 autograd.  The ReLU of the gradient chain is the mask
             the run under test produced (the forward check holds that mask to the oracle's wherever the two can be told apart).
* `chain`    D: the longest chain of dependent fp32 additions of the device's summation for (R, C, type) — a lane's rows, the LDS tree,
             the merge of the tiles — restated from csrc/sparse_bn_common.h.
* `bound`    (k D + c) u A per quantity, u = 2^-24, with A the scale of the quantity's own terms (DESIGN.md §3.21 derives k, c and A); a
             16-bit output adds its one final rounding, E + u16 (|want| + E), as in §3.19.
"""
import numpy as np
import torch
import torch.nn.functional as F

import sparse_conv_ref as ref

U = 2.0 ** -24
U16 = {'fp16': 2.0 ** -11, 'bf16': 2.0 ** -8}
DTYPES = {'fp32': torch.float32, 'fp16': torch.float16, 'bf16': torch.bfloat16}
KINDS = tuple(DTYPES)
T, P, BLOCK = 64, 256, 256             # the row tile, the cap on the partials, the workgroup (csrc/sparse_bn_common.h)
# (k, c) of the bound (k D + c) u A, per quantity
COEF = dict(out=(1, 12), mean=(1, 12), invstd=(1, 12), rm=(1, 12), rv=(1, 12), gb=(1, 2), gw=(3, 16), gx=(5, 40))


def cut_rows(R):
    """-> (tiles, chunk) as csrc/sparse_bn_common.h cuts R rows"""
    t = min(max((R + T - 1) // T, 1), P)
    c = max(((R + t - 1) // t + T - 1) // T * T, T)
    return ((R + c - 1) // c if R > 0 else 0), c


def lanes_of(C, kind):
    """-> (vec, groups, rows): channels a lane owns, lanes across a row, rows a workgroup covers at a time"""
    wide = 4 if kind == 'fp32' else 8
    vec = wide if C % wide == 0 else 1
    return vec, C // vec, BLOCK // (C // vec)


def chain(R, C, kind):
    """D of the device's sums over R rows"""
    tiles, chunk = cut_rows(R)
    rows = lanes_of(C, kind)[2]
    return -(-chunk // rows) + int(np.ceil(np.log2(rows))) + -(-max(tiles, 1) // 64) + 6


def rounded(a, kind):
    """a rounded to the kernel's type, as fp64 numpy"""
    return torch.from_numpy(np.asarray(a, np.float32)).to(DTYPES[kind]).double().numpy()


def oracle(x, gamma, beta, rm, rv, res, gy, mask, training, momentum, eps):
    """x, res, gy, mask: the LIVE rows (res, mask None: absent); gamma, beta, rm, rv (C,) or None -> (o64, A): dicts of fp64 numpy arrays
    out (before and after the ReLU: `pre`, `out`), mean, invstd, rm, rv (training), gx, gres, gw, gb"""
    f64 = lambda a: None if a is None else np.asarray(a, np.float64)
    x, gamma, beta, rm, rv, res, gy = (f64(a) for a in (x, gamma, beta, rm, rv, res, gy))
    n, C = x.shape
    t = lambda a, grad=False: None if a is None else torch.tensor(np.asarray(a, np.float64), requires_grad=grad)
    X, G, Bt, Rs = t(x, True), t(gamma, True), t(beta, True), t(res, True)
    batch = training or rm is None
    rm64, rv64 = (None, None) if rm is None else (t(rm), t(rv))
    y = F.batch_norm(X, rm64, rv64, G, Bt, batch, momentum, eps)
    pre = y if Rs is None else y + Rs
    out = pre if mask is None else pre * torch.from_numpy(mask.astype(np.float64))
    inputs = [v for v in (X, G, Bt, Rs) if v is not None]
    grads = iter(torch.autograd.grad(out, inputs, t(gy)))
    gx = next(grads).numpy()
    gw = next(grads).numpy() if G is not None else None
    gb = next(grads).numpy() if Bt is not None else None
    gres = next(grads).numpy() if Rs is not None else None
    ax = np.abs(x)
    g = np.abs(gy) if mask is None else np.abs(gy) * mask
    ag = np.ones(C) if gamma is None else np.abs(gamma)
    ab = np.zeros(C) if beta is None else np.abs(beta)
    ar = 0.0 if res is None else np.abs(res)
    if batch:
        mean, var = x.mean(0), x.var(0)
        invstd, abar = 1.0 / np.sqrt(var + eps), ax.mean(0)               # abar: the scale of the mean's own terms (>= |mean|)
    else:
        mean, invstd, abar = np.asarray(rm, np.float64), 1.0 / np.sqrt(np.asarray(rv, np.float64) + eps), np.abs(rm)
    s, xa = ag * invstd, invstd * (ax + abar)
    o64 = dict(pre=pre.detach().numpy(), out=np.maximum(pre.detach().numpy(), 0.0) if mask is not None else pre.detach().numpy(), mean=mean, invstd=invstd,
               gx=gx, gw=gw, gb=gb, gres=gres)
    A = dict(out=s * (ax + abar) + ab + ar, mean=abar, invstd=invstd, gb=g.sum(0), gw=(g * xa).sum(0))
    A['gx'] = s * (g + g.sum(0) / max(n, 1) + xa * (g * xa).sum(0) / max(n, 1)) if batch else g * s
    if training and rm is not None:
        o64['rm'], o64['rv'] = rm64.numpy(), rv64.numpy()
        A['rm'] = (1 - momentum) * np.abs(rm) + momentum * abar
        A['rv'] = (1 - momentum) * np.abs(rv) + momentum * x.var(0, ddof=1)
    return o64, A


def within(got, want, A, key, D, kind=None):
    """-> (|got - want| <= (k D + c) u A everywhere [a 16-bit quantity: + u16 (|want| + E)], the worst |got - want| / A)"""
    k, c = COEF[key]
    err = np.abs(np.asarray(got, np.float64) - want)
    E = (k * D + c) * U * A
    if kind in U16:
        E = E + U16[kind] * (np.abs(want) + E)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(A > 0, err / A, 0.0)
    return bool((err <= E).all()), float(ratio.max()) if ratio.size else 0.0


def live_rows(coors, shape, B):
    return ref.active_rows(np.asarray(coors), shape, B)
