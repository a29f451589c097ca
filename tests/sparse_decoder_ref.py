"""Reference side of the sparse decoder tests: the inverse convolution, the max pooling and SparseUNet.

* `inverse_oracle`  densify the (R, Cin) features at `out_coors` in fp64, `F.conv_transpose3d` with output_padding = (n + 2p - k) % s (which
                    restores the input shape), read at the input rows, add the bias, zero the rows whose `nbr_t` row holds no valid entry;
                    autograd through it gives the gradients.  Run on absolute values it gives A, the scale of `sparse_conv_ref`'s bound.
* `inverse_tables`  the restated tables with the roles swapped, for `sparse_conv_ref.term_counts` / `sparse_oracle`.
* `pool_oracle`     densify with -inf fill in fp64, `F.max_pool3d`, read at `out_coors`.
* `pool_ref` / `unpool_ref`  the restatement over the tables: the maximum (a NaN wins), and the tie rule — every input equal to its window's
                    maximum receives grad_out — with the number of terms m and the sum of their magnitudes S of the backward's bound
                    |got - want| <= (m - 1) 2^-24 S.
* `POOL_BLOCK`, `POOL_MAX_BLOCKS`, `pool_rows`  the Python mirror of csrc/sparse_pool_common.h: the rows one workgroup covers.
* `synthetic_tables`  a random (nbr, nbr_t) pair with exactly R output and N input rows: per offset a partial injection outputs -> inputs.
"""
import numpy as np
import torch
import torch.nn.functional as F

import sparse_conv_ref as ref

POOL_BLOCK = 256            # threads of a workgroup (csrc/sparse_pool_common.h, BLOCK)
POOL_MAX_BLOCKS = 2048      # workgroups of a launch; the rows beyond are reached by striding over the grid (MAX_BLOCKS)
DTYPES = {'fp32': torch.float32, 'fp16': torch.float16, 'bf16': torch.bfloat16}
CODES = {'fp32': 0, 'fp16': 1, 'bf16': 2}
U16 = {'fp16': 2.0 ** -11, 'bf16': 2.0 ** -8}
SUB = {'fp16': 2.0 ** -25, 'bf16': 0.0}


def pool_rows(C, kind):
    """the rows one workgroup covers at a time (csrc/sparse_pool_common.h, lanes_of): BLOCK / (lanes per row)"""
    wide = 4 if kind == 'fp32' else 8
    return POOL_BLOCK // (C // wide if C % wide == 0 else C)


def rounded(a, kind):
    """an fp32 array after rounding to the kind's type, in fp64"""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DTYPES[kind]).double().numpy()


# ---- the inverse convolution -------------------------------------------------------------------------------------------------------------

def inverse_tables(idx):
    return dict(nbr=idx['nbr_t'], nbr_t=idx['nbr'])


def inverse_oracle(coors, shape, B, kernel, stride, padding, idx, X, W, bias, gY):
    """-> dict(out (N, Cout), gx (R, Cin), gw (K, Cin, Cout), gb) fp64.  X (R, Cin) on the rows of idx['out_coors'] (dead rows are left out)"""
    shape, kernel, stride, padding = ref.triple(shape), ref.triple(kernel), ref.triple(stride), ref.triple(padding)
    kept = np.nonzero((idx['out_coors'] >= 0).all(1))[0]
    oc = torch.from_numpy(idx['out_coors'][kept].astype(np.int64))
    x = torch.tensor(np.asarray(X, np.float64), requires_grad=True)
    w = torch.tensor(np.asarray(W, np.float64), requires_grad=True)
    b = None if bias is None else torch.tensor(np.asarray(bias, np.float64), requires_grad=True)
    dense = torch.zeros((B,) + tuple(idx['out_shape']) + (x.shape[1],), dtype=torch.float64)
    dense = dense.index_put((oc[:, 0], oc[:, 1], oc[:, 2], oc[:, 3]), x[torch.from_numpy(kept)]).permute(0, 4, 1, 2, 3)
    op = tuple((n + 2 * p - k) % s for n, k, s, p in zip(shape, kernel, stride, padding))
    y = F.conv_transpose3d(dense, w.reshape(*kernel, w.shape[1], w.shape[2]).permute(3, 4, 0, 1, 2), None, stride, padding, output_padding=op)
    assert tuple(y.shape[2:]) == shape, (y.shape, shape)
    has = (idx['nbr_t'] >= 0).any(1)
    c = torch.from_numpy(np.where(has[:, None], coors, 0).astype(np.int64))
    out = y[c[:, 0], :, c[:, 1], c[:, 2], c[:, 3]]
    if b is not None:
        out = out + b
    out = out * torch.from_numpy(has.astype(np.float64))[:, None]
    grads = torch.autograd.grad(out, [x, w] + ([] if b is None else [b]), torch.from_numpy(np.asarray(gY, np.float64)))
    return dict(out=out.detach().numpy(), gx=grads[0].numpy(), gw=grads[1].numpy(), gb=None if b is None else grads[2].numpy())


# ---- the max pooling -------------------------------------------------------------------------------------------------------------------

def pool_oracle(coors, shape, B, kernel, stride, padding, idx, X):
    """fp64: -inf-filled dense tensor, F.max_pool3d, read at out_coors; rows past the count are zero"""
    shape, kernel, stride, padding = ref.triple(shape), ref.triple(kernel), ref.triple(stride), ref.triple(padding)
    act = np.nonzero(ref.active_rows(np.asarray(coors), shape, B))[0]
    c = torch.from_numpy(np.asarray(coors)[act].astype(np.int64))
    x = torch.from_numpy(np.asarray(X, np.float64))
    dense = torch.full((B,) + shape + (x.shape[1],), -np.inf, dtype=torch.float64)
    dense[c[:, 0], c[:, 1], c[:, 2], c[:, 3]] = x[torch.from_numpy(act)]
    y = F.max_pool3d(dense.permute(0, 4, 1, 2, 3), kernel, stride, padding)
    live = (idx['out_coors'] >= 0).all(1)
    oc = torch.from_numpy(np.where(live[:, None], idx['out_coors'], 0).astype(np.int64))
    out = y[oc[:, 0], :, oc[:, 1], oc[:, 2], oc[:, 3]].numpy()
    return np.where(live[:, None], out, 0.0)


def pool_ref(idx, X):
    """the restatement over the table: the maximum over the valid entries (a NaN wins), zero for a row without one"""
    nbr, X = idx['nbr'], np.asarray(X, np.float64)
    if len(nbr) == 0 or len(X) == 0:
        return np.zeros((len(nbr), X.shape[1]))
    valid = nbr >= 0
    with np.errstate(invalid='ignore'):
        g = np.where(valid[:, :, None], X[np.maximum(nbr, 0)], -np.inf).max(1)
    return np.where(valid.any(1)[:, None], g, 0.0)


def unpool_ref(idx, X, out, gY):
    """the tie rule -> (gx, S, m): gx[i, c] = the sum over the offsets with o = nbr_t[i, j] valid and X[i, c] == out[o, c] of gY[o, c]"""
    nbr_t, X, out, gY = idx['nbr_t'], np.asarray(X, np.float64), np.asarray(out, np.float64), np.asarray(gY, np.float64)
    if len(nbr_t) == 0 or len(out) == 0:
        z = np.zeros(X.shape)
        return z, z, np.zeros(X.shape, np.int64)
    valid, o = nbr_t >= 0, np.maximum(nbr_t, 0)
    eq = valid[:, :, None] & (X[:, None, :] == out[o])
    terms = np.where(eq, gY[o], 0.0)
    return terms.sum(1), np.abs(terms).sum(1), eq.sum(1)


def within_pool_backward_bound(got, want, S, m, kind):
    """|got - want| <= E in fp32, E + u16 (|want| + E) + s on a 16-bit type, E = (m - 1) 2^-24 S -> (holds everywhere, worst error)"""
    err = np.abs(np.asarray(got, np.float64) - want)
    E = np.maximum(m - 1, 0) * ref.U * S
    bound = E if kind == 'fp32' else E + U16[kind] * (np.abs(want) + E) + SUB[kind]
    return bool((err <= bound).all()), float(err.max(initial=0.0))


def synthetic_tables(R, N, K, seed, fill=0.7):
    """(nbr (R, K), nbr_t (N, K)) int32 with N >= R: per offset a random partial injection of the outputs into the inputs"""
    assert N >= R
    rng = np.random.default_rng(seed)
    nbr, nbr_t = np.full((R, K), -1, np.int32), np.full((N, K), -1, np.int32)
    for j in range(K):
        o = np.nonzero(rng.random(R) < fill)[0]
        i = rng.permutation(N)[:R][o]
        nbr[o, j] = i
        nbr_t[i, j] = o
    return dict(nbr=nbr, nbr_t=nbr_t)
