"""numpy restatement of the serial semantics of the voxel-set-abstraction ops (stacked ball query, grouping, QueryAndGroup,
furthest point sampling) — the oracle of tests/test_vsa_cpu.py and tests/test_gpu_vsa.py.

Every decision is made with fp32 ELEMENTWISE numpy operations in the stated order, (dx*dx + dy*dy) + dz*dz with dx = nx - x;
each is correctly rounded, so `d2 < radius2` and the arg max are exact statements of the contract, not approximations of it.
Sums (the backward) are taken in fp64.  Counts are assumed consistent with the arrays (the kernels' clamping of inconsistent
counts is a robustness property, not part of these semantics).
"""
import numpy as np


def _f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def starts(cnt):
    cnt = np.asarray(cnt, dtype=np.int64)
    return np.concatenate(([0], np.cumsum(cnt)))[:-1]


def sample_of_rows(cnt):
    """(rows,) sample id of every stacked row"""
    return np.repeat(np.arange(len(cnt)), np.asarray(cnt, dtype=np.int64))


def has_points(features_cnt, idx_cnt):
    """(rows,) bool: the row's sample has at least one point"""
    return (np.asarray(features_cnt, dtype=np.int64) > 0)[sample_of_rows(idx_cnt)]


def dist2(c, pts):
    """fp32: (cx-x)*(cx-x) + (cy-y)*(cy-y) + (cz-z)*(cz-z), left to right"""
    c = _f32(c)
    pts = _f32(pts).reshape(-1, 3)
    dx, dy, dz = c[0] - pts[:, 0], c[1] - pts[:, 1], c[2] - pts[:, 2]
    return (dx * dx + dy * dy) + dz * dz


def ball_query(radius, nsample, xyz, xyz_cnt, new_xyz, new_cnt):
    """-> idx (M, nsample) int32, cnt (M,) int32 (clipped to nsample), empty mask (M,) bool"""
    xyz, new_xyz = _f32(xyz).reshape(-1, 3), _f32(new_xyz).reshape(-1, 3)
    r2 = np.float32(radius) * np.float32(radius)
    m = new_xyz.shape[0]
    idx = np.zeros((m, nsample), np.int32)
    cnt = np.zeros((m,), np.int32)
    ps, qb = starts(xyz_cnt), sample_of_rows(new_cnt)
    for q in range(m):
        b = qb[q]
        pts = xyz[ps[b]:ps[b] + int(xyz_cnt[b])]
        members = np.nonzero(dist2(new_xyz[q], pts) < r2)[0][:nsample]
        k = len(members)
        cnt[q] = k
        if k:
            idx[q, :k] = members
            idx[q, k:] = members[0]
    return idx, cnt, cnt == 0


def grouping(features, features_cnt, idx, idx_cnt):
    """out[m, c, s] = features[start_b + idx[m, s], c] -> (M, C, nsample); a sample without points has no row to name: zeros"""
    features = np.asarray(features)
    rows = starts(features_cnt)[sample_of_rows(idx_cnt)][:, None] + np.asarray(idx, dtype=np.int64)      # (M, nsample) global rows
    has = has_points(features_cnt, idx_cnt)
    out = np.zeros((rows.shape[0], features.shape[1], rows.shape[1]), features.dtype)
    out[has] = features[rows[has]].transpose(0, 2, 1)
    return out


def grouping_backward(grad_out, idx, idx_cnt, features_cnt, n, live=None):
    """fp64 grad_features (n, C), and per element the number of contributions and the sum of their magnitudes (what the
    rounding bound of an fp32 sum in any order is made of).  `live` (M,) bool: rows that pass a gradient (default all); the rows
    of a sample without points never do."""
    g = np.asarray(grad_out, dtype=np.float64)                     # (M, C, nsample)
    m, c, ns = g.shape
    rows = starts(features_cnt)[sample_of_rows(idx_cnt)][:, None] + np.asarray(idx, dtype=np.int64)
    if live is None:
        live = np.ones((m,), bool)
    live = live & has_points(features_cnt, idx_cnt)
    rows, g = rows[live], g[live]
    grad = np.zeros((n, c))
    mag = np.zeros((n, c))
    num = np.zeros((n,), np.int64)
    flat = rows.reshape(-1)
    contrib = g.transpose(0, 2, 1).reshape(-1, c)                  # one row of C per (m, s)
    np.add.at(grad, flat, contrib)
    np.add.at(mag, flat, np.abs(contrib))
    np.add.at(num, flat, 1)
    return grad, num, mag


def query_and_group(radius, nsample, xyz, xyz_cnt, new_xyz, new_cnt, features=None, use_xyz=True):
    """-> new_features (M, 3 + C, nsample) fp32, idx, cnt, mask"""
    assert features is not None or use_xyz
    xyz, new_xyz = _f32(xyz).reshape(-1, 3), _f32(new_xyz).reshape(-1, 3)
    idx, cnt, mask = ball_query(radius, nsample, xyz, xyz_cnt, new_xyz, new_cnt)
    parts = []
    if use_xyz:
        parts.append(grouping(xyz, xyz_cnt, idx, new_cnt) - new_xyz[:, :, None])      # fp32 subtraction
    if features is not None:
        parts.append(grouping(_f32(features), xyz_cnt, idx, new_cnt))
    out = np.concatenate(parts, axis=1).astype(np.float32)
    out[mask] = 0
    return out, idx, cnt, mask


def fps(xyz, npoint, trace=None):
    """one sample (n, 3) -> (npoint,) int64: pick 0 is index 0, then the arg max of the running min of the squared distances to
    all earlier picks, the lowest index on exactly equal distances (np.argmax returns the first); n < npoint: the n picks
    cyclically; n == 0: zeros.  `trace(p, t)` is called with the running minima from which pick p is about to be taken."""
    xyz = _f32(xyz).reshape(-1, 3)
    n = xyz.shape[0]
    out = np.zeros((npoint,), np.int64)
    if n == 0 or npoint == 0:
        return out
    t = np.full((n,), 1e10, np.float32)
    picks = min(n, npoint)
    old = 0
    x, y, z = (np.ascontiguousarray(xyz[:, k]) for k in range(3))   # dist2's arithmetic on contiguous columns, in place
    dx, dy, dz = (np.empty((n,), np.float32) for _ in range(3))
    for p in range(1, picks):
        np.subtract(x[old], x, out=dx)
        np.subtract(y[old], y, out=dy)
        np.subtract(z[old], z, out=dz)
        np.multiply(dx, dx, out=dx)
        np.multiply(dy, dy, out=dy)
        np.multiply(dz, dz, out=dz)
        np.add(dx, dy, out=dx)
        np.add(dx, dz, out=dx)                                      # (dx * dx + dy * dy) + dz * dz
        np.copyto(t, dx, where=dx < t)                              # d < t ? d : t
        if trace is not None:
            trace(p, t)
        old = int(np.argmax(t))
        out[p] = old
    for j in range(picks, npoint):
        out[j] = out[j % n]
    return out


def fps_stacked(xyz, xyz_cnt, npoint):
    xyz = _f32(xyz).reshape(-1, 3)
    ps = starts(xyz_cnt)
    return np.stack([fps(xyz[ps[b]:ps[b] + int(xyz_cnt[b])], npoint) for b in range(len(xyz_cnt))]) if len(xyz_cnt) else \
        np.zeros((0, npoint), np.int64)
