"""numpy restatement of the voxel query ops (include/gd3d.h, gd3d_vsa_voxel_*): the loops as the header states them, elementwise fp32
in the stated order (numpy rounds every float32 operation on its own: no fma).  Independent of the library: nothing here imports it.
"""
import numpy as np

F = np.float32


def cell_keys(coors, shape, B):
    """coors (N, 4) [b, z, y, x] -> int64 keys ((b*Z + z)*Y + y)*X + x; B*Z*Y*X for a row with any coordinate outside the grid."""
    Z, Y, X = shape
    c = np.asarray(coors).astype(np.int64).reshape(-1, 4)
    ok = (c[:, 0] >= 0) & (c[:, 0] < B) & (c[:, 1] >= 0) & (c[:, 1] < Z) & (c[:, 2] >= 0) & (c[:, 2] < Y) & (c[:, 3] >= 0) & (c[:, 3] < X)
    key = ((c[:, 0] * Z + c[:, 1]) * Y + c[:, 2]) * X + c[:, 3]
    return np.where(ok, key, np.int64(B) * Z * Y * X)


def index_ref(coors, shape, B):
    """-> skey (N,) int64 ascending, srow (N,) int32: the stable sort of the keys."""
    key = cell_keys(coors, shape, B)
    srow = np.argsort(key, kind='stable')
    return key[srow], srow.astype(np.int32)


def table_ref(coors, shape, B):
    """-> (B, Z, Y, X) int32: the LOWEST row of every cell, -1 where there is none."""
    Z, Y, X = shape
    key = cell_keys(coors, shape, B)
    table = np.full(B * Z * Y * X, -1, dtype=np.int32)
    for i in range(len(key) - 1, -1, -1):        # descending: the lowest row is written last
        if key[i] < table.size:
            table[key[i]] = i
    return table.reshape(B, Z, Y, X)


def coords_ref(new_xyz, counts, voxel_size, pc_range, scale):
    """-> (M, 4) int32 [b, z, y, x]: per axis floor((p - lo) / (voxel_size * scale)) in fp32; b from the (clamped) counts."""
    q = np.asarray(new_xyz, dtype=F).reshape(-1, 3)
    M = q.shape[0]
    out = np.zeros((M, 4), dtype=np.int32)
    b = np.full(M, -1, dtype=np.int32)
    start = 0
    for k, c in enumerate(counts):
        n = min(max(int(c), 0), M - start)
        b[start:start + n] = k
        start += n
    ok = np.ones(M, dtype=bool)
    with np.errstate(all='ignore'):
        for axis in range(3):                    # x, y, z -> columns 3, 2, 1
            vsl = F(float(voxel_size[axis]) * float(scale))
            f = np.floor((q[:, axis] - F(pc_range[axis])) / vsl)
            good = (f >= F(-2.0 ** 30)) & (f < F(2.0 ** 30))
            out[:, 3 - axis] = np.where(good, f, F(0)).astype(np.int32)
            ok &= good
    out[:, 0] = np.where(ok, b, -1)
    return out


def window(max_range):
    """-> (cells, 3) int64 offsets (dz, dy, dx) in window order: dz slowest, dx fastest, each ascending."""
    rz, ry, rx = max_range
    dz, dy, dx = np.meshgrid(np.arange(-rz, rz + 1), np.arange(-ry, ry + 1), np.arange(-rx, rx + 1), indexing='ij')
    return np.stack([dz.ravel(), dy.ravel(), dx.ravel()], axis=1).astype(np.int64)


def query_ref(xyz, new_xyz, new_coords, table, max_range, radius, nsample):
    """-> dict(idx (M, nsample) int32, cnt (M,) int32, mask (M,) bool, members (M,) uncapped member counts, pos_cell / pos_row (M,) the
    window cell / window row that holds the nsample-th member (-1: fewer members)).  `table` (B, Z, Y, X): the cells' rows, any int."""
    xyz = np.asarray(xyz, dtype=F).reshape(-1, 3)
    q = np.asarray(new_xyz, dtype=F).reshape(-1, 3)
    nc = np.asarray(new_coords).astype(np.int64).reshape(-1, 4)
    B, Z, Y, X = table.shape
    N, M = xyz.shape[0], q.shape[0]
    flat = table.reshape(-1).astype(np.int64)
    off = window(max_range)
    nx = 2 * max_range[2] + 1
    r2 = F(radius) * F(radius)
    idx = np.zeros((M, nsample), dtype=np.int32)
    cnt = np.zeros(M, dtype=np.int32)
    members = np.zeros(M, dtype=np.int64)
    pos_cell = np.full(M, -1, dtype=np.int64)
    for m in range(M):
        b = nc[m, 0]
        if b < 0 or b >= B:
            continue
        cell = nc[m, 1:] + off
        ok = (cell[:, 0] >= 0) & (cell[:, 0] < Z) & (cell[:, 1] >= 0) & (cell[:, 1] < Y) & (cell[:, 2] >= 0) & (cell[:, 2] < X)
        j = np.nonzero(ok)[0]
        rows = flat[((b * Z + cell[j, 0]) * Y + cell[j, 1]) * X + cell[j, 2]]
        live = (rows >= 0) & (rows < N)
        j, rows = j[live], rows[live]
        p = xyz[rows]
        with np.errstate(all='ignore'):
            dx, dy, dz = q[m, 0] - p[:, 0], q[m, 1] - p[:, 1], q[m, 2] - p[:, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            inside = d2 <= r2                      # inclusive; NaN compares false
        j, rows = j[inside], rows[inside]
        members[m] = len(rows)
        k = min(len(rows), nsample)
        cnt[m] = k
        if k > 0:
            idx[m, :k] = rows[:k]
            idx[m, k:] = rows[0]
        if len(rows) >= nsample:
            pos_cell[m] = j[nsample - 1]
    return dict(idx=idx, cnt=cnt, mask=cnt == 0, members=members, pos_cell=pos_cell, pos_row=np.where(pos_cell >= 0, pos_cell // nx, -1))


def group_ref(xyz, new_xyz, features, idx, cnt, use_xyz):
    """-> (M, (3 if use_xyz) + C, nsample) fp32: grouped xyz minus the centre, then the features; empty queries all zero."""
    xyz = np.asarray(xyz, dtype=F).reshape(-1, 3)
    q = np.asarray(new_xyz, dtype=F).reshape(-1, 3)
    parts = []
    with np.errstate(all='ignore'):
        if use_xyz:
            parts.append(np.transpose(xyz[idx] - q[:, None, :], (0, 2, 1)))          # (M, 3, nsample): ONE fp32 subtraction
        if features is not None:
            parts.append(np.transpose(np.asarray(features, dtype=F)[idx], (0, 2, 1)))
    out = np.concatenate(parts, axis=1).astype(F)
    out[np.asarray(cnt) == 0] = 0
    return out


def backward_ref(grad_out, idx, cnt, N, C, c_off):
    """fp64 sums of grad_out (M, c_off + C, nsample) into (N, C), with per element the number of contributions k and sum |terms|."""
    g = np.asarray(grad_out, dtype=np.float64)[:, c_off:c_off + C, :]
    M, _, nsample = g.shape
    total = np.zeros((N, C))
    mag = np.zeros((N, C))
    k = np.zeros((N, C), dtype=np.int64)
    for m in range(M):
        if cnt[m] <= 0:
            continue
        for s in range(nsample):
            total[idx[m, s]] += g[m, :, s]
            mag[idx[m, s]] += np.abs(g[m, :, s])
            k[idx[m, s]] += 1
    return total, mag, k
