"""numpy oracles of the point-in-rotated-box ops (tests/test_pib_cpu.py, tests/test_gpu_pib.py), in two forms.

(a) `inside_f32`: the contract of include/gd3d.h restated in np.float32, one correctly rounded ELEMENTWISE operation per step in
    the stated order, including the fixed-sequence sine / cosine polynomial (`fx_sincos`) operation by operation.  Comparisons of
    the library against it are EXACT.  `grid_points` (the RoI grid) is of this form too.
(b) `inside_f64` + `face_distance_f64`: an independent evaluation in fp64 with np.cos / np.sin, which shares neither the
    polynomial nor the operation order with the library: it guards against (a) and the kernel sharing one misreading.  It is
    compared on the (point, box) pairs whose fp64 distance to each of the six face planes is at least a margin.

Counts are assumed consistent with the arrays (clamping of inconsistent counts is a robustness property, not part of these
semantics).
"""
import numpy as np

F = np.float32


def _f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def fx_sincos(x):
    """The library's fixed-sequence sincos on an fp32 array: Cody-Waite reduction by pi/2 in three steps, two polynomials, quadrant
    selection.  Every line is one fp32 operation per element."""
    with np.errstate(all='ignore'):
        x = _f32(x)
        q = np.rint(x * F(0.63661977236758134))
        r = x - q * F(1.5703125)
        r = r - q * F(4.837512969970703125e-4)
        r = r - q * F(7.54978995489188216e-8)
        n = np.where(np.isfinite(q), q, 0).astype(np.int64) & 3
        z = r * r
        ps = F(-1.9515295891e-4) * z
        ps = ps + F(8.3321608736e-3)
        ps = ps * z
        ps = ps - F(1.6666654611e-1)
        ps = ps * z
        ps = ps * r
        ps = ps + r
        pc = F(2.443315711809948e-5) * z
        pc = pc - F(1.388731625493765e-3)
        pc = pc * z
        pc = pc + F(4.166664568298827e-2)
        pc = pc * z
        pc = pc * z
        pc = pc - F(0.5) * z
        pc = pc + F(1.0)
        s = np.where(n & 1, pc, ps)
        c = np.where(n & 1, ps, pc)
        s = np.where(n & 2, -s, s)
        c = np.where((n + 1) & 2, -c, c)
    assert s.dtype == np.float32 and c.dtype == np.float32
    return s, c


def enlarge(boxes, w):
    """mmdet3d's enlarged_box in fp32: z - w, every dim + 2 w"""
    b = _f32(boxes).copy()
    w = F(w)
    w2 = w * F(2.0)
    b[..., 2] = b[..., 2] - w
    b[..., 3:6] = b[..., 3:6] + w2
    return b


def inside_f32(points, boxes):
    """points (N, 3), boxes (T, 7) -> (N, T) bool, form (a)"""
    p, b = _f32(points).reshape(-1, 3), _f32(boxes).reshape(-1, 7)
    with np.errstate(all='ignore'):
        hz = b[:, 5] * F(0.5)
        czm = b[:, 2] + hz
        hx = b[:, 3] * F(0.5)
        hy = b[:, 4] * F(0.5)
        s, c = fx_sincos(-b[:, 6])
        in_z = np.abs(p[:, None, 2] - czm[None]) <= hz[None]
        sx = p[:, None, 0] - b[None, :, 0]
        sy = p[:, None, 1] - b[None, :, 1]
        lx = sx * c[None] + sy * (-s)[None]
        ly = sx * s[None] + sy * c[None]
        assert lx.dtype == np.float32
        return in_z & (lx > -hx[None]) & (lx < hx[None]) & (ly > -hy[None]) & (ly < hy[None])


def face_distance_f64(points, boxes):
    """(N, T) fp64: the smallest distance of the point to the six face PLANES of the box"""
    p, b = np.asarray(points, np.float64).reshape(-1, 3), np.asarray(boxes, np.float64).reshape(-1, 7)
    ang = -b[:, 6]
    sx, sy = p[:, None, 0] - b[None, :, 0], p[:, None, 1] - b[None, :, 1]
    lx = sx * np.cos(ang)[None] - sy * np.sin(ang)[None]
    ly = sx * np.sin(ang)[None] + sy * np.cos(ang)[None]
    lz = p[:, None, 2] - (b[:, 2] + b[:, 5] / 2)[None]
    d = [np.abs(np.abs(lx) - b[None, :, 3] / 2), np.abs(np.abs(ly) - b[None, :, 4] / 2), np.abs(np.abs(lz) - b[None, :, 5] / 2)]
    return np.minimum(np.minimum(d[0], d[1]), d[2]), (lx, ly, lz)


def inside_f64(points, boxes):
    """form (b): -> (inside (N, T) bool, distance to the nearest face plane (N, T))"""
    b = np.asarray(boxes, np.float64).reshape(-1, 7)
    dist, (lx, ly, lz) = face_distance_f64(points, boxes)
    inside = (np.abs(lz) <= b[None, :, 5] / 2) & (np.abs(lx) < b[None, :, 3] / 2) & (np.abs(ly) < b[None, :, 4] / 2)
    return inside, dist


def starts(cnt):
    cnt = np.asarray(cnt, dtype=np.int64)
    return np.concatenate(([0], np.cumsum(cnt)))


def all_stacked(xyz, pts_cnt, boxes, box_cnt=None):
    """-> (N, T) bool; columns t >= box_cnt[b] False"""
    xyz, boxes = _f32(xyz), _f32(boxes)
    st = starts(pts_cnt)
    t = boxes.shape[1]
    out = np.zeros((xyz.shape[0], t), bool)
    for b in range(len(pts_cnt)):
        tb = t if box_cnt is None else int(box_cnt[b])
        if tb and st[b + 1] > st[b]:
            out[st[b]:st[b + 1], :tb] = inside_f32(xyz[st[b]:st[b + 1]], boxes[b, :tb])
    return out


def first_of(flags):
    """(N, T) bool -> (N,) int32: the lowest set column, -1 if none"""
    if flags.shape[1] == 0:
        return np.full((flags.shape[0],), -1, np.int32)
    return np.where(flags.any(1), flags.argmax(1), -1).astype(np.int32)


def part_stacked(xyz, pts_cnt, boxes, box_cnt=None):
    return first_of(all_stacked(xyz, pts_cnt, boxes, box_cnt))


def mask_targets(xyz, pts_cnt, boxes, labels, box_cnt, extra_width, num_classes):
    """-> (seg (N,) int64, box_idx (N,) int32)"""
    i = part_stacked(xyz, pts_cnt, boxes, box_cnt)
    e = part_stacked(xyz, pts_cnt, enlarge(boxes, extra_width), box_cnt)
    sample = np.repeat(np.arange(len(pts_cnt)), np.asarray(pts_cnt, dtype=np.int64))
    labels = np.asarray(labels, np.int64)
    seg = np.full(i.shape, num_classes, np.int64)
    hit = i >= 0
    seg[hit] = labels[sample[hit], i[hit]]
    seg[hit != (e >= 0)] = -1
    return seg, i


def grid_points(rois, g, clockwise=False):
    """rois (R, 7) -> (R, G^3, 3) fp32, one fp32 operation per step"""
    r = _f32(rois).reshape(-1, 7)
    gf = F(g)
    idx = np.arange(g, dtype=np.float32)
    frac = (idx + F(0.5)) / gf                      # (i + 0.5f) / G, correctly rounded
    cen = frac - F(0.5)
    i, j, k = np.meshgrid(np.arange(g), np.arange(g), np.arange(g), indexing='ij')
    i, j, k = i.reshape(-1), j.reshape(-1), k.reshape(-1)        # k fastest
    s, c = fx_sincos(r[:, 6])
    lx = cen[i][None] * r[:, 3:4]
    ly = cen[j][None] * r[:, 4:5]
    lz = frac[k][None] * r[:, 5:6]
    s, c = s[:, None], c[:, None]
    if clockwise:
        x = lx * c + ly * s
        y = ly * c - lx * s
    else:
        x = lx * c - ly * s
        y = lx * s + ly * c
    out = np.stack((x + r[:, 0:1], y + r[:, 1:2], lz + r[:, 2:3]), -1)
    assert out.dtype == np.float32
    return out.reshape(r.shape[0], g ** 3, 3)
