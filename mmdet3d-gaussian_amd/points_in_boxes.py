"""Point-in-rotated-box ops, PV-RCNN's keypoint segmentation targets and the dense RoI grid points, on top of the HIP kernels of
csrc/pib.hip (include/gd3d.h, gd3d_pib_*, gd3d_roi_grid_points).

  * `points_in_boxes_part` / `points_in_boxes_all` — the call surface of mmdet3d 1.0's roiaware_pool3d ops (third party, CUDA only),
    which the reference reaches for in models/roi_heads/mask_heads/pointwise_mask_head.py:62-92 and
    core/bbox/assigners/sim_ota_3d_assigner.py:158-182; `*_stacked` are the same ops on stacked points.
  * `pointwise_mask_targets` — `PointwiseMaskHead.get_targets` for the whole batch in ONE launch (the reference: a Python loop over
    the samples with two `points_in_boxes_part` calls, a pad, a gather and an xor each).
  * `roi_grid_points` / `roi_grid_queries` — `Batch3DRoIGridExtractor.get_dense_grid_points`
    (models/roi_heads/roi_extractors/batch_roigrid_extractor.py:56-71) and the (new_xyz, new_xyz_batch_cnt) pair its forward
    (:27-42) hands to `QueryAndGroup`, without the per-sample host reads.

A box is [x, y, z, dx, dy, dz, rz] with (x, y, z) the BOTTOM centre.  A point is inside when, in fp32 and one operation per step,
|pz - (z + dz/2)| <= dz/2 (z faces inclusive) and its offset from (x, y) turned by -rz lies STRICTLY inside (-dx/2, dx/2) x (-dy/2, dy/2).
So a zero or negative dx or dy, or a negative dz, contains nothing (zero-padded box rows are harmless), and a point with a NaN
coordinate is in no box.

Conventions as in `vsa.py`: CUDA tensors go to the kernels on the current stream, CPU tensors to the library's `_cpu` twins
(bit-identical results); non-fp32 floats are evaluated in fp32; no wrapper reads a value back from the device, so every op can be
captured in a hipGraph (the counts are clamped inside the kernels instead of validated on the host); shape and dtype errors raise
RuntimeError.  Nothing here is differentiable (the reference's versions are not either).
"""
import torch

from ._host import call as _call, counts_i32 as _cnt32, ptr_or_null as _ptr, rows_f32 as _rows

BOX_TILE = 256            # boxes a workgroup holds in LDS at a time (gd3d_pib_box_tile())
WORKGROUP_POINTS = 256    # points of one sample a workgroup owns (gd3d_pib_workgroup_points())
MAX_GRID_SIZE = 16


def _boxes(boxes, like, name='boxes'):
    if boxes.dim() != 3 or boxes.size(2) < 7 or not boxes.dtype.is_floating_point:
        raise RuntimeError(f'shape mismatch: {name} must be a floating-point (B, T, 7) tensor, got {boxes.dtype} {tuple(boxes.shape)}')
    if boxes.device != like.device:
        raise RuntimeError(f'{name} is on {boxes.device}, the points on {like.device}')
    return boxes.detach()[..., :7].to(torch.float32).contiguous()


def _stacked_args(xyz, xyz_batch_cnt, boxes, box_cnt):
    x = _rows(xyz, 3, 'xyz')
    xc = _cnt32(xyz_batch_cnt, x, 'xyz_batch_cnt')
    bx = _boxes(boxes, x)
    if bx.size(0) != xc.numel():
        raise RuntimeError(f'shape mismatch: boxes has {bx.size(0)} samples, xyz_batch_cnt {xc.numel()}')
    bc = None
    if box_cnt is not None:
        bc = _cnt32(box_cnt, x, 'box_cnt')
        if bc.numel() != xc.numel():
            raise RuntimeError(f'shape mismatch: box_cnt has {bc.numel()} samples, xyz_batch_cnt {xc.numel()}')
    return x, xc, bx, bc


def points_in_boxes_part_stacked(xyz, xyz_batch_cnt, boxes, box_cnt=None):
    """xyz (N1+N2+..., 3), xyz_batch_cnt (B,), boxes (B, T, 7), box_cnt (B,) or None -> box_idx (N,) int32: the LOWEST index of a
    box of the point's own sample that contains it, -1 if none.  Rows t >= box_cnt[b] of sample b are ignored (None: all T)."""
    x, xc, bx, bc = _stacked_args(xyz, xyz_batch_cnt, boxes, box_cnt)
    out = torch.empty((x.size(0),), dtype=torch.int32, device=x.device)
    if x.size(0) > 0:
        _call('gd3d_pib_part', x.device, (_ptr(x), _ptr(xc), _ptr(bx), _ptr(bc), xc.numel(), x.size(0), bx.size(1), _ptr(out)), (0,))
    return out


def points_in_boxes_all_stacked(xyz, xyz_batch_cnt, boxes, box_cnt=None, dtype=torch.bool):
    """-> flags (N, T) of `dtype` torch.bool (one byte per flag, what a mask consumer wants) or torch.int32 (what mmdet3d's op
    returns): flags[n, t] = point n lies in box t of its sample.  Columns t >= box_cnt[b] are 0; every element is written."""
    if dtype not in (torch.bool, torch.uint8, torch.int32):
        raise RuntimeError(f'dtype must be torch.bool, torch.uint8 or torch.int32, got {dtype}')
    x, xc, bx, bc = _stacked_args(xyz, xyz_batch_cnt, boxes, box_cnt)
    out = torch.empty((x.size(0), bx.size(1)), dtype=dtype, device=x.device)
    if out.numel() > 0:
        _call('gd3d_pib_all', x.device, (_ptr(x), _ptr(xc), _ptr(bx), _ptr(bc), xc.numel(), x.size(0), bx.size(1), _ptr(out),
                                         4 if dtype == torch.int32 else 1), (0,))
    return out


def _batched(points, boxes):
    if points.dim() != 3 or points.size(2) != 3 or not points.dtype.is_floating_point:
        raise RuntimeError(f'shape mismatch: points must be a floating-point (B, N, 3) tensor, got {points.dtype} {tuple(points.shape)}')
    if boxes.dim() != 3 or boxes.size(0) != points.size(0):
        raise RuntimeError(f'shape mismatch: boxes must be (B, T, 7) with B = {points.size(0)}, got {tuple(boxes.shape)}')
    b, n = points.size(0), points.size(1)
    return points.reshape(b * n, 3), torch.full((b,), n, dtype=torch.int32, device=points.device), b, n


def points_in_boxes_part(points, boxes):
    """mmdet3d's `points_in_boxes_part`: points (B, N, 3), boxes (B, T, 7) -> (B, N) int32, the lowest index of a box that contains
    the point, -1 if none."""
    xyz, cnt, b, n = _batched(points, boxes)
    return points_in_boxes_part_stacked(xyz, cnt, boxes).reshape(b, n)


def points_in_boxes_all(points, boxes):
    """mmdet3d's `points_in_boxes_all`: points (B, N, 3), boxes (B, T, 7) -> (B, N, T) int32 flags."""
    xyz, cnt, b, n = _batched(points, boxes)
    return points_in_boxes_all_stacked(xyz, cnt, boxes, dtype=torch.int32).reshape(b, n, boxes.size(1))


def _pad_samples(gt_boxes, gt_labels, dev):
    """per-sample lists -> (B, T, 7) boxes, (B, T) labels, (B,) box counts, padded on the device"""
    if len(gt_boxes) != len(gt_labels):
        raise RuntimeError(f'shape mismatch: {len(gt_boxes)} samples of gt_boxes, {len(gt_labels)} of gt_labels')
    for bx, lb in zip(gt_boxes, gt_labels):
        if bx.dim() != 2 or bx.size(1) < 7 or lb.dim() != 1 or lb.size(0) != bx.size(0):
            raise RuntimeError(f'shape mismatch: a sample needs gt_boxes (T, 7) and gt_labels (T,), got {tuple(bx.shape)} and {tuple(lb.shape)}')
    b = len(gt_boxes)
    t = max([bx.size(0) for bx in gt_boxes], default=0)
    boxes = torch.zeros((b, t, 7), dtype=torch.float32, device=dev)
    labels = torch.zeros((b, t), dtype=torch.int64, device=dev)
    for i, (bx, lb) in enumerate(zip(gt_boxes, gt_labels)):
        boxes[i, :bx.size(0)] = bx[:, :7]
        labels[i, :bx.size(0)] = lb
    cnt = torch.tensor([bx.size(0) for bx in gt_boxes], dtype=torch.int32).to(dev)   # sizes are host data: no read back
    return boxes, labels, cnt


def pointwise_mask_targets(xyz, xyz_batch_cnt, gt_boxes, gt_labels, extra_width, num_classes, return_box_idx=False, box_cnt=None):
    """`PointwiseMaskHead.get_targets` for the whole batch in one launch -> seg_targets (N,) int64 (and box_idx (N,) int32 with
    `return_box_idx`): per point, i = the first of its sample's gt boxes that contains it and e = the first of the boxes enlarged by
    `extra_width` (z - w, every dim + 2 w) that does; seg = gt_labels[b, i] if i >= 0 else num_classes (background), and -1
    (ignore) where (i >= 0) != (e >= 0) — the reference's xor, so a negative `extra_width` behaves as there.

    xyz (N, 3) with xyz_batch_cnt (B,), or the reference's points_bxyz (N, 4) = [sample id, x, y, z] with xyz_batch_cnt=None
    (rows grouped by ascending sample id, as the reference's per-sample slicing yields them; counted on the device).
    gt_boxes / gt_labels: per-sample lists of (T_b, 7) / (T_b,) tensors, padded here on the device (the list form copies the T_b
    from the host, so capture the padded form), or already padded (B, T, 7) / (B, T) with an optional `box_cnt` (B,)."""
    if isinstance(gt_boxes, (list, tuple)):
        boxes, labels, box_cnt = _pad_samples(gt_boxes, gt_labels, xyz.device)
    else:
        boxes, labels = gt_boxes, gt_labels
    if xyz_batch_cnt is None:
        if xyz.dim() != 2 or xyz.size(1) != 4:
            raise RuntimeError(f'shape mismatch: without xyz_batch_cnt the points must be (N, 4) [sample id, x, y, z], got {tuple(xyz.shape)}')
        ids = xyz[:, 0].long()
        xyz_batch_cnt = (ids[:, None] == torch.arange(boxes.size(0), device=xyz.device)[None, :]).sum(0).to(torch.int32)
        xyz = xyz[:, 1:]
    x, xc, bx, bc = _stacked_args(xyz, xyz_batch_cnt, boxes, box_cnt)
    if labels.shape != bx.shape[:2] or labels.dtype.is_floating_point or labels.dtype == torch.bool:
        raise RuntimeError(f'shape mismatch: gt_labels must be an integer {tuple(bx.shape[:2])} tensor, got {labels.dtype} {tuple(labels.shape)}')
    if labels.device != x.device:
        raise RuntimeError(f'gt_labels is on {labels.device}, the points on {x.device}')
    lb = labels.to(torch.int64).contiguous()
    seg = torch.empty((x.size(0),), dtype=torch.int64, device=x.device)
    idx = torch.empty((x.size(0),), dtype=torch.int32, device=x.device) if return_box_idx else None
    if x.size(0) > 0:
        _call('gd3d_pib_mask_targets', x.device,
              (_ptr(x), _ptr(xc), _ptr(bx), _ptr(lb), _ptr(bc), xc.numel(), x.size(0), bx.size(1),
               float(extra_width), int(num_classes), _ptr(seg), _ptr(idx)), (0,))
    return (seg, idx) if return_box_idx else seg


def _check_grid(grid_size):
    grid_size = int(grid_size)
    if not 1 <= grid_size <= MAX_GRID_SIZE:
        raise RuntimeError(f'grid_size must be in [1, {MAX_GRID_SIZE}], got {grid_size}')
    return grid_size


def _grid_points(rows, first, grid_size, clockwise):
    g = _check_grid(grid_size)
    r = rows.detach().to(torch.float32).contiguous()
    out = torch.empty((r.size(0), g ** 3, 3), dtype=torch.float32, device=r.device)
    if r.size(0) > 0:
        _call('gd3d_roi_grid_points', r.device, (_ptr(r), r.size(1), first, r.size(0), g, 1 if clockwise else 0, _ptr(out)), (0,))
    return out.to(rows.dtype)


def roi_grid_points(rois, grid_size=6, clockwise=False):
    """rois (R, 7) [x, y, z, dx, dy, dz, rz] -> (R, G^3, 3): the centres of the G x G x G cells of every RoI, point (i, j, k) with k
    fastest (the order `nonzero()` yields in the reference): ((i + .5)/G - .5) dx, ((j + .5)/G - .5) dy, ((k + .5)/G) dz, turned
    about z by rz and moved to (x, y, z).  The rotation has the sense and the `clockwise` flag of the RoI decode
    (`PVRCNNBboxHead`): counter-clockwise (mmdet3d 1.0) by default."""
    if rois.dim() != 2 or rois.size(1) != 7 or not rois.dtype.is_floating_point:
        raise RuntimeError(f'shape mismatch: rois must be a floating-point (R, 7) tensor, got {rois.dtype} {tuple(rois.shape)}')
    return _grid_points(rois, 0, grid_size, clockwise)


def roi_grid_queries(rois, batch_size, grid_size=6, clockwise=False):
    """rois (R, 8) [sample id, x, y, z, dx, dy, dz, rz] -> (new_xyz (R * G^3, 3), new_xyz_batch_cnt (batch_size,) int32): the pair
    `QueryAndGroup` takes as its queries.  The RoIs must be grouped by ascending sample id, as the reference assumes (it slices
    them per sample); the counts are made on the device, without a host read."""
    if rois.dim() != 2 or rois.size(1) != 8 or not rois.dtype.is_floating_point:
        raise RuntimeError(f'shape mismatch: rois must be a floating-point (R, 8) tensor, got {rois.dtype} {tuple(rois.shape)}')
    batch_size = int(batch_size)
    if batch_size < 0:
        raise RuntimeError(f'batch_size must not be negative, got {batch_size}')
    pts = _grid_points(rois, 1, grid_size, clockwise)
    ids = rois[:, 0].long()
    per_sample = (ids[:, None] == torch.arange(batch_size, device=rois.device)[None, :]).sum(0)
    return pts.reshape(-1, 3), (per_sample * int(grid_size) ** 3).to(torch.int32)
