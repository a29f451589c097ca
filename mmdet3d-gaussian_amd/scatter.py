"""Dynamic point-to-voxel scatter ops — the call surface of /root/reference/mmdet3d_gaussian/ops/voxel/scatter.py
(`scatter_index` :10-26, `scatter_reduce` :29-72, `Scatter` :75-144) on top of the HIP kernels of
csrc/voxel_scatter.hip.

The reference indexes with masked_fill + unique_dim per SAMPLE (src/scatter_points_cuda.cu:221-251, scatter.py:101-117).
Here one mixed-radix int64 key per point, one stable sort and one unique_consecutive index the whole batch and produce
the by-voxel grouping of the points that the atomic-free reduce / backward kernels walk; nothing reads a value back to
the host (`_index_and_grouping`).  `scatter_reduce` keeps the reference's signature.
"""
import torch

from . import _host, _lib

REDUCE = {'sum': 0, 'mean': 1, 'max': 2}  # reduce_t, src/voxelization.h:4


def _index_and_grouping(coors):
    """From point coordinates to everything the scatter ops need, batched or not: ONE library call (vox_index_build:
    per-column extents, a mixed-radix int64 key per point, a stable radix sort of (key, point id), run heads -> voxel ids
    -> map / segments / counts / decoded voxel rows, csrc/voxel_index.hip) and ONE host read of two integers — the
    number of voxels is data dependent, as in the reference's unique_dim.  Round 2 did the same with ~20 ATen launches
    (`_index_and_grouping_torch` below, kept as the statement the tests compare against)."""
    n, ndim = coors.shape
    if not coors.is_cuda:
        raise RuntimeError('scatter_index: the MI355X implementation has no CPU path (neither has the reference: '
                           'voxelization.h:46)')
    if ndim > 8 or n >= 2 ** 31:
        return _index_and_grouping_torch(coors)     # beyond the kernels' limits: the same result from device-side ATen ops
    dev = coors.device
    lib = _lib.load()
    over = None
    if coors.dtype == torch.int32:
        c32 = coors
    else:
        # wider integers: anything negative is a dropped point whatever its size (clamped to -1 before the cast); a value beyond
        # int32 cannot be a coordinate of this index (int32 coordinates, as the reference's op) and is reported, not wrapped
        over = (coors > 2147483647).any()
        c32 = coors.clamp(min=-1).to(torch.int32)
    c32 = c32.contiguous()
    pmap = torch.empty(n, dtype=torch.int32, device=dev)
    order = torch.empty(n, dtype=torch.int32, device=dev)
    seg = torch.empty(n + 1, dtype=torch.int32, device=dev)
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    vcoors = torch.empty((n, ndim), dtype=torch.int32, device=dev)
    num = torch.empty(2, dtype=torch.int64, device=dev)
    nbytes = lib.vox_index_workspace_bytes(n, ndim)
    if nbytes == 0:
        raise RuntimeError('vox_index_workspace_bytes failed (no usable device for the sort-size query)')
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    with _host.on_device(dev) as stream:
        rc = lib.vox_index_build(c32.data_ptr(), n, ndim, ws.data_ptr(), pmap.data_ptr(), order.data_ptr(), seg.data_ptr(),
                                 counts.data_ptr(), vcoors.data_ptr(), num.data_ptr(), stream)
    _lib.check(rc, 'vox_index_build')
    if over is None:
        v = int(num[0].item())                                                 # the one wait: V sizes every output
    else:
        v, bad = torch.stack((num[0], over.to(torch.int64))).tolist()          # still one wait
        if bad:
            raise RuntimeError('scatter_index: a coordinate exceeds the int32 range')
    if v < 0:
        raise RuntimeError('scatter_index: the product of the per-column extents does not fit a 63-bit voxel key')
    voxel_coors = vcoors[:v]
    if coors.dtype != torch.int32:
        voxel_coors = voxel_coors.to(coors.dtype)
    return voxel_coors, pmap, counts[:v], (order, seg[:v + 1])


def _index_and_grouping_torch(coors):
    """One pass from point coordinates to everything the scatter ops need, batched or not, without a per-sample loop
    and without a host read of any VALUE (the only wait is the one inside torch.unique_consecutive: the number of
    voxels is data dependent).

    A point row (any number of integer columns; a leading batch column is just one more) becomes ONE int64 key, mixed
    radix over the per-column extents taken on the device; a row with a negative entry gets key -1 (dropped point,
    scatter_points_cuda.cu:236-246).  A stable sort of the keys is at once
      * the order of the voxels: ascending keys = lexicographically sorted unique rows = what the reference's
        unique_dim yields per sample, samples in batch order (ops/voxel/scatter.py:101-117);
      * the grouping of the points by voxel in ascending point id that the atomic-free kernels walk (`order`, `seg`).
    A sentinel key -1 is put in front so that the dropped-points bucket always exists and can be cut off without asking
    the device whether it is there."""
    n, ndim = coors.shape
    dev = coors.device
    c64 = coors.to(torch.int64)
    ext = c64.amax(0).clamp_(min=0).add_(1)                                   # (ndim,) per-column extent, on the device
    stride = torch.ones(ndim, dtype=torch.int64, device=dev)
    if ndim > 1:
        stride[:-1] = ext[1:].flip(0).cumprod(0).flip(0)
    key = (c64 * stride).sum(-1)
    key = torch.where((c64 < 0).any(-1), key.new_full((), -1), key)
    key = torch.cat((key.new_full((1,), -1), key))                            # sentinel FIRST: bucket 0 = dropped points
    skey, order = torch.sort(key, stable=True)                                # order[0] == 0: the sentinel itself
    ukey, inv, cnt = torch.unique_consecutive(skey, return_inverse=True, return_counts=True)
    pmap = torch.empty(n + 1, dtype=torch.int32, device=dev)
    pmap[order] = (inv - 1).to(torch.int32)                                   # voxel id per point, -1 = dropped
    pmap = pmap[1:]
    vkey = ukey[1:]
    counts = cnt[1:].to(torch.int32)
    voxel_coors = ((vkey.unsqueeze(-1) // stride) % ext).to(coors.dtype)
    order = (order[1:] - 1).to(torch.int32)                                   # point ids, ascending inside every voxel
    seg = torch.empty(counts.numel() + 1, dtype=torch.int32, device=dev)
    seg[0] = 0
    torch.cumsum(counts, 0, out=seg[1:])
    seg += (cnt[0] - 1).to(torch.int32)                                        # dropped points come first in `order`
    return voxel_coors, pmap.contiguous(), counts.contiguous(), (order.contiguous(), seg)


def scatter_index(coors):
    """coors (N, ndim) int -> (voxel_coors (M, ndim), point2voxel_map (N,) int32 with -1 for dropped points,
    voxel_points_count (M,) int32).  Voxels are the sorted unique rows; a point with ANY negative coordinate is
    dropped (scatter_points_cuda.cu:236-246)."""
    if coors.size(0) == 0:
        return (coors.clone().detach(), coors.new_empty((0,), dtype=torch.int32),
                coors.new_empty((0,), dtype=torch.int32))
    return _index_and_grouping(coors.contiguous())[:3]


def group_points(point2voxel_map, voxel_points_count):
    """(order, seg) from an existing map: point ids grouped by voxel in ascending id, and the (M+1) segment bounds into
    `order` (the dropped points, map -1, come first).  No host read."""
    order = torch.sort(point2voxel_map, stable=True)[1].to(torch.int32)
    seg = torch.zeros(voxel_points_count.numel() + 1, dtype=torch.int32, device=point2voxel_map.device)
    torch.cumsum(voxel_points_count, 0, out=seg[1:])
    seg += (point2voxel_map.numel() - seg[-1:]).to(torch.int32)              # leading -1 entries, taken on the device
    return order.contiguous(), seg.contiguous()


def _scatter_reduce(feats, point2voxel_map, voxel_points_count, reduce_type='max', grouping=None):
    """The reduce with its autograd node in the host glue (`_lib.load_node()`: _pynode.GDScatterReduce — the shape of the
    reference's own `_ScatterReduce` Function, ops/voxel/scatter.py:29-72 — or its C++ twin in csrc/torch_node.cpp): forward
    vox_scatter_reduce over the grouped points; backward the voxel-ordered form for rows of one 128-byte line and more (c % 4 == 0, 32 <= c <= 256:
    every gradient row read once and streamed to its points), the map-ordered gather for narrower rows (c = 10: 40 us against
    118 us, profiles/r04_scatter_kernel_time.txt).  With the Python glue the call is host-bound at ~110 us forward + backward
    below ~0.5 M points, with the C++ node at ~70 us."""
    if not feats.is_cuda:
        raise RuntimeError('scatter_reduce: the MI355X implementation has no CPU path '
                           '(neither has the reference: voxelization.h:46)')
    if feats.size(0) == 0:
        return feats.clone().detach()
    n = feats.shape[0]
    if point2voxel_map.numel() != n or point2voxel_map.dtype != torch.int32 or \
            voxel_points_count.dtype != torch.int32:
        raise RuntimeError('scatter_reduce: point2voxel_map must be an int32 tensor with one entry per point and '
                           'voxel_points_count int32 (as scatter_index returns them)')
    order, seg = grouping if grouping is not None else group_points(point2voxel_map, voxel_points_count)
    return _lib.load_node().scatter_reduce(feats, point2voxel_map.contiguous(), voxel_points_count.contiguous(), REDUCE[reduce_type],
                                           order, seg)


def scatter_reduce(feats, point2voxel_map, voxel_points_count, reduce_type='max', grouping=None):
    """feats (N,C) -> (M,C): max | mean | sum of the rows that share a voxel (reference signature + optional
    precomputed `grouping` = group_points(...))."""
    assert reduce_type in REDUCE, f'do not support reduce type {reduce_type}'
    return _scatter_reduce(feats, point2voxel_map, voxel_points_count, reduce_type, grouping)


class Scatter(object):
    """Voxelise once, reduce / map back many times — the reference's `Scatter` surface
    (/root/reference/mmdet3d_gaussian/ops/voxel/scatter.py:75-144: `voxel_coors`, `pts_voxel_maps`,
    `voxel_pts_counts`, `pts_coors`, `batch_size`, `reduce`, `mapback`, `reduce_mapback`).

    The reference walks the batch in Python (one unique_dim + index_put per sample, and `.max().item()` to learn the
    batch size).  Here batched (b, z, y, x) rows are indexed in ONE device pass: the batch column is simply the most
    significant digit of the voxel key, which orders the voxels exactly as the per-sample loop does.  The same pass
    yields the by-voxel grouping every `reduce` needs."""

    def __init__(self, coors):
        self._pts_coors = coors
        self._batched = coors.size(-1) != 3
        self._batch_size = None
        self._grouping = None
        if coors.numel() == 0:
            if self._batched:
                self._batch_size = 1
            self.voxel_coors = coors.clone().detach()
            self.pts_voxel_maps = coors.new_empty((0,), dtype=torch.int32)
            self.voxel_pts_counts = coors.new_empty((0,), dtype=torch.int32)
            return
        (self.voxel_coors, self.pts_voxel_maps, self.voxel_pts_counts,
         self._grouping) = _index_and_grouping(coors.contiguous())

    @property
    def pts_coors(self):
        return self._pts_coors

    @property
    def batch_size(self):
        """None for (z, y, x) rows; otherwise 1 + the largest batch index (read from the device on first use only)."""
        if self._batched and self._batch_size is None:
            self._batch_size = int(self._pts_coors[:, 0].max()) + 1
        return self._batch_size

    def mapback(self, voxel_feats, default_feat=0):
        """(M, C) voxel rows -> (N, C) point rows; dropped points receive `default_feat`."""
        if voxel_feats.size(0) == 0:
            return voxel_feats.new_full((self.pts_voxel_maps.numel(),) + tuple(voxel_feats.shape[1:]), default_feat)
        idx = self.pts_voxel_maps.long()
        rows = voxel_feats.index_select(0, idx.clamp(min=0))
        keep = (idx >= 0).reshape((-1,) + (1,) * (rows.dim() - 1))
        return torch.where(keep, rows, rows.new_full((), default_feat))

    def reduce(self, pts_feats, reduce_op):
        if reduce_op not in REDUCE:
            raise AssertionError(f'reduce_op must be one of {sorted(REDUCE)}, got {reduce_op!r}')
        voxel_feats = scatter_reduce(pts_feats.contiguous(), self.pts_voxel_maps, self.voxel_pts_counts, reduce_op,
                                     self._grouping)
        return voxel_feats, self.voxel_coors

    def reduce_mapback(self, pts_feats, reduce_op, default_feat=0):
        return self.mapback(self.reduce(pts_feats, reduce_op)[0], default_feat)
