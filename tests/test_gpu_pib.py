"""The point-in-box kernels of csrc/pib.hip on the MI355X: device against the `_cpu` twin and against the fp32 numpy oracle
(tests/pib_ref.py), all with EXACT equality, on the smallest shapes at which each kernel can still go wrong (tests/pib_cases.py);
outputs pre-filled with a sentinel to show that every element is written; strided and non-fp32 inputs; graph capture."""
import numpy as np
import pytest
import torch

import mmdet3d_gaussian_amd as amd
import pib_cases as cases
import pib_ref
from mmdet3d_gaussian_amd import _lib
from mmdet3d_gaussian_amd.vsa import _ptr

pytestmark = pytest.mark.gpu


def _t(*arrays):
    return [torch.from_numpy(np.array(a)) for a in arrays]


def _dev(*tensors):
    return [t.cuda() for t in tensors]


@pytest.mark.parametrize('with_cnt', [True, False])
@pytest.mark.parametrize('name', sorted(cases.STACKS))
def test_device_equals_oracle_and_twin_on_stacked_batches(name, with_cnt):
    """part and both element types of all: B = 3 with unequal counts, a sample without points, one without boxes, sample sizes around
    the wave and the workgroup, T around the LDS box tile (two column tiles of `all`), T % 4 == 0 (packed bytes) and not"""
    host = _t(*cases.stack(name))
    xyz, pc, boxes, labels, bc = _dev(*host)
    cnt, hcnt = (bc, host[4]) if with_cnt else (None, None)
    want_flags, want_idx = cases.reference(name, with_cnt)
    idx = amd.points_in_boxes_part_stacked(xyz, pc, boxes, cnt)
    assert idx.dtype == torch.int32 and np.array_equal(idx.cpu().numpy(), want_idx)
    assert torch.equal(idx.cpu(), amd.points_in_boxes_part_stacked(host[0], host[1], host[2], hcnt))
    for dtype in (torch.bool, torch.int32):
        flags = amd.points_in_boxes_all_stacked(xyz, pc, boxes, cnt, dtype=dtype)
        assert flags.dtype == dtype and np.array_equal(flags.cpu().numpy().astype(bool), want_flags)
        assert torch.equal(flags.cpu(), amd.points_in_boxes_all_stacked(host[0], host[1], host[2], hcnt, dtype=dtype))


@pytest.mark.parametrize('extra_width', cases.EXTRA_WIDTHS)
@pytest.mark.parametrize('name', sorted(cases.STACKS))
def test_mask_targets_equal_oracle_and_twin(name, extra_width):
    host = _t(*cases.stack(name))
    xyz, pc, boxes, labels, bc = _dev(*host)
    for with_cnt in (True, False):
        want_seg, want_idx = cases.mask_reference(name, with_cnt, extra_width)
        seg, idx = amd.pointwise_mask_targets(xyz, pc, boxes, labels, extra_width, cases.NUM_CLASSES, return_box_idx=True,
                                              box_cnt=bc if with_cnt else None)
        assert seg.dtype == torch.int64 and np.array_equal(seg.cpu().numpy(), want_seg) and np.array_equal(idx.cpu().numpy(), want_idx)
        t_seg = amd.pointwise_mask_targets(host[0], host[1], host[2], host[3], extra_width, cases.NUM_CLASSES,
                                           box_cnt=host[4] if with_cnt else None)
        assert torch.equal(seg.cpu(), t_seg)


@pytest.mark.parametrize('name', ['t65_wg+1_nopoints', 't64_packed_bytes', 'tile+1_far_first_tile', 't1_63_wg-1_noboxes'])
def test_every_output_element_is_written(name):
    """the C entry points on sentinel-filled outputs: every flag (columns past box_cnt and the rows of the sample without boxes
    included), every target and every index is written, and nothing beyond the arrays (a guard row either side stays intact)"""
    xyz, pc, boxes, labels, bc = _dev(*_t(*cases.stack(name)))
    lib = _lib.load()
    n, t, b = xyz.shape[0], boxes.shape[1], pc.numel()
    want_flags, want_idx = cases.reference(name, True)
    want_seg, _ = cases.mask_reference(name, True, 0.2)
    stream = torch.cuda.current_stream().cuda_stream
    for dtype, size, sentinel in ((torch.uint8, 1, 0x5A), (torch.int32, 4, 0x5A5A5A5A)):
        buf = torch.full((n + 2, t), sentinel, dtype=dtype, device='cuda')
        _lib.check(lib.gd3d_pib_all(_ptr(xyz), _ptr(pc), _ptr(boxes), _ptr(bc), b, n, t, buf[1:].data_ptr(), size, stream), 'gd3d_pib_all')
        got = buf.cpu().numpy()
        assert (got[0] == sentinel).all() and (got[-1] == sentinel).all()
        assert np.array_equal(got[1:-1], want_flags.astype(got.dtype))
    seg = torch.full((n + 2,), -77, dtype=torch.int64, device='cuda')
    idx = torch.full((n + 2,), -77, dtype=torch.int32, device='cuda')
    _lib.check(lib.gd3d_pib_mask_targets(_ptr(xyz), _ptr(pc), _ptr(boxes), _ptr(labels), _ptr(bc), b, n, t, 0.2, cases.NUM_CLASSES,
                                         seg[1:].data_ptr(), idx[1:].data_ptr(), stream), 'gd3d_pib_mask_targets')
    assert seg[0] == -77 and seg[-1] == -77 and idx[0] == -77 and idx[-1] == -77
    assert np.array_equal(seg[1:-1].cpu().numpy(), want_seg) and np.array_equal(idx[1:-1].cpu().numpy(), want_idx)
    part = torch.full((n + 2,), -77, dtype=torch.int32, device='cuda')
    _lib.check(lib.gd3d_pib_part(_ptr(xyz), _ptr(pc), _ptr(boxes), _ptr(bc), b, n, t, part[1:].data_ptr(), stream), 'gd3d_pib_part')
    assert part[0] == -77 and part[-1] == -77 and np.array_equal(part[1:-1].cpu().numpy(), want_idx)


def test_counts_that_do_not_cover_the_rows_or_overrun_them_are_clamped():
    """point rows past the counts' sum are in no box (written: -1, zeros, background); a count beyond the rows left is cut"""
    xyz, pc, boxes, labels, bc = _dev(*_t(*cases.stack('t7_small')))
    n = xyz.shape[0]
    short = torch.tensor([1, 64, 10], dtype=torch.int32, device='cuda')        # 55 rows uncovered
    idx = amd.points_in_boxes_part_stacked(xyz, short, boxes, bc)
    flags = amd.points_in_boxes_all_stacked(xyz, short, boxes, bc)
    seg = amd.pointwise_mask_targets(xyz, short, boxes, labels, 0.2, cases.NUM_CLASSES, box_cnt=bc)
    assert (idx[75:] == -1).all() and not flags[75:].any() and (seg[75:] == cases.NUM_CLASSES).all()
    _, want_idx = cases.reference('t7_small', True)
    assert np.array_equal(idx[:65].cpu().numpy(), want_idx[:65])
    over = torch.tensor([1, 64, 1 << 30], dtype=torch.int32, device='cuda')
    big = torch.tensor([1 << 30, 3, -5], dtype=torch.int32, device='cuda')     # box counts: clamped to T and to 0
    assert np.array_equal(amd.points_in_boxes_part_stacked(xyz, over, boxes, bc).cpu().numpy(), want_idx)
    got = amd.points_in_boxes_part_stacked(xyz, pc, boxes, big).cpu().numpy()
    assert np.array_equal(got[:65], want_idx[:65]) and (got[65:] == -1).all() and len(got) == n


def test_crafted_faces_nesting_degenerate_dims_and_non_finite_points():
    xyz, pc, boxes, labels, want = cases.crafted()
    hx, hpc, hb, hl = _t(xyz, pc, boxes, labels)
    xyz, pc, boxes, labels = _dev(hx, hpc, hb, hl)
    assert np.array_equal(amd.points_in_boxes_all_stacked(xyz, pc, boxes).cpu().numpy(), want)
    assert np.array_equal(amd.points_in_boxes_all(xyz[None], boxes).cpu().numpy()[0], want.astype(np.int32))
    assert np.array_equal(amd.points_in_boxes_part(xyz[None], boxes).cpu().numpy()[0], pib_ref.first_of(want))
    for w in cases.EXTRA_WIDTHS + (0.25,):
        assert torch.equal(amd.pointwise_mask_targets(xyz, pc, boxes, labels, w, cases.NUM_CLASSES).cpu(),
                           amd.pointwise_mask_targets(hx, hpc, hb, hl, w, cases.NUM_CLASSES))


def test_fp64_cloud_on_the_device():
    """the 4099 x 37 cloud: device == fp32 oracle exactly, and == the fp64 evaluation away from the faces"""
    xyz, boxes, inside64, dist = cases.fp64_cloud()
    pts, bx = _dev(*_t(xyz, boxes))
    flags = amd.points_in_boxes_all(pts[None], bx[None])[0].cpu().numpy().astype(bool)
    assert np.array_equal(flags, pib_ref.inside_f32(xyz, boxes))
    far = dist >= cases.FP64_MARGIN
    assert 1.0 - far.mean() <= cases.FP64_MAX_EXCLUDED and np.array_equal(flags[far], inside64[far])
    assert np.array_equal(amd.points_in_boxes_part(pts[None], bx[None])[0].cpu().numpy(), pib_ref.first_of(flags))


@pytest.mark.parametrize('clockwise', [False, True])
@pytest.mark.parametrize('g', cases.GRID_SIZES)
def test_roi_grid_points_equal_oracle_and_twin(g, clockwise):
    for r in cases.ROI_COUNTS:
        host = torch.from_numpy(np.array(cases.rois(r)))
        got = amd.roi_grid_points(host.cuda(), g, clockwise)
        assert got.shape == (r, g ** 3, 3) and np.array_equal(got.cpu().numpy(), cases.grid_reference(r, g, clockwise))
        assert torch.equal(got.cpu(), amd.roi_grid_points(host, g, clockwise))
    guard = torch.full((67, g ** 3, 3), -77.0, device='cuda')                    # the C entry on a sentinel-filled output
    rois = torch.from_numpy(np.array(cases.rois(65))).cuda()
    _lib.check(_lib.load().gd3d_roi_grid_points(_ptr(rois), 7, 0, 65, g, int(clockwise), guard[1:].data_ptr(),
                                                torch.cuda.current_stream().cuda_stream), 'gd3d_roi_grid_points')
    assert (guard[0] == -77).all() and (guard[-1] == -77).all()
    assert np.array_equal(guard[1:-1].cpu().numpy(), cases.grid_reference(65, g, clockwise))


def test_strided_and_non_fp32_inputs():
    host = _t(*cases.stack('t65_wg+1_nopoints'))
    xyz, pc, boxes, labels, bc = _dev(*host)
    want = amd.points_in_boxes_part_stacked(xyz, pc, boxes, bc)
    wide = torch.zeros(len(xyz), 6, device='cuda')
    wide[:, ::2] = xyz
    wide_boxes = torch.zeros(3, 65, 9, device='cuda')
    wide_boxes[..., :7] = boxes
    assert torch.equal(amd.points_in_boxes_part_stacked(wide[:, ::2], pc.long(), wide_boxes, bc.long()), want)
    assert torch.equal(amd.points_in_boxes_part_stacked(xyz.double(), pc, boxes.double(), bc), want)
    h, hb = xyz.half(), boxes.half()
    assert torch.equal(amd.points_in_boxes_part_stacked(h, pc, hb, bc), amd.points_in_boxes_part_stacked(h.float(), pc, hb.float(), bc))
    assert torch.equal(amd.points_in_boxes_all_stacked(h, pc, hb, bc).cpu(),
                       amd.points_in_boxes_all_stacked(h.float().cpu(), host[1], hb.float().cpu(), host[4]))
    rois = torch.from_numpy(np.array(cases.rois(65))).cuda()
    assert torch.equal(amd.roi_grid_points(rois.double(), 6).float(), amd.roi_grid_points(rois, 6))
    r8 = torch.cat([torch.zeros(65, 1, device='cuda'), rois], 1)
    assert torch.equal(amd.roi_grid_queries(r8, 1)[0], amd.roi_grid_points(rois, 6).reshape(-1, 3))


def test_ops_are_capturable_in_one_graph():
    """points_in_boxes_part_stacked + pointwise_mask_targets + roi_grid_queries -> QueryAndGroup captured in one torch.cuda.graph
    and replayed on new input values: no wrapper synchronises with the host"""
    xyz, pc, boxes, labels, bc = _dev(*_t(*cases.stack('t65_wg+1_nopoints')))
    xyz, boxes = xyz.clone(), boxes.clone()
    r7 = torch.from_numpy(np.array(cases.rois(65))).cuda()
    r7[:, :2] = torch.from_numpy(np.random.default_rng(1).uniform(-9, 9, (65, 2)).astype(np.float32)).cuda()   # among the points
    r7[:, 2] = -1.0
    ids = torch.tensor([0] * 30 + [2] * 35, dtype=torch.float32, device='cuda')
    rois = torch.cat([ids[:, None], r7], 1)
    mod = amd.QueryAndGroup(1.5, 8)

    def step():
        idx = amd.points_in_boxes_part_stacked(xyz, pc, boxes, bc)
        seg = amd.pointwise_mask_targets(xyz, pc, boxes, labels, 0.2, cases.NUM_CLASSES, box_cnt=bc)
        new_xyz, new_cnt = amd.roi_grid_queries(rois, 3, grid_size=2)
        out, gidx = mod(xyz, pc, new_xyz, new_cnt)
        return idx, seg, new_xyz, new_cnt, out, gidx

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        first = [t.clone() for t in step()]      # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    with torch.no_grad():
        xyz[:, :2].mul_(0.8)                     # new values in the static buffers
        boxes[..., 6].add_(0.4)
        rois[:, 1:3].add_(0.5)
    graph.replay()
    torch.cuda.synchronize()
    eager = step()
    assert not torch.equal(eager[0], first[0]) and not torch.equal(eager[4], first[4])      # the inputs did change the results
    assert new_cnt_ok(eager[3])
    for got, want in zip(captured, eager):
        assert torch.equal(got, want)


def new_cnt_ok(cnt):
    return cnt.tolist() == [30 * 8, 0, 35 * 8]
