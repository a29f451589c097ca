"""The `_cpu` twins of the point-in-box ops (csrc/pib_cpu.cpp: the kernels' operation sequence compiled for the host) against the
numpy oracles of tests/pib_ref.py — EXACT against the fp32 restatement, and against the independent fp64 evaluation on every pair
that is not within a margin of a face plane — plus the host layer's identities and argument checks.  No GPU needed."""
import numpy as np
import pytest
import torch

import mmdet3d_gaussian_amd as amd
import pib_cases as cases
import pib_ref
from mmdet3d_gaussian_amd import _lib
from mmdet3d_gaussian_amd import points_in_boxes as pib


def _t(*arrays):
    return [torch.from_numpy(np.array(a)) for a in arrays]


def test_module_constants_are_the_kernels():
    lib = _lib.load()
    assert pib.BOX_TILE == lib.gd3d_pib_box_tile() and pib.WORKGROUP_POINTS == lib.gd3d_pib_workgroup_points()
    sizes = {n for pts, _, _ in cases.STACKS.values() for n in pts}
    assert {0, 1, 63, 64, 65, cases.WG - 1, cases.WG, cases.WG + 1} <= sizes
    assert {0, 1, 7, 64, 65, cases.TILE - 1, cases.TILE, cases.TILE + 1} <= {t for _, _, t in cases.STACKS.values()}


@pytest.mark.parametrize('with_cnt', [True, False])
@pytest.mark.parametrize('name', sorted(cases.STACKS))
def test_twins_equal_the_fp32_oracle_on_stacked_batches(name, with_cnt):
    xyz, pc, boxes, labels, bc = _t(*cases.stack(name))
    cnt = bc if with_cnt else None
    want_flags, want_idx = cases.reference(name, with_cnt)
    idx = amd.points_in_boxes_part_stacked(xyz, pc, boxes, cnt)
    assert idx.dtype == torch.int32 and np.array_equal(idx.numpy(), want_idx)
    for dtype in (torch.bool, torch.int32):
        flags = amd.points_in_boxes_all_stacked(xyz, pc, boxes, cnt, dtype=dtype)
        assert flags.dtype == dtype and flags.shape == want_flags.shape
        assert np.array_equal(flags.numpy().astype(bool), want_flags)
        if dtype == torch.int32:
            assert set(np.unique(flags.numpy())) <= {0, 1}
    # part == first nonzero column of all
    assert np.array_equal(idx.numpy(), pib_ref.first_of(flags.numpy().astype(bool)))
    if boxes.shape[1] >= 64 and with_cnt:
        assert (want_idx >= 0).any() and (want_idx < 0).any() and (want_flags.sum(1) > 1).any()


def test_second_tile_decides_when_the_first_holds_no_hit():
    _, want_idx = cases.reference('tile+1_far_first_tile', True)
    first = want_idx[:cases.WG]
    assert (first >= cases.TILE - 1).any() and (first == cases.TILE).any() and not ((first >= 0) & (first < cases.TILE - 1)).any()


@pytest.mark.parametrize('extra_width', cases.EXTRA_WIDTHS)
@pytest.mark.parametrize('with_cnt', [True, False])
@pytest.mark.parametrize('name', sorted(cases.STACKS))
def test_mask_targets_twin_equals_the_oracle(name, with_cnt, extra_width):
    xyz, pc, boxes, labels, bc = _t(*cases.stack(name))
    want_seg, want_idx = cases.mask_reference(name, with_cnt, extra_width)
    seg, idx = amd.pointwise_mask_targets(xyz, pc, boxes, labels, extra_width, cases.NUM_CLASSES, return_box_idx=True,
                                          box_cnt=bc if with_cnt else None)
    assert seg.dtype == torch.int64 and idx.dtype == torch.int32
    assert np.array_equal(seg.numpy(), want_seg) and np.array_equal(idx.numpy(), want_idx)
    if boxes.shape[1] >= 64 and extra_width != 0:
        assert (want_seg == -1).any()
    if extra_width == 0:
        assert not (want_seg == -1).any()


@pytest.mark.parametrize('extra_width', cases.EXTRA_WIDTHS)
def test_mask_targets_equal_the_literal_reference_chain(extra_width):
    """PointwiseMaskHead.get_targets_single as the reference writes it — two `points_in_boxes_part` calls per sample (the gt boxes,
    the enlarged boxes), the labels padded with the background class, a gather, and the xor into -1 — built from this package's own
    part op, against the one-launch form; the per-sample list form and the (N, 4) points form of the wrapper too."""
    name = 't65_wg+1_nopoints'
    xyz, pc, boxes, labels, bc = _t(*cases.stack(name))
    st = pib_ref.starts(pc.numpy())
    chain, gt_list, lb_list, bxyz = [], [], [], []
    for b in range(len(pc)):
        p = xyz[st[b]:st[b + 1]]
        gb, gl = boxes[b, :bc[b]], labels[b, :bc[b]]
        gt_list.append(gb)
        lb_list.append(gl)
        bxyz.append(torch.cat([torch.full((len(p), 1), float(b)), p], 1))
        big = torch.from_numpy(pib_ref.enlarge(gb.numpy(), extra_width))
        i = amd.points_in_boxes_part(p[None], gb[None])[0].long()
        e = amd.points_in_boxes_part(p[None], big[None])[0].long()
        padded = torch.nn.functional.pad(gl, (1, 0), mode='constant', value=cases.NUM_CLASSES)
        seg = padded[i + 1]
        seg[(i >= 0) ^ (e >= 0)] = -1
        chain.append(seg)
    chain = torch.cat(chain)
    assert torch.equal(amd.pointwise_mask_targets(xyz, pc, boxes, labels, extra_width, cases.NUM_CLASSES, box_cnt=bc), chain)
    assert torch.equal(amd.pointwise_mask_targets(xyz, pc, gt_list, lb_list, extra_width, cases.NUM_CLASSES), chain)
    assert torch.equal(amd.pointwise_mask_targets(torch.cat(bxyz), None, gt_list, lb_list, extra_width, cases.NUM_CLASSES), chain)


def test_crafted_faces_nesting_degenerate_dims_and_non_finite_points():
    """x / y faces strict, z faces inclusive; nested and overlapping boxes (part: the lowest index, all: both); zero and negative
    dims contain nothing; NaN and +-inf coordinates are in no box; |rz| up to 100; the SimOTA tall box"""
    xyz, pc, boxes, labels, want = cases.crafted()
    for row, (_, inside) in enumerate(cases.CRAFTED_POINTS):
        assert sorted(np.flatnonzero(want[row])) == sorted(inside), (row, np.flatnonzero(want[row]))   # the oracle says what the table says
    assert not want[:, 2:5].any() and want[len(cases.CRAFTED_POINTS):, 6:8].sum() > 20
    xyz, pc, boxes, labels = _t(xyz, pc, boxes, labels)
    flags = amd.points_in_boxes_all_stacked(xyz, pc, boxes)
    assert np.array_equal(flags.numpy(), want)
    assert np.array_equal(amd.points_in_boxes_all(xyz[None], boxes).numpy()[0], want.astype(np.int32))
    idx = amd.points_in_boxes_part(xyz[None], boxes)
    assert idx.shape == (1, len(xyz)) and np.array_equal(idx.numpy()[0], pib_ref.first_of(want))
    assert idx[0, :12].tolist() == [1, 1, 1, 1, 0, 0, 1, 0, 0, 1, -1, 1]
    seg = amd.pointwise_mask_targets(xyz, pc, boxes, labels, 0.25, cases.NUM_CLASSES)
    # on a strict face of 0 but inside 1 -> label of 1; (4, 0, 1) on the face of 1: inside the enlarged 1 only -> ignore
    assert seg[:12].tolist() == [0, 0, 0, 0, 2, 2, 0, 2, 2, 0, -1, 0]
    assert (seg[12:18] == cases.NUM_CLASSES).all()             # NaN / inf points: background, not even "ignore"


def test_twin_agrees_with_the_independent_fp64_evaluation():
    """Every (point, box) pair whose fp64 distance to each of the six face planes is >= 1e-4 must be decided as fp64 decides it;
    at most 0.1 % of the pairs may lie nearer (and are not compared)."""
    xyz, boxes, inside64, dist = cases.fp64_cloud()
    far = dist >= cases.FP64_MARGIN
    excluded = 1.0 - far.mean()
    print(f'excluded {excluded:.5%} of pairs; {inside64.any(1).mean():.1%} of points in a box, {(inside64.sum(1) > 1).mean():.1%} in several')
    assert excluded <= cases.FP64_MAX_EXCLUDED
    assert inside64.any(1).mean() > 0.1 and (inside64.sum(1) > 1).mean() > 0.01
    pts, bx = _t(xyz, boxes)
    flags = amd.points_in_boxes_all(pts[None], bx[None])[0].numpy().astype(bool)
    assert np.array_equal(flags[far], inside64[far])
    assert np.array_equal(pib_ref.inside_f32(xyz, boxes)[far], inside64[far])      # form (a) against form (b)


@pytest.mark.parametrize('clockwise', [False, True])
@pytest.mark.parametrize('g', cases.GRID_SIZES)
@pytest.mark.parametrize('r', cases.ROI_COUNTS)
def test_roi_grid_points_twin_equals_the_oracle(r, g, clockwise):
    rois = torch.from_numpy(np.array(cases.rois(r)))
    got = amd.roi_grid_points(rois, g, clockwise)
    assert got.shape == (r, g ** 3, 3) and got.dtype == torch.float32
    assert np.array_equal(got.numpy(), cases.grid_reference(r, g, clockwise))


def test_roi_grid_points_geometry():
    """an axis-aligned RoI: the cell centres; a quarter turn counter-clockwise sends local +x to +y, clockwise to -y"""
    roi = torch.tensor([[10.0, 20.0, -1.0, 4.0, 2.0, 2.0, 0.0]])
    p = amd.roi_grid_points(roi, 2)[0]
    assert torch.equal(p, torch.tensor([[9, 19.5, -.5], [9, 19.5, .5], [9, 20.5, -.5], [9, 20.5, .5],
                                        [11, 19.5, -.5], [11, 19.5, .5], [11, 20.5, -.5], [11, 20.5, .5]]))
    roi[0, 6] = np.pi / 2
    ccw, cw = amd.roi_grid_points(roi, 2)[0], amd.roi_grid_points(roi, 2, clockwise=True)[0]
    assert torch.allclose(ccw[4], torch.tensor([10.5, 21.0, -0.5]), atol=1e-5)     # local (+1, -.5) -> (+.5, +1)
    assert torch.allclose(cw[4], torch.tensor([9.5, 19.0, -0.5]), atol=1e-5)       # local (+1, -.5) -> (-.5, -1)


def test_roi_grid_queries_counts_and_row_order():
    r7 = torch.from_numpy(np.array(cases.rois(65)))
    ids = torch.tensor([0] * 20 + [2] * 40 + [3] * 5, dtype=torch.float32)          # sample 1 has no RoI
    rois = torch.cat([ids[:, None], r7], 1)
    new_xyz, cnt = amd.roi_grid_queries(rois, 4, grid_size=6)
    assert cnt.dtype == torch.int32 and cnt.tolist() == [20 * 216, 0, 40 * 216, 5 * 216]
    assert new_xyz.shape == (65 * 216, 3) and np.array_equal(new_xyz.numpy().reshape(65, 216, 3), cases.grid_reference(65, 6, False))
    # it is the pair QueryAndGroup takes
    xyz = new_xyz[::50].contiguous()
    pc = torch.tensor([len(xyz), 0, 0, 0], dtype=torch.int32)
    out, idx = amd.QueryAndGroup(0.8, 4)(xyz, pc, new_xyz, cnt)
    assert out.shape == (65 * 216, 3, 4) and idx.shape == (65 * 216, 4)


def test_other_float_dtypes_and_strides_are_evaluated_in_fp32():
    xyz, pc, boxes, labels, bc = _t(*cases.stack('t7_small'))
    want = amd.points_in_boxes_part_stacked(xyz, pc, boxes, bc)
    wide = torch.zeros(len(xyz), 6)
    wide[:, ::2] = xyz
    assert torch.equal(amd.points_in_boxes_part_stacked(wide[:, ::2], pc.long(), boxes.double(), bc.long()), want)
    h = xyz.half()
    assert torch.equal(amd.points_in_boxes_part_stacked(h, pc, boxes, bc), amd.points_in_boxes_part_stacked(h.float(), pc, boxes, bc))


def test_argument_validation_raises():
    xyz, pc, boxes, labels, bc = _t(*cases.stack('t7_small'))
    with pytest.raises(RuntimeError, match='shape mismatch'):
        amd.points_in_boxes_part_stacked(xyz[:, :2], pc, boxes)
    with pytest.raises(RuntimeError, match='shape mismatch'):
        amd.points_in_boxes_part_stacked(xyz, pc, boxes[..., :6])
    with pytest.raises(RuntimeError, match='shape mismatch'):
        amd.points_in_boxes_part_stacked(xyz, pc[:2], boxes)
    with pytest.raises(RuntimeError, match='shape mismatch'):
        amd.points_in_boxes_part_stacked(xyz, pc, boxes, bc[:2])
    with pytest.raises(RuntimeError, match='integer'):
        amd.points_in_boxes_part_stacked(xyz, pc.float(), boxes)
    with pytest.raises(RuntimeError, match='floating-point'):
        amd.points_in_boxes_part_stacked(xyz.long(), pc, boxes)
    with pytest.raises(RuntimeError, match='dtype'):
        amd.points_in_boxes_all_stacked(xyz, pc, boxes, dtype=torch.float32)
    with pytest.raises(RuntimeError, match='shape mismatch'):
        amd.points_in_boxes_part(xyz, boxes)
    with pytest.raises(RuntimeError, match='shape mismatch'):
        amd.points_in_boxes_all(xyz[None], boxes)                     # B = 1 points, B = 3 boxes
    with pytest.raises(RuntimeError, match='shape mismatch'):
        amd.pointwise_mask_targets(xyz, pc, boxes, labels[:, :3], 0.2, 3)
    with pytest.raises(RuntimeError, match='integer'):
        amd.pointwise_mask_targets(xyz, pc, boxes, labels.float(), 0.2, 3)
    with pytest.raises(RuntimeError, match='shape mismatch'):
        amd.pointwise_mask_targets(xyz, None, boxes, labels, 0.2, 3)  # (N, 3) points without counts
    with pytest.raises(RuntimeError, match='shape mismatch'):
        amd.pointwise_mask_targets(xyz, pc, [boxes[0]], [labels[0], labels[1]], 0.2, 3)
    with pytest.raises(RuntimeError, match='shape mismatch'):
        amd.roi_grid_points(torch.zeros(3, 8))
    with pytest.raises(RuntimeError, match='shape mismatch'):
        amd.roi_grid_queries(torch.zeros(3, 7), 2)
    for g in (0, 17):
        with pytest.raises(RuntimeError, match='grid_size'):
            amd.roi_grid_points(torch.zeros(3, 7), g)
    lib = _lib.load()
    assert lib.gd3d_pib_all_cpu(256, 256, 256, None, 1, 4, 4, 256, 2, 0) == 10001          # element size 2
    assert lib.gd3d_roi_grid_points_cpu(256, 6, 0, 4, 6, 0, 256, 0) == 10001               # row stride below 7
    assert lib.gd3d_pib_part_cpu(256, 256, 256, None, -1, 4, 4, 256, 0) == 10001
