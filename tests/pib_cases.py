"""Seeded inputs of the point-in-box tests (tests/test_pib_cpu.py, tests/test_gpu_pib.py) and their numpy-oracle results, computed
once per process and never modified.

The kernels' constants the shapes are chosen around (csrc/pib.hip): 256 points of one sample per workgroup, waves of 64 lanes,
256 boxes per LDS tile; the byte form of `all` packs 4 flags per store when T % 4 == 0 and writes single bytes otherwise."""
import functools

import numpy as np

import pib_ref
from mmdet3d_gaussian_amd import points_in_boxes as pib

WG, TILE = pib.WORKGROUP_POINTS, pib.BOX_TILE
NUM_CLASSES = 3

# name -> (points per sample, boxes per sample (box_cnt), T).  B = 3 with unequal counts; a sample without points and one without
# boxes; samples of 1, 63, 64, 65, WG - 1, WG, WG + 1 points; T of 0, 1, 7, 64, 65, TILE - 1, TILE, TILE + 1 (box_cnt reaches T in
# some sample of every stack, and stays below it in others).
STACKS = {
    't65_wg+1_nopoints': ((WG + 1, 0, 64), (7, 5, 65), 65),
    't1_63_wg-1_noboxes': ((63, WG - 1, 1), (1, 0, 1), 1),
    't7_small': ((1, 64, 65), (7, 3, 0), 7),
    't64_packed_bytes': ((300, 0, 129), (64, 10, 0), 64),
    'tile-1': ((65, WG, 2), (TILE - 1, 17, 100), TILE - 1),
    'tile': ((WG, 65, 300), (TILE, 64, TILE - 1), TILE),
    'tile+1_far_first_tile': ((WG, 65, 300), (TILE + 1, 64, TILE - 1), TILE + 1),
    't0': ((5, 3, 2), (0, 0, 0), 0),
}


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def stack(name):
    """-> xyz (N, 3), pts_cnt (B,), boxes (B, T, 7), labels (B, T), box_cnt (B,).  EVERY row of `boxes` is a proper box, the rows past
    box_cnt too: with the counts they must be ignored, without them (box_cnt=None) they are tested."""
    pts, bcnt, t = STACKS[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    n, b = sum(pts), len(pts)
    xyz = np.concatenate([rng.uniform(-10, 10, (n, 2)), rng.uniform(-3, 3, (n, 1))], 1).astype(np.float32)
    boxes = np.concatenate([rng.uniform(-9, 9, (b, t, 2)), rng.uniform(-3, 0, (b, t, 1)), rng.uniform(0.5, 6, (b, t, 2)),
                            rng.uniform(0.5, 3, (b, t, 1)), rng.uniform(-4, 4, (b, t, 1))], 2).astype(np.float32)
    if name.endswith('far_first_tile'):
        boxes[0, :TILE - 1, 0] += 100.0      # sample 0: nothing is hit before box TILE - 1, so the second tile decides
        boxes[0, TILE - 1:, 3:5] = 9.0
    labels = rng.integers(0, NUM_CLASSES, (b, t)).astype(np.int64)      # repeated classes
    return _freeze(xyz, np.asarray(pts, np.int32), boxes, labels, np.asarray(bcnt, np.int32))


EXTRA_WIDTHS = (0.2, 0.0, -0.1)


@functools.lru_cache(maxsize=None)
def reference(name, with_cnt):
    """oracle (flags (N, T) bool, box_idx (N,) int32)"""
    xyz, pc, boxes, _, bc = stack(name)
    flags = pib_ref.all_stacked(xyz, pc, boxes, bc if with_cnt else None)
    return _freeze(flags, pib_ref.first_of(flags))


@functools.lru_cache(maxsize=None)
def mask_reference(name, with_cnt, extra_width):
    xyz, pc, boxes, labels, bc = stack(name)
    return _freeze(*pib_ref.mask_targets(xyz, pc, boxes, labels, bc if with_cnt else None, extra_width, NUM_CLASSES))


NAN, INF = float('nan'), float('inf')
# one sample, binary-exact coordinates: 0 a plain box, 1 a box around it (nested), 2 zero dx, 3 negative dy, 4 negative dz,
# 5 the SimOTA tall form, 6 and 7 |rz| up to 100 (range reduction), 8 overlaps 0 on x in (1, 2)
CRAFTED_BOXES = np.asarray([
    (0, 0, 0, 4, 2, 2, 0),
    (0, 0, 0, 8, 8, 4, 0),
    (0, 0, 0, 0, 2, 2, 0),
    (0, 0, 0, 4, -2, 2, 0),
    (0, 0, 0, 4, 2, -2, 0),
    (20, 20, -1e8, 2, 2, 2e8, 0),
    (-20, -20, 0, 4, 2, 2, 100.0),
    (-20, 20, 0, 4, 2, 2, -77.5),
    (2, 0, 0, 2, 2, 2, 0),
], np.float32)
# point -> the boxes that contain it, written out by hand for the cases the issue names
CRAFTED_POINTS = (
    ((2, 0, 1), (1, 8)),            # ON the +x face of 0: outside 0
    ((-2, 0, 1), (1,)),             # ON the -x face of 0
    ((0, 1, 1), (1,)),              # ON the +y face of 0
    ((0, -1, 1), (1,)),             # ON the -y face of 0
    ((0, 0, 0), (0, 1)),            # ON the bottom z face: inside
    ((0, 0, 2), (0, 1)),            # ON the top z face of 0: inside
    ((0, 0, 2.5), (1,)),
    ((1, 0.5, 1), (0, 1)),          # nested: both
    ((1.5, 0, 1), (0, 1, 8)),       # overlapping 0 and 8
    ((3, 3, 3), (1,)),
    ((4, 0, 1), ()),                # ON the +x face of 1
    ((0, 0, 4), (1,)),              # ON the top face of 1
    ((NAN, 0, 1), ()),
    ((0, NAN, 1), ()),
    ((0, 0, NAN), ()),
    ((INF, 0, 1), ()),
    ((0, -INF, 1), ()),
    ((0, 0, INF), ()),
    ((20.5, 20.5, 12345.0), (5,)),
    ((20.5, 19.5, -9e7), (5,)),
    ((21, 20, 0), ()),              # ON a face of the tall box
    ((-20, -20, 1), (6,)),
    ((-20, 20, 1), (7,)),
    ((50, 50, 1), ()),
)


@functools.lru_cache(maxsize=None)
def crafted():
    """-> xyz, pts_cnt, boxes (1, T, 7), labels (1, T), expected flags (N, T) — the hand-written table, plus points strewn around the
    two turned boxes whose flags come from the oracle"""
    rng = np.random.default_rng(3)
    hand = np.asarray([p for p, _ in CRAFTED_POINTS], np.float32)
    around = np.concatenate([rng.uniform(-3, 3, (80, 2)) + c for c in ((-20, -20), (-20, 20))]).astype(np.float32)
    around = np.concatenate([around, rng.uniform(-0.5, 2.5, (160, 1)).astype(np.float32)], 1)
    xyz = np.concatenate([hand, around])
    boxes = CRAFTED_BOXES[None].copy()
    want = pib_ref.inside_f32(xyz, boxes[0])
    labels = np.asarray([[2, 0, 1, 1, 0, 2, 1, 1, 0]], np.int64)
    return _freeze(xyz, np.asarray((len(xyz),), np.int32), boxes, labels, want)


@functools.lru_cache(maxsize=None)
def fp64_cloud():
    """the cloud of the fp64 comparison: 4099 points in [-10, 10]^2 x [-3, 3], 37 boxes with centres in [-9, 9]^2 x [-3, 0], dims
    U(0.5, 6)^2 x U(0.5, 3), yaw U(-4, 4)"""
    rng = np.random.default_rng(7)
    n, t = 4099, 37
    xyz = np.concatenate([rng.uniform(-10, 10, (n, 2)), rng.uniform(-3, 3, (n, 1))], 1).astype(np.float32)
    boxes = np.concatenate([rng.uniform(-9, 9, (t, 2)), rng.uniform(-3, 0, (t, 1)), rng.uniform(0.5, 6, (t, 2)),
                            rng.uniform(0.5, 3, (t, 1)), rng.uniform(-4, 4, (t, 1))], 1).astype(np.float32)
    inside, dist = pib_ref.inside_f64(xyz, boxes)
    return _freeze(xyz, boxes, inside, dist)


FP64_MARGIN = 1e-4          # ~10x the fp32 rounding of coordinates up to 100 with lever arms up to 30
FP64_MAX_EXCLUDED = 1e-3    # share of pairs nearer than the margin to a face plane

GRID_SIZES = (1, 2, 6, 7)
ROI_COUNTS = (0, 1, 65)


@functools.lru_cache(maxsize=None)
def rois(r):
    """(r, 7): centres in a KITTI-like range, yaw mostly in (-4, 4), every eighth up to +-100"""
    rng = np.random.default_rng(100 + r)
    out = np.concatenate([rng.uniform(-40, 70, (r, 2)), rng.uniform(-3, 1, (r, 1)), rng.uniform(0.5, 6, (r, 3)),
                          rng.uniform(-4, 4, (r, 1))], 1).astype(np.float32)
    out[::8, 6] = rng.uniform(-100, 100, out[::8, 6].shape).astype(np.float32)
    return _freeze(out)[0]


@functools.lru_cache(maxsize=None)
def grid_reference(r, g, clockwise):
    return _freeze(pib_ref.grid_points(rois(r), g, clockwise))[0]
