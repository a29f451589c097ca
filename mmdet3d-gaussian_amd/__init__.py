"""mmdet3d-gaussian hot path for AMD MI355X (gfx950) — the rows of SURVEY.md §8 and nothing else at the top level.

  * ``GDLoss``                 — §8 a1-a9: /root/reference/mmdet3d_gaussian/models/losses/gaussian_distance_loss.py:251
  * ``LOSSES`` / ``build_loss``— §8 b: the registry verbs heads use to build it from config dicts
  * ``nms_gpu`` & friends      — §8 aN: the mmdet3d iou3d ops the reference imports (gd_centerpoint_head.py:9, pvrcnn_bbox_head.py:12)
                                 and the multi-class loops around them at the call sites
  * ``iou_bev`` / ``iou_3d`` / ``trans_bev`` / ``boxes_iou_bev`` / ``match_coco`` — §8 aI, f3: ops/eval/affinity.cpp, matcher.cpp
  * ``sharded``                — §8 e: pair-sharded multi-GPU evaluation (one process per GPU, RCCL)
  * coders + ``anchor_*_loss`` / ``center_head_*`` loss slices — §8 f1, f2: the bbox coders either side of the loss and the two
                                 head-level regression slices with the decode fused into the kernel
                                 (gd_anchor3d_head.py:95-161, gd_centerpoint_head.py:413-434)
  * ``Scatter`` / ``scatter_index`` / ``scatter_reduce`` — §8 f4: ops/voxel/scatter.py
  * ``QueryAndGroup`` / ``ball_query`` / ``grouping`` / ``furthest_point_sample`` / ``furthest_point_sample_stacked`` — PV-RCNN's
                                 voxel-set-abstraction ops: ops/vsa/group_points.py, ops/vsa/sample_points.py
  * ``points_in_boxes_part`` / ``points_in_boxes_all`` (+ ``*_stacked``) / ``pointwise_mask_targets`` / ``roi_grid_points`` /
    ``roi_grid_queries``       — mmdet3d's roiaware_pool3d point-in-box ops, PointwiseMaskHead.get_targets
                                 (pointwise_mask_head.py:62-92) and the RoI grid points (batch_roigrid_extractor.py:56-71)
  * ``pvrcnn_head_get_targets`` / ``pvrcnn_head_loss`` — PVRCNNBboxHead's training slice (pvrcnn_bbox_head.py:140-351): the targets
                                 in one launch, the class, box and corner losses with their gradients in one more, no host sync
  * ``pvrcnn_seg_loss`` / ``keypoint_reweight`` — the keypoint segmentation slice: PointwiseMaskHead.loss
                                 (pointwise_mask_head.py:124-144) with its gradient in one launch, and the keypoint reweighting of
                                 PVRCNNROIHead._bbox_forward (pvrcnn_roi_head.py:211-212), forward and backward, one launch each
  * ``bev_interpolate`` / ``voxel_centers`` / ``sample_keypoints`` — VoxelSetAbstraction.forward's statements outside the MLPs
                                 (voxel_set_abstraction.py:153-244, :303-305): the keypoints' bilinear BEV features in one launch
                                 (backward: a fill and one launch), the voxel centres with their per-sample counts, the keypoint gather
  * ``hard_voxelize`` / ``dynamic_voxelize`` / ``Voxelization`` / ``HardSimpleVFE`` / ``voxel_mean`` / ``pvrcnn_voxelize`` — the first
                                 stage: mmdet3d's hard Voxelization op and the mean voxel encoder for the whole batch in one
                                 stream-ordered call (pv_rcnn.py:43-49, 66-86), in the deterministic first-appearance order
  * ``point_voxel_stats`` / ``PointVoxelStatsCalculator`` / ``pillar_decorate`` / ``PillarFeatureDecorator`` — the pillar encoders'
                                 point decoration between voxelization and the first nn.Linear (voxel_encoders/utils.py:48-89,
                                 pillar_encoder.py:105-153, 214-216): two launches and one, fixed fp32 sequences
  * ``multi_view_voxelize`` / ``to_cylindrical`` / ``to_spherical`` / ``pillar_scatter`` / ``PointPillarsScatter`` / ``view_sample`` — the
                                 multi-view pillar encoder's view ops (pillar_od.py:24-70, pillar_mvf_encoder.py:80-107): every view's
                                 transform and cells in one launch, the dense pillar canvas, the per-point view-map sampling
  * ``sparse_conv_index`` / ``sparse_conv`` / ``sparse_to_dense`` / ``SparseConvTensor`` / ``SubMConv3d`` / ``SparseConv3d`` /
    ``SparseSequential`` / ``SparseBasicBlock`` / ``make_sparse_convmodule`` / ``SparseEncoder`` / ``MlvlSparseEncoder`` — the sparse 3D
                                 convolution of the middle encoders (middle_encoders/mlvl_sparse_encoder.py:11-32; spconv 1.x's surface,
                                 restated): neighbour tables in one stream-ordered build, one launch per layer forward, no atomics;
                                 ``compute_dtype=torch.float16 / torch.bfloat16 / 'auto'`` (off by default) runs a layer on 16-bit
                                 operands on the matrix cores with fp32 accumulation and fp32 parameter gradients
  * ``fuse_sparse_conv_bn`` / ``FusedSparseConv`` / ``FusedSparseBasicBlock`` / ``SparseEncoder.fuse()`` — the eval BatchNorm, the residual
                                 add and the ReLU of a sparse layer inside the convolution's launch (``sparse_conv(..., scale=, shift=,
                                 residual=, activation=)``): one fixed fp32 sequence per element, one rounding on the 16-bit path
  * ``sparse_batch_norm`` / ``SparseBatchNorm1d`` / ``SparseNormBasicBlock`` / ``convert_sparse_batchnorm`` / ``SparseEncoder.convert_norm()``
                               — batch normalisation over the LIVE rows of a sparse tensor with the residual add and the ReLU in the same
                                 pass, training and eval, forward and backward: what training in the static ``max_out`` form needs
  * ``sparse_inverse_conv`` / ``sparse_conv_index_inverse`` / ``SparseInverseConv3d`` / ``make_sparse_inverse_convmodule`` / ``sparse_max_pool`` /
    ``SparseMaxPool3d`` / ``ToDense`` / ``SparseUNet`` — the way back up: spconv 1.x's inverse convolution as the existing launches over the
                                 swapped tables of the strided layer it undoes, max pooling over the same tables (one gather launch
                                 each way, the output a copy of an input element, ties share the gradient), and mmdet3d's sparse U-Net
                                 middle encoder with per-voxel ``seg_features``
  * ``GraphedStep``            — a launch-bound loss slice, forward and backward, captured once as a hipGraph and replayed
Everything outside §8 that earlier rounds built (frozen, DESIGN_EXTRAS.md) lives in ``mmdet3d_gaussian_amd.extras``.

All arithmetic runs in hand-written HIP kernels reached through the C ABI of include/gd3d.h (libgd3d.so, built in-tree by
``build.py``); CPU tensors take the library's own `_cpu` twins (the kernels' per-pair source compiled for the host).  Nothing
substitutes for the library: a GPU tensor never takes a CPU path.  The host layer above the C ABI is Python
(torch.autograd.Function + ctypes, ``_pynode.py``); ``csrc/torch_node.cpp`` is an optional C++ accelerator with the same surface
(``GD3D_HOST=python|cpp``, ``_lib.host_glue()``).
"""
from . import build as _build_mod
from ._lib import host_glue, load as load_library, lib_path, set_host_glue
from .gd_loss import GDLoss, make_params
from .iou3d import (box3d_multiclass_nms, boxes_iou_bev, circle_nms, iou_3d, iou_bev, multi_class_nms, multi_class_nms_batch, nms_gpu, nms_gpu_batched,
                    nms_gpu_multi, nms_normal_gpu, xywhr2xyxyr)
from .registry import LOSSES, Registry, build_loss
from . import sharded
from .coders import CenterPointBBoxCoderRev, CenterPointBBoxYawCoder, DeltaXYZWLHRBBoxCoder, PointBBoxYawCoder
from .graphed import GraphedStep
from .evaluation import ap_accumulate, frames_records, match_coco, tp_records, trans_bev
from .registry import (EVAL_AFFINITYCALS, EVAL_BREAKDOWNS, EVAL_MATCHERS, EVAL_TPMETRIC, build_eval_affinity_calculator, build_eval_breakdown,
                       build_eval_matcher, build_eval_tp_metric)
from .eval_map import (FlexibleStatisticsEval, LidarCenterTransBEV, LidarIOU3D, LidarIOUBEV, MatcherCoCo, NoBreakdown, RangeBreakdown,
                       VolumeBreakdown, eval_map_flexible)
from .scatter import Scatter, scatter_index, scatter_reduce
from .vsa import QueryAndGroup, ball_query, furthest_point_sample, furthest_point_sample_stacked, grouping
from .points_in_boxes import (pointwise_mask_targets, points_in_boxes_all, points_in_boxes_all_stacked, points_in_boxes_part,
                              points_in_boxes_part_stacked, roi_grid_points, roi_grid_queries)
from .pvrcnn_train import pvrcnn_head_get_targets, pvrcnn_head_loss
from .pvrcnn_sample import bbox_overlaps_3d, pvrcnn_assign_and_sample
from .pvrcnn_seg import keypoint_reweight, pvrcnn_seg_loss
from .vsa_bev import bev_interpolate, sample_keypoints, voxel_centers
from .voxel_query import (VoxelQueryAndGroup, VoxelQueryIndex, voxel_point_indices, voxel_query, voxel_query_coords, voxel_query_index)
from .voxelize import HardSimpleVFE, Voxelization, dynamic_voxelize, hard_voxelize, pvrcnn_voxelize, voxel_mean
from .pillar_feat import PillarFeatureDecorator, PointVoxelStatsCalculator, pillar_decorate, point_voxel_stats
from .view_net import PointPillarsScatter, multi_view_voxelize, pillar_scatter, to_cylindrical, to_spherical, view_sample
from .simota import Point3DRangeGenerator, SimOTABEVAssigner, simota_assign
from .rpn_proposal import PartA2RPNHeadProposals, rpn_proposals
from .sparse_tensor import SparseConvTensor, SparseModule, SparseSequential, ToDense, sparse_to_dense
from .sparse_conv import (FusedSparseConv, SparseConv3d, SparseConvIndex, SparseInverseConv3d, SubMConv3d, sparse_conv, sparse_conv_index,
                          sparse_conv_index_inverse, sparse_inverse_conv)
from .sparse_bn import SparseBatchNorm1d, sparse_batch_norm
from .sparse_pool import SparseMaxPool3d, sparse_max_pool
from .sparse_encoder import (FusedSparseBasicBlock, MlvlSparseEncoder, SparseBasicBlock, SparseEncoder, SparseNormBasicBlock, SparseUNet,
                             convert_sparse_batchnorm, fuse_sparse_conv_bn, make_sparse_convmodule, make_sparse_inverse_convmodule)
from .head_loss import (anchor_decoded_gd_loss, anchor_head_bbox_loss, anchor_head_decoded_loss,
                        anchor_head_decoded_loss_fused, center_head_gd_loss, center_head_losses)
from . import extras


def build(force=False, verbose=False):
    """Compile csrc/*.hip for gfx950 into mmdet3d-gaussian_amd/libgd3d.so, and csrc/torch_node.cpp (GDLoss's autograd node,
    host C++ above the C ABI) into mmdet3d-gaussian_amd/_gd3d_node.so.  Returns the library's path."""
    path = _build_mod.build(force=force, verbose=verbose)
    _build_mod.build_node(force=force, verbose=verbose)
    return path


__all__ = ['GDLoss', 'LOSSES', 'Registry', 'build_loss', 'make_params', 'nms_gpu', 'nms_normal_gpu', 'nms_gpu_batched', 'nms_gpu_multi',
           'multi_class_nms', 'multi_class_nms_batch', 'box3d_multiclass_nms', 'circle_nms', 'boxes_iou_bev', 'iou_bev', 'iou_3d', 'xywhr2xyxyr',
           'trans_bev', 'match_coco', 'sharded', 'build', 'load_library', 'lib_path', 'host_glue', 'set_host_glue',
           'CenterPointBBoxCoderRev', 'CenterPointBBoxYawCoder', 'DeltaXYZWLHRBBoxCoder', 'PointBBoxYawCoder', 'GraphedStep',
           'anchor_decoded_gd_loss', 'anchor_head_decoded_loss', 'anchor_head_decoded_loss_fused', 'anchor_head_bbox_loss', 'center_head_gd_loss',
           'center_head_losses', 'Scatter', 'scatter_index', 'scatter_reduce', 'QueryAndGroup', 'ball_query', 'grouping',
           'furthest_point_sample', 'furthest_point_sample_stacked', 'points_in_boxes_part', 'points_in_boxes_all',
           'points_in_boxes_part_stacked', 'points_in_boxes_all_stacked', 'pointwise_mask_targets', 'roi_grid_points', 'roi_grid_queries',
           'pvrcnn_head_get_targets', 'pvrcnn_head_loss', 'bbox_overlaps_3d', 'pvrcnn_assign_and_sample', 'pvrcnn_seg_loss',
           'keypoint_reweight', 'bev_interpolate', 'voxel_centers', 'sample_keypoints', 'hard_voxelize', 'dynamic_voxelize', 'Voxelization',
           'HardSimpleVFE', 'voxel_mean', 'pvrcnn_voxelize', 'point_voxel_stats', 'PointVoxelStatsCalculator',
           'pillar_decorate', 'PillarFeatureDecorator', 'multi_view_voxelize', 'to_cylindrical', 'to_spherical', 'pillar_scatter',
           'PointPillarsScatter', 'view_sample', 'simota_assign', 'SimOTABEVAssigner', 'Point3DRangeGenerator', 'sparse_conv_index', 'sparse_conv',
           'sparse_to_dense', 'SparseConvIndex', 'SparseConvTensor', 'SparseModule', 'SubMConv3d', 'SparseConv3d', 'SparseSequential', 'SparseBasicBlock',
           'make_sparse_convmodule', 'SparseEncoder', 'MlvlSparseEncoder', 'fuse_sparse_conv_bn', 'FusedSparseConv', 'FusedSparseBasicBlock', 'sparse_batch_norm',
           'SparseBatchNorm1d', 'SparseNormBasicBlock', 'convert_sparse_batchnorm', 'sparse_conv_index_inverse', 'sparse_inverse_conv', 'SparseInverseConv3d',
           'make_sparse_inverse_convmodule', 'sparse_max_pool', 'SparseMaxPool3d', 'ToDense', 'SparseUNet', 'rpn_proposals', 'PartA2RPNHeadProposals',
           'extras', 'voxel_query_index', 'voxel_point_indices', 'voxel_query_coords', 'voxel_query', 'VoxelQueryIndex', 'VoxelQueryAndGroup',
           'tp_records', 'frames_records', 'ap_accumulate', 'FlexibleStatisticsEval', 'eval_map_flexible', 'NoBreakdown', 'RangeBreakdown', 'VolumeBreakdown',
           'LidarIOU3D', 'LidarIOUBEV', 'LidarCenterTransBEV', 'MatcherCoCo', 'EVAL_MATCHERS', 'EVAL_AFFINITYCALS', 'EVAL_BREAKDOWNS',
           'EVAL_TPMETRIC', 'build_eval_matcher', 'build_eval_affinity_calculator', 'build_eval_breakdown', 'build_eval_tp_metric']
