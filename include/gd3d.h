/*
 * gd3d.h — C ABI of libgd3d.so: the MI355X (gfx950) hot path of mmdet3d-gaussian.
 *
 * Drop-in boundary.  The reference has NO native entry point on
 * this path: the losses are ~110-145 ATen ops per call in
 *   /root/reference/mmdet3d_gaussian/models/losses/gaussian_distance_loss.py:8-310
 * and the NMS is the third-party mmdet3d `iou3d_cuda.nms_gpu` pybind call reached from
 *   /root/reference/mmdet3d_gaussian/models/dense_heads/gd_centerpoint_head.py:9,340-345
 *   /root/reference/mmdet3d_gaussian/models/roi_heads/bbox_heads/pvrcnn_bbox_head.py:12,463-464
 * Each entry point below names the reference interface it replaces.
 *
 * Conventions
 *   - plain pointers + sizes; no torch types; every pointer is DEVICE memory of the
 *     current HIP device unless the name says `_host`;
 *   - the caller allocates everything, including the workspace (size from the
 *     *_workspace_bytes query); the library keeps no global state and frees nothing;
 *   - every call is asynchronous and stream-ordered on `stream` (a hipStream_t passed
 *     as void*; NULL = the null stream); no hipDeviceSynchronize / hipMalloc inside,
 *     so calls may be captured in a hipGraph;
 *   - return value: 0 on success, otherwise a hipError_t value or one of the
 *     GD3D_E_* codes below; nothing throws, nothing calls exit().
 *   - float arrays must be 4-byte aligned; 16-byte aligned (N,7) arrays take the fast
 *     LDS-DMA path, others a slower scalar path with identical results.
 */
#ifndef GD3D_H_
#define GD3D_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GD3D_ABI_VERSION 6

/* error codes outside the hipError_t range */
#define GD3D_E_BADARG 10001   /* null pointer / negative size / unknown enum */
#define GD3D_E_TOOLARGE 10002 /* n exceeds what the launch geometry supports */
#define GD3D_E_HOST 10003     /* `_cpu` twins only: a worker thread failed (out of host memory); outputs are not to be used */

/* loss_type: keys of GDLoss.BAG_GD_LOSS (gaussian_distance_loss.py:253-259) */
enum {
  GD3D_GWD3D = 0,        /* gwd3d_loss        :42-106  */
  GD3D_KLD3D = 1,        /* kld3d_loss        :109-141 */
  GD3D_BD3D = 2,         /* bd3d_loss         :144-186 */
  GD3D_JD3D = 3,         /* jd3d_loss         :189-198 */
  GD3D_KLD3D_SYMMAX = 4, /* kld3d_symmax_loss :201-211 */
  GD3D_KLD3D_SYMMIN = 5, /* kld3d_symmin_loss :214-224 */
  GD3D_KFIOU3D = 6,      /* kfiou3d_loss      :227-248 */
  GD3D_NUM_LOSS_TYPES = 7
};

/* fun: postprocess non-linearity (gaussian_distance_loss.py:24-39) */
enum { GD3D_FUN_NONE = 0, GD3D_FUN_LOG1P = 1, GD3D_FUN_EXPM1 = 2, GD3D_FUN_NLOG = 3 };

/* GDLoss hyper-parameters that reach the arithmetic (gaussian_distance_loss.py:261-278). */
typedef struct gd3d_params {
  int32_t loss_type;      /* GD3D_* above */
  int32_t fun;            /* GD3D_FUN_* */
  float tau;              /* tau >= 1 -> 1 - tau/(tau+d); else identity (:36-39) */
  float alpha;            /* xyz vs whlr balance */
  float center_offset[3]; /* gravity-centre offset, default (0,0,0.5) (:12) */
  int32_t flag;           /* gwd3d: `normalize`; all others: `sqrt` (kwargs at :42,:109,...) */
} gd3d_params;

/* ------------------------------------------------------------------------------------
 * Gaussian-distance loss, fused forward + gradient.
 * Replaces: preprocess x2 + one BAG_GD_LOSS function + postprocess + mmdet
 * weight_reduce_loss + `* loss_weight`, and the autograd backward of all of it
 * (gaussian_distance_loss.py:8-39, :42-248, :280-310).
 *
 * For pair i (rows pred[i,:], target[i,:] = (x,y,z,w,h,l,r), fp32, row-major, stride 7):
 *     L_i            = BAG_GD_LOSS[loss_type](preprocess(pred_i), preprocess(target_i))
 *     loss[i]        = scale * w_i * L_i                       (if loss != NULL)
 *     *loss_sum      = scale * sum_i w_i * L_i                 (if loss_sum != NULL; fp32,
 *                      deterministic: fixed-order two-stage reduction, no float atomics)
 *     grad_pred[i,:] = scale * w_i * dL_i/dpred_i              (if grad_pred != NULL)
 *     grad_target[i,:] = scale * w_i * dL_i/dtarget_i          (if grad_target != NULL)
 * with w_i = row_weight[i] (1 if row_weight == NULL).  `scale` carries
 * loss_weight / (avg_factor | N | 1) so that the kernel writes final gradients.
 * n == 0 is legal (loss_sum = 0).  workspace: gd3d_loss_workspace_bytes(n) bytes,
 * 16-byte aligned; required when loss_sum != NULL; whenever it is given the kernel leaves one
 * fp32 partial sum per 256-pair tile at its start.
 * The order in which a launch visits the tiles is internal (it alternates between launches on the same
 * target); every output, the partial sums included, is bit-identical in either order.
 * ---------------------------------------------------------------------------------- */
size_t gd3d_loss_workspace_bytes(int64_t n);

int gd3d_loss_fused(const gd3d_params* params, const float* pred, const float* target,
                    const float* row_weight, int64_t n, float scale, float* loss,
                    float* loss_sum, float* grad_pred, float* grad_target, void* workspace,
                    void* stream);

/* Same, with the per-row weight given as an (n,7) fp32 array whose row mean is taken inside the kernel:
 *   w_i = mean(weight7[i,:])   (GDLoss.forward: `if weight.shape == pred.shape: weight = weight.mean(dim=-1)`,
 * gaussian_distance_loss.py:295-296; the heads pass decode_weight of shape (P,7), gd_anchor3d_head.py:129-141).
 * Saves the separate mean pass.  row_weight and weight7 are mutually exclusive (GD3D_E_BADARG if both). */
int gd3d_loss_fused_w7(const gd3d_params* params, const float* pred, const float* target,
                       const float* row_weight, const float* weight7, int64_t n, float scale,
                       float* loss, float* loss_sum, float* grad_pred, float* grad_target,
                       void* workspace, void* stream);

/* ------------------------------------------------------------------------------------
 * Head-level fusion: the bbox-coder decode that the dense heads run
 * immediately before GDLoss is applied inside the kernel prologue, and the gradient is chained back
 * to the ENCODED prediction, so `pred`/`grad_pred` are the raw head outputs of the positives.
 *   kind = GD3D_PRO_ANCHOR_DELTA: mmdet3d DeltaXYZWLHRBBoxCoder.decode(anchors, deltas) applied to BOTH
 *          pred and target (gd_anchor3d_head.py:133-136).  aux = anchors (n,7) [xa,ya,za,wa,la,ha,ra]:
 *            diag = sqrt(la^2+wa^2); x = xt*diag+xa; y = yt*diag+ya; w = exp(wt)*wa; l = exp(lt)*la;
 *            h = exp(ht)*ha; z = zt*ha + (za + ha/2) - h/2; r = rt + ra
 *   kind = GD3D_PRO_CENTER: CenterPointBBoxYawCoder.decode(locs, pred, correct_yaw=False)[..., :7] applied to
 *          pred only (core/bbox/coders/centerpoint_bbox_yaw_coders.py:32-42, gd_centerpoint_head.py:422-423);
 *          target rows are the annotated boxes as they are.  aux = locs (n,2) fp32 grid coordinates:
 *            x = (p0 + loc0) * out_size_factor * voxel_size[0] + pc_range[0]; y likewise; z = p2;
 *            dims = exp(p3..p5) if norm_bbox else p3..p5; yaw = p6
 * ---------------------------------------------------------------------------------- */
enum { GD3D_PRO_NONE = 0, GD3D_PRO_ANCHOR_DELTA = 1, GD3D_PRO_CENTER = 2 };

typedef struct gd3d_prologue {
  int32_t kind;           /* GD3D_PRO_* */
  int32_t norm_bbox;      /* GD3D_PRO_CENTER: dims are predicted as logs */
  const float* aux;       /* anchors (n,7) or locs (n,2), device memory */
  float out_size_factor;  /* GD3D_PRO_CENTER */
  float voxel_size[2];
  float pc_range[2];
  float reserved;
} gd3d_prologue;

int gd3d_loss_fused_decoded(const gd3d_params* params, const gd3d_prologue* prologue,
                            const float* pred, const float* target, const float* row_weight,
                            const float* weight7, int64_t n, float scale, float* loss,
                            float* loss_sum, float* grad_pred, float* grad_target,
                            void* workspace, void* stream);

/* Profiling form of the same call (bench.py): the two hipEvent_t (as void*, from gd3d_prof_event_create; either may be
 * NULL) are bound to the begin / end timestamps of the fused kernel's OWN dispatch (hipExtLaunchKernel), so
 * gd3d_prof_event_elapsed_ms(start, stop) is that kernel's execution time — what rocprofv3 --kernel-trace reports for
 * it — and no marker packets are added to the stream (events recorded around a launch cost two barrier packets, ~3 us
 * per bracket, and would be charged to the kernel).  The reduce stage, when loss_sum != NULL, follows as usual and is
 * outside the bracket.  With both events NULL this IS gd3d_loss_fused_decoded.  The elapsed-time query has
 * hipEventElapsedTime semantics: it returns hipErrorNotReady (600) while the dispatch is in flight — synchronise first.
 * (No reference counterpart: the reference has no native entry point on this path) */
int gd3d_loss_fused_timed(const gd3d_params* params, const gd3d_prologue* prologue,
                          const float* pred, const float* target, const float* row_weight,
                          const float* weight7, int64_t n, float scale, float* loss,
                          float* loss_sum, float* grad_pred, float* grad_target,
                          void* workspace, void* stream, void* start_event, void* stop_event);
int gd3d_prof_event_create(void** event);
int gd3d_prof_event_destroy(void* event);
int gd3d_prof_event_elapsed_ms(void* start_event, void* stop_event, float* ms);

/* The same slice with the GATHER of the positives fused in as well (one thread per positive, gd_anchor3d_head.py:95-141):
 *   bbox_pred (B, A*7, H, W) raw head output (NCHW, read in place: no permute copy, no index kernels);
 *   bbox_targets / bbox_weights (M,7) with M = B*H*W*A and row m = ((b*H + h)*W + w)*A + a (bbox_weights nullable);
 *   decode_weight: HOST array of 7 floats or NULL (train_cfg['decode_weight']); w_i = mean(bbox_weights[m,:] * decode_weight);
 *   anchors (H*W*A, 7): anchors of ONE sample (the reference repeats them over the batch, :110-112);
 *   pos_inds (P) int64 positive rows m; scale = loss_weight / avg_factor;
 *   *loss_sum = scale * sum_i w_i L_i ;  grad_bbox_pred (B, A*7, H, W) must be ZERO-FILLED by the caller and receives
 *   d loss / d bbox_pred at the positives' 7 channels (nullable).  workspace: gd3d_loss_workspace_bytes(P). */
int gd3d_anchor_head_loss(const gd3d_params* params, const float* bbox_pred, int32_t B, int32_t A,
                          int32_t H, int32_t W, const float* bbox_targets, const float* bbox_weights,
                          const float* decode_weight, const float* anchors, const int64_t* pos_inds,
                          int64_t P, float scale, float* loss_sum, float* grad_bbox_pred,
                          void* workspace, void* stream);

/* Dense form of the same slice: no positive list at all.  One thread per ANCHOR m tests labels[m] (int64 (M), positive iff
 * 0 <= label < num_classes, gd_anchor3d_head.py:101-105) and leaves unless positive — torch.nonzero() (a host sync), the
 * compaction and every index kernel disappear from the training step.  workspace: gd3d_loss_workspace_bytes(M). */
int gd3d_anchor_head_loss_dense(const gd3d_params* params, const float* bbox_pred, int32_t B, int32_t A,
                                int32_t H, int32_t W, const float* bbox_targets, const float* bbox_weights,
                                const float* decode_weight, const float* anchors, const int64_t* labels,
                                int32_t num_classes, float scale, float* loss_sum, float* grad_bbox_pred,
                                void* workspace, void* stream);

/* The whole regression loss of GDAnchor3DHead.loss_single (gd_anchor3d_head.py:95-159) in one launch:
 *   loss_bbox = loss_decoded_bbox(decode(anchors, pred), decode(anchors, target), decode_weight, avg_factor)   (:133-141)
 *             + loss_bbox(pred', target', code_weight, avg_factor)                                             (:152-159)
 * where the second term is mmdet's SmoothL1Loss (third party) on the ENCODED rows, after mmdet3d's
 * add_sin_difference when diff_rad_by_sin (pred'[6] = sin p6 cos t6, target'[6] = cos p6 sin t6).
 *   smooth_l1 == NULL         : only the Gaussian-distance term (same as the two functions above);
 *   smooth_l1->beta           : SmoothL1Loss.beta; 0 selects L1Loss;
 *   smooth_l1->scale          : loss_weight / avg_factor of that term;
 *   smooth_l1->has_code_weight: element weight = bbox_weights[m,k] * code_weight[k] (bbox_weights required), else 1
 *                               (the reference passes weight=None when train_cfg['code_weight'] is falsy, :124-127).
 * The positives are named by EXACTLY ONE of pos_inds (P rows) or labels (dense form, P ignored).
 * With smooth_l1 != NULL the Gaussian term is weighted by mean_k(bbox_weights*decode_weight) only when decode_weight
 * != NULL (:128-131); *loss_sum receives the SUM of both terms, grad_bbox_pred (zero-filled by the caller) their
 * combined gradient.  workspace: gd3d_loss_workspace_bytes(P or M). */
typedef struct gd3d_smooth_l1 {
  float beta;
  float scale;
  int32_t diff_rad_by_sin;
  int32_t has_code_weight;
  float code_weight[7];
  float reserved;
} gd3d_smooth_l1;

int gd3d_anchor_head_bbox_loss(const gd3d_params* params, const gd3d_smooth_l1* smooth_l1,
                               const float* bbox_pred, int32_t B, int32_t A, int32_t H, int32_t W,
                               const float* bbox_targets, const float* bbox_weights,
                               const float* decode_weight, const float* anchors,
                               const int64_t* pos_inds, int64_t P, const int64_t* labels,
                               int32_t num_classes, float scale, float* loss_sum,
                               float* grad_bbox_pred, void* workspace, void* stream);
/* gd3d_anchor_head_bbox_loss, dense form, with the normaliser ON THE DEVICE (ABI 4): scale = gd_weight / *avg_dev and the SmoothL1
 * scale = sl1_weight / *avg_dev (smooth_l1->scale is ignored), divided in double and rounded once.  gd_weight / sl1_weight are the two
 * modules' loss_weight. */
int gd3d_anchor_head_bbox_loss_dyn(const gd3d_params* params, const gd3d_smooth_l1* smooth_l1, const float* bbox_pred,
                                   int32_t B, int32_t A, int32_t H, int32_t W, const float* bbox_targets,
                                   const float* bbox_weights, const float* decode_weight, const float* anchors,
                                   const int64_t* labels, int32_t num_classes, double gd_weight, double sl1_weight,
                                   const float* avg_dev, float* loss_sum, float* grad_bbox_pred, void* workspace,
                                   void* stream);

/* CenterGDHead regression losses of up to 8 tasks in ONE launch (gd_centerpoint_head.py:402-441), reading the head
 * outputs where they lie.  Per task (host struct, device pointers):
 *   maps[6]   : reg (B,2,H,W) | height (B,1,H,W) | dim (B,3,H,W) | yaw (B,1,H,W) | dir (B,2,H,W) | vel (B,2,H,W), NCHW
 *               fp32; reg may be NULL (0.5 is used, :377-378), vel NULL when n_l1 == 2, dir NULL when n_l1 == 0;
 *   grads[6]  : gradient maps of the same shapes, ZERO-FILLED by the caller (any may be NULL).  Two objects may share a
 *               cell: contributions are added in ascending object index by one thread per cell — deterministic, no
 *               float atomics; cell_count receives the number of objects per cell (integer atomics);
 *   pos_ind   : (n,3) int64 [batch, x, y] (:72-80);  anno : (n, anno_cols) fp32 boxes [x,y,z,w,l,h,yaw(,vx,vy)];
 *   gd_scale  : loss_weight / avg_factor of loss_gd,  l1_scale: the same for loss_bbox (L1Loss).
 * coder: kind GD3D_PRO_CENTER (norm_bbox, out_size_factor, voxel_size, pc_range; aux ignored).
 * code_weights: HOST array of n_l1 (0, 2 or 4) floats = train_cfg['code_weights'] for [sin, cos(, vx, vy)].
 * losses (num_tasks, 2) fp32 on the device: [loss_l1, loss_gd] per task.
 * workspace: gd3d_center_head_workspace_bytes(num_tasks, max n).
 * gd3d_center_head_scale: autograd backward for upstream gradients != 1: grads of task t are multiplied by
 *   grad_losses[t*2+1] (reg/height/dim/yaw) or grad_losses[t*2] (dir/vel), device scalars, early exit when == 1. */
typedef struct gd3d_center_task {
  const float* maps[6];
  float* grads[6];
  const int64_t* pos_ind;
  const float* anno;
  int32_t* cell_count; /* (B*H*W) int32, ZERO-FILLED by the caller; required when any grads[] is non-NULL */
  int64_t n;
  int32_t B, H, W, anno_cols;
  float gd_scale, l1_scale;
  /* device-resident form (ABI 4), both nullable: rows_dev -> two int64 on the device, the task's rows are
   * [rows_dev[0], rows_dev[1]) of pos_ind / anno (shared arrays; `n` is then the CAPACITY the launch is sized for, rows
   * beyond it are ignored);  avg_dev -> one fp32 on the device, the scales become gd_weight / max(*avg_dev, 1) and
   * l1_weight / max(*avg_dev, 1) (gd_scale / l1_scale ignored).  With them neither the task's size nor its normaliser
   * passes through the host: center_targets_build's task_start and gd3d_heat_focal_loss's num_pos plug in directly and
   * the whole CenterGDHead.loss becomes one stream-ordered, graph-capturable sequence. */
  const int64_t* rows_dev;
  const float* avg_dev;
  double gd_weight, l1_weight;
} gd3d_center_task;

size_t gd3d_center_head_workspace_bytes(int32_t num_tasks, int64_t max_n);

int gd3d_center_head_loss(const gd3d_params* params, const gd3d_prologue* coder,
                          const gd3d_center_task* tasks, int32_t num_tasks,
                          const float* code_weights, int32_t n_l1, float* losses, void* workspace,
                          void* stream);

int gd3d_center_head_scale(const gd3d_center_task* tasks, int32_t num_tasks,
                           const float* grad_losses, void* stream);

/* The same call in its two steps, for callers that can sort (ABI 3).  gd3d_center_head_loss adds the objects of a shared
 * cell by letting the cell's lowest-index object scan the task's keys: O(shared objects x n / 64) wave steps — nothing at
 * detection sizes (n = 4000, a handful of shared cells), quadratic when tens of thousands of objects fall into few cells.
 *   gd3d_center_head_stage : first step only (losses per object, staged gradient rows, per-object cell keys: one int32 row
 *                            of max_n entries per task inside the workspace, -1 = not live);
 *   gd3d_center_head_keys  : where those rows are: task t's row starts byte_offset + t * byte_stride into the workspace;
 *   gd3d_center_head_finish: second step with the SAME arguments plus `order` (num_tasks, max_n) int64: per task the
 *                            positions 0..max_n-1 of its key row sorted by key, STABLE (so that objects of one cell stay in
 *                            ascending index; e.g. torch.sort(rows, dim=1, stable=True).indices).  One thread per run of equal
 *                            keys adds the run in that order: O(n).  order == NULL: the scanning form.
 * stage + finish(order = NULL) == gd3d_center_head_loss; every form is deterministic, none uses float atomics. */
int gd3d_center_head_stage(const gd3d_params* params, const gd3d_prologue* coder,
                           const gd3d_center_task* tasks, int32_t num_tasks, const float* code_weights,
                           int32_t n_l1, float* losses, void* workspace, void* stream);
int gd3d_center_head_keys(int32_t num_tasks, int64_t max_n, int64_t* byte_offset, int64_t* byte_stride);
int gd3d_center_head_finish(const gd3d_params* params, const gd3d_prologue* coder,
                            const gd3d_center_task* tasks, int32_t num_tasks, const float* code_weights,
                            int32_t n_l1, float* losses, void* workspace, const int64_t* order,
                            void* stream);

/* GDLoss.forward with an (n,7) weight and a reduced result, INCLUDING its early-out, without a host sync.  The reference
 * begins with `if not torch.any(weight > 0): return (pred * weight).sum()` (gaussian_distance_loss.py:290-292) — a full
 * pass over the weights and a device-to-host wait on every training call.  Here the fused kernel leaves, per tile, the
 * loss partial, sum(pred * weight7) and "some weight > 0"; the reduce stage adds them and selects on the device:
 *     *any_positive = any(weight7 > 0)                  (int32, device; NaN weights are not > 0)
 *     *loss_sum     = *any_positive ? scale * sum_i mean(weight7[i,:]) L_i : sum(dec(pred) * weight7)
 * grad_pred / grad_target receive the gradient of the FIRST branch; gd3d_grad_finish (below) puts the second branch's
 * gradient there when *any_positive == 0.  `prologue` as in gd3d_loss_fused_decoded (the early-out's `pred` is then the
 * decoded row); start_event / stop_event as in gd3d_loss_fused_timed (NULL: none).  n == 0: *loss_sum = 0, flag 0. */
int gd3d_loss_fused_select(const gd3d_params* params, const gd3d_prologue* prologue, const float* pred,
                           const float* target, const float* weight7, int64_t n, float scale,
                           float* loss_sum, int32_t* any_positive, float* grad_pred, float* grad_target,
                           void* workspace, void* stream, void* start_event, void* stop_event);

/* Training-size form (n <= gd3d_one_launch_max_n() = 16384 pairs): the same result in ONE launch.  The workgroup whose
 * arrival ticket comes last adds the per-tile partials itself (lane order, fp64) and writes *loss_sum (and, when
 * any_positive != NULL, selects as gd3d_loss_fused_select does; weight7 is then required and row_weight must be NULL).
 *   ticket: device int32 that is 0 when the call is launched and is 0 again when it has completed; calls that share a
 *   ticket must be ordered on one stream (allocate one zeroed word per stream once).  hipGraph-replay safe.
 * The two-stage form above stays the general one: in the streaming regime the arrival ticket costs 20 %. */
int64_t gd3d_one_launch_max_n(void);
int gd3d_loss_fused_one_launch(const gd3d_params* params, const gd3d_prologue* prologue, const float* pred,
                               const float* target, const float* row_weight, const float* weight7, int64_t n,
                               float scale, float* loss_sum, int32_t* any_positive, float* grad_pred,
                               float* grad_target, void* workspace, int32_t* ticket, void* stream);

/* Several losses on ONE target in one fused launch and one second-stage launch (count = 2 or 3): the target tile is read
 * once per 256 rows instead of once per loss.  Loss k is params[k] on (preds[k], target) with scale scales[k]; it writes
 * *loss_sums[k] and grad_preds[k] (nullable), bit-identical to gd3d_loss_fused(&params[k], preds[k], target, NULL, n,
 * scales[k], NULL, loss_sums[k], grad_preds[k], NULL, ...).  No weights, no prologue, no target gradient.
 *   Every params[k] must satisfy gd3d_loss_fused_multi_eligible (the kernel is compiled for those instances only: gwd3d, kld3d
 *   and bd3d with fun log1p and their flag set; any order, repeats allowed), else GD3D_E_BADARG; so is count outside [2, 3].
 *   workspace: gd3d_loss_fused_multi_workspace_bytes(count, n) bytes, 16-byte aligned (<= gd3d_loss_workspace_bytes(n)).
 *   n == 0: every *loss_sums[k] = 0.  The launch after it on this stream gets no target reuse from the Infinity Cache. */
size_t gd3d_loss_fused_multi_workspace_bytes(int32_t count, int64_t n);
int gd3d_loss_fused_multi_eligible(const gd3d_params* params);
int gd3d_loss_fused_multi(int32_t count, const gd3d_params* params, const float* const* preds, const float* target,
                          int64_t n, const float* scales, float* const* loss_sums, float* const* grad_preds,
                          void* workspace, void* stream);

/* Autograd backward of a reduced call; g is the upstream gradient (device scalar).
 *   any_positive == NULL or *any_positive != 0 : grad_pred *= g, grad_target *= g (the grid leaves after two scalar loads
 *       when g == 1: one empty launch, no HBM traffic, no host sync — gd3d_scale_rows for both arrays at once);
 *   *any_positive == 0 : grad_pred = g * d sum(dec(pred) * weight7) / d pred (= g * weight7 without a prologue),
 *       grad_target = 0.  weight7 (and pred / prologue when the forward had a prologue) must be the forward's. */
int gd3d_grad_finish(float* grad_pred, float* grad_target, const float* g, int64_t n,
                     const int32_t* any_positive, const float* weight7, const float* pred,
                     const gd3d_prologue* prologue, void* stream);

/* HBM ceiling probe with the fused kernel's access mix (two streams read, one written): z = x + y over n_floats fp32
 * (multiple of 4, 16-byte aligned arrays), nontemporal 16-byte loads and stores, one vector per thread, 64-thread
 * workgroups (the fastest and most repeatable flat-copy shape measured on MI355X).  The two events
 * (nullable) are bound to the dispatch as in gd3d_loss_fused_timed.  bench.py runs it on the fused kernel's own buffers
 * to report the box's copy ceiling next to roofline.frac.  (Measurement aid; no reference counterpart.) */
int gd3d_probe_stream(const float* x, const float* y, float* z, int64_t n_floats, void* stream,
                      void* start_event, void* stop_event);

/* ------------------------------------------------------------------------------------
 * CenterPointBBoxYawCoder on the device.  Replaces the elementwise torch ops (and their autograd nodes) of
 *   /root/reference/mmdet3d_gaussian/core/bbox/coders/centerpoint_bbox_yaw_coders.py:18-56 (decode), :11-16 (encode);
 * decode is what CenterGDHead.get_bboxes runs at inference (gd_centerpoint_head.py:244, correct_yaw=True).
 *   coder : kind GD3D_PRO_CENTER fields (norm_bbox, out_size_factor, voxel_size, pc_range; aux ignored)
 *   locs (n,2) fp32 grid coordinates, preds (n,c) fp32 rows [dx, dy, z, dim x3, yaw, sin, cos, others...], c >= 7
 *   (c >= 9 when correct_yaw);  out (n, 7 + max(c-9, 0)) = [x, y, z, dim x3, yaw, others...].
 *   correct_yaw == 1: k = floor((atan2(sin, cos) - yaw) / (pi/2) + 0.5), yaw += k pi/2, w <-> l swapped when k is odd.
 *   correct_yaw == 2: CenterPointBBoxCoderRev.decode instead (centerpoint_bbox_coders.py:87-112): preds rows
 *   [dx, dy, z, dim x3, sin, cos, others...], c >= 8, rot = atan2(sin, cos), out (n, c - 1); no backward.
 *   num_rot_parity (n) int32, nullable: receives k & 1 (what the backward needs).
 * coder_center_decode_backward: grad_preds (n,c) from grad_out (n, out cols), `out` of the forward and the parity
 *   flags (NULL = no swap); the sin / cos columns receive 0 (k is computed under no_grad in the reference).
 * coder_center_encode: boxes (n,c) [x,y,z,w,l,h,yaw, others] -> out (n,c+2) [first 7, sin yaw, cos yaw, others].
 * ---------------------------------------------------------------------------------- */
int coder_center_decode(const gd3d_prologue* coder, const float* locs, const float* preds, int64_t n,
                        int32_t c, int32_t correct_yaw, float* out, int32_t* num_rot_parity, void* stream);

int coder_center_decode_backward(const gd3d_prologue* coder, const float* grad_out, const float* out,
                                 const int32_t* num_rot_parity, int64_t n, int32_t c,
                                 float* grad_preds, void* stream);

int coder_center_encode(const float* boxes, int64_t n, int32_t c, float* out, void* stream);

/* PointBBoxYawCoder.decode (/root/reference/mmdet3d_gaussian/core/bbox/coders/point_bbox_yaw_coders.py:19-52) and its backward
 * wrt preds.  priors (n,3) [px, py, scale]; preds (n,c) [dx, dy, z, log dims x3, yaw, sin dir, cos dir, others], c >= 7
 * (>= 9 with correct_yaw = 1); out (n, 7 + max(c - 9, 0)) = [dx scale + px, dy scale + py, z, exp(dims) (first two x scale),
 * yaw, others]; correct_yaw = 1: yaw snapped by whole quarter turns towards atan2(sin, cos), w <-> l on odd turns;
 * num_rot_parity (n) nullable: parity of the turns for the backward.  encode (:12-16) is coder_center_encode. */
int coder_point_decode(const float* priors, const float* preds, int64_t n, int32_t c, int32_t correct_yaw, float* out,
                       int32_t* num_rot_parity, void* stream);
int coder_point_decode_backward(const float* priors, const float* grad_out, const float* out,
                                const int32_t* num_rot_parity, int64_t n, int32_t c, float* grad_preds, void* stream);

/* The decode in front of PVRCNNBboxHead.get_bboxes' NMS (/root/reference/mmdet3d_gaussian/models/roi_heads/bbox_heads/pvrcnn_bbox_head.py:
 * 376-386, with mmdet3d's DeltaXYZWLHRBBoxCoder.decode and rotation_3d_in_axis, third party): rois (n, roi_stride) with the box
 * [x, y, z, dx, dy, dz, yaw] at columns first_col .. first_col + 6 (1 for the head's [batch_id, box] rows), bbox_pred (n, 7) residuals
 * -> boxes (n, 7) and, if not NULL, bev_xyxyr (n, 5) = [x - dx/2, y - dy/2, x + dx/2, y + dy/2, yaw] as multi_class_nms builds it (:447-448).
 * clockwise = 0: the centre is turned counter-clockwise by the roi's yaw (mmdet3d 1.0); 1: the transpose (0.x). */
int coder_roi_decode(const float* rois, int32_t roi_stride, int32_t first_col, const float* bbox_pred, int64_t n,
                     int32_t clockwise, float* boxes, float* bev_xyxyr, void* stream);

/* Second stage of the reduction on its own: *loss_sum = fixed-order fp64 sum of the per-workgroup
 * partials that gd3d_loss_fused(..., workspace != NULL) left in `workspace` for the same n.
 * gd3d_loss_fused calls it itself when loss_sum != NULL; it is exported so that a caller can
 * bracket the fused kernel alone with events (bench.py) or defer the scalar. */
int gd3d_loss_reduce(const void* workspace, int64_t n, float* loss_sum, void* stream);

/* In-place row scaling used by autograd backward when the upstream gradient is not 1:
 *   grad[i,:] *= (per_row ? g[i] : g[0]),  grad is (n,7) fp32, g is DEVICE memory.
 * With per_row == 0 the kernel reads g[0] first and exits without touching grad when it is
 * exactly 1.0f, so the common `loss.backward()` costs one empty launch and no HBM traffic
 * and no host sync.  (Replaces the autograd mul nodes of `* self.loss_weight`, :310.) */
int gd3d_scale_rows(float* grad, const float* g, int per_row, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------
 * `_cpu` twins: the same contracts on HOST memory, no stream, no HIP call — they run on a machine
 * without a GPU.  The reference's GDLoss.forward is device-agnostic (gaussian_distance_loss.py:280-310: the same op chain
 * on CPU tensors, BASELINE configs[0]); these entry points are what a CPU tensor takes in this library.  They evaluate the
 * kernel's own per-pair closed forms and hand-derived gradients (csrc/gd3d_device.h compiled for the host), one pass,
 * loss and final gradients together, over `nthreads` host threads (<= 0: std::thread::hardware_concurrency()).
 *   gd3d_loss_fused_cpu : contract of gd3d_loss_fused_w7 (row_weight / weight7 mutually exclusive, n == 0 legal).
 *       workspace: gd3d_loss_workspace_bytes(n) bytes of host memory, required when loss_sum != NULL; whenever given it
 *       receives one fp32 partial per 256-pair tile (fp64 accumulation in row order, rounded once).  *loss_sum = the
 *       fixed-order fp64 sum of those partials, rounded to fp32: independent of nthreads.
 *   gd3d_loss_reduce_cpu: the second stage alone (twin of gd3d_loss_reduce).
 *   gd3d_scale_rows_cpu : twin of gd3d_scale_rows (g is host memory; per_row == 0 and g[0] == 1 touches nothing).
 * The bbox-coder prologues (gd3d_loss_fused_decoded) have no CPU twin: the head-level fusions are GPU-only.
 * ---------------------------------------------------------------------------------- */
int gd3d_loss_fused_cpu(const gd3d_params* params, const float* pred, const float* target,
                        const float* row_weight, const float* weight7, int64_t n, float scale,
                        float* loss, float* loss_sum, float* grad_pred, float* grad_target,
                        void* workspace, int32_t nthreads);
int gd3d_loss_reduce_cpu(const void* workspace, int64_t n, float* loss_sum);
int gd3d_scale_rows_cpu(float* grad, const float* g, int per_row, int64_t n, int32_t nthreads);

/* `_cpu` twins of the rotated-box entry points (declared further down): csrc/rbox_device.h — the geometry of the GPU kernels,
 * every step one IEEE fp32 operation in a fixed order — compiled for the host with the same -ffp-contract=off, so results
 * are BIT-IDENTICAL to the HIP kernels'.  Host memory, no stream, no workspace.  The reference's own pairwise IoU helpers are
 * CPU code (ops/eval/affinity.cpp:8-105); rnms_*_cpu are the greedy scan on one thread (decisions of rnms_bev /
 * rnms_normal_bev; mmdet3d's nms_gpu itself has no CPU form).  nthreads <= 0: std::thread::hardware_concurrency(). */
int riou_bev_xyxyr_cpu(const float* a, int64_t na, const float* b, int64_t nb, float* iou, int32_t nthreads);
int riou_eval_bev_cpu(const float* det, int64_t nd, const float* gt, int64_t ng, float* iou, int32_t nthreads);
int riou_eval_3d_cpu(const float* det, int64_t nd, const float* gt, int64_t ng, float z_offset, float* iou, int32_t nthreads);
int riou_eval_trans_bev_cpu(const float* det, int64_t nd, int32_t det_cols, const float* gt, int64_t ng, int32_t gt_cols,
                            float* dist, int32_t nthreads);
int rnms_bev_cpu(const float* boxes_sorted, int64_t n, float thresh, int64_t* keep, int64_t* num_keep);
int rnms_normal_bev_cpu(const float* boxes_sorted, int64_t n, float thresh, int64_t* keep, int64_t* num_keep);

/* ------------------------------------------------------------------------------------
 * Rotated BEV NMS.  Replaces mmdet3d `iou3d_cuda.nms_gpu(boxes, keep, thresh, device)`
 * behind `nms_gpu(boxes, scores, thresh, pre_max_size, post_max_size)`
 * (call sites gd_centerpoint_head.py:340-345, pvrcnn_bbox_head.py:463-464).
 *   boxes_sorted : (n,5) fp32 [x1,y1,x2,y2,ry], ALREADY sorted by descending score
 *   keep         : (n) int64, receives indices into boxes_sorted, ascending
 *   num_keep     : (1) int64; -1 (every rnms_* entry, per group): the device-side scan gave
 *                  up — a wave of the list scan stopped making progress and its bounded
 *                  polling loop ended (never observed; the host layer raises on it).
 *                  Every rnms_* entry writes each num_keep word EXACTLY ONCE, with the kernel
 *                  that resolves the group's last box: the pointer may be device-visible PINNED
 *                  HOST memory that the caller pre-sets to a sentinel and polls instead of
 *                  copying the count back (what nms_gpu does: iou3d.py, _host.launch_counted).
 * Greedy: box i is kept iff no kept j < i has IoU_bev(j,i) > thresh.  The suppression
 * bit-mask (n x ceil(n/64) uint64), from 768 boxes on also per-box victim lists, and the
 * greedy scan all stay on the device; nothing in the workspace needs initialising.
 * rnms_normal_bev: same with axis-aligned IoU (mmdet3d nms_normal_gpu; angle ignored).
 * ---------------------------------------------------------------------------------- */
size_t rnms_workspace_bytes(int64_t n);

int rnms_bev(const float* boxes_sorted, int64_t n, float thresh, int64_t* keep,
             int64_t* num_keep, void* workspace, void* stream);

int rnms_normal_bev(const float* boxes_sorted, int64_t n, float thresh, int64_t* keep,
                    int64_t* num_keep, void* workspace, void* stream);

/* The whole `nms_gpu` body in one call for up to rnms_scored_max_n() (= 16384) candidates — the heads cut to nms_pre
 * before they call it.  The score order (descending, ties by ascending index, NaN first: what
 * torch.sort(descending=True, stable=True) yields) is obtained by COUNTING, for every box, the boxes with a larger
 * (score, -index) key — parallel over the whole chip, no sort — and the per-box prep is scattered straight to its rank;
 * the `pre_max` cut (pre_max < 0: none) keeps ranks < pre_max.  Mask and scan follow as in rnms_bev_ordered.
 *   boxes (n_all,5) fp32, scores (n_all) fp32; keep (min(n_all, pre_max)) int64 receives indices into `boxes` by
 *   descending score; num_keep (1) int64; workspace: rnms_scored_workspace_bytes(n_all, min(n_all, pre_max)).
 *   normal != 0: axis-aligned IoU (nms_normal_gpu).  n_all > rnms_scored_max_n(): GD3D_E_TOOLARGE (sort outside and
 *   call rnms_bev_ordered). */
int rnms_scored_max_n(void);
size_t rnms_scored_workspace_bytes(int64_t n_all, int64_t n_keep);
int rnms_scored(int32_t normal, const float* boxes, const float* scores, int64_t n_all, int64_t pre_max, float thresh,
                int64_t* keep, int64_t* num_keep, void* workspace, void* stream);

/* Same, taking the UNSORTED boxes plus the score order (what `scores.sort(descending=True)` returns, already cut to
 * pre_max_size): box i of the NMS is boxes[order[i]], and `keep` receives indices into the caller's original box
 * numbering (= order[kept]) — the gather before and the index mapping after the call disappear.
 *   boxes (any number of rows >= max(order)+1, 5) fp32;  order (n) int64;  keep (n) int64;  num_keep (1) int64. */
int rnms_bev_ordered(const float* boxes, const int64_t* order, int64_t n, float thresh, int64_t* keep,
                     int64_t* num_keep, void* workspace, void* stream);

int rnms_normal_bev_ordered(const float* boxes, const int64_t* order, int64_t n, float thresh,
                            int64_t* keep, int64_t* num_keep, void* workspace, void* stream);

/* G independent NMS problems in ONE set of launches (classes of a multi-class NMS, pvrcnn_bbox_head.py:452-477; the
 * samples / tasks a head loops over, gd_centerpoint_head.py:322-345): all groups index the same box array.
 *   mode     : 0 rotated BEV IoU (nms_gpu), 1 axis-aligned IoU (nms_normal_gpu), 2 circle (below; boxes is (N,2));
 *   order    : (groups, cap) int64, row g = box indices of group g by descending score; only its first counts[g] used;
 *   counts   : (groups) int32 ON THE DEVICE — group sizes are data dependent (score thresholds), reading them in the
 *              kernels removes the per-group host sync the reference loop pays; values are clamped to [0, cap];
 *   thresh   : (groups) fp32 on the device (per-class thresholds);
 *   keep     : (groups, cap) int64, row g receives the kept box indices (caller's numbering) in score order;
 *   num_keep : (groups) int64.   workspace: rnms_batched_workspace_bytes(groups, cap).
 * Each group's result equals the single call on that group (same kernels, blockIdx.y = group). */
size_t rnms_batched_workspace_bytes(int32_t groups, int64_t cap);

int rnms_batched(int32_t mode, const float* boxes, const int64_t* order, const int32_t* counts,
                 int32_t groups, int64_t cap, const float* thresh, int64_t* keep, int64_t* num_keep,
                 void* workspace, void* stream);

/* rnms_batched (mode 0) for a caller INSIDE the library that has already written the oriented boxes: the first counts[g]
 * entries of row g of a (groups, cap) array of 64-byte records (csrc/rbox_device.h `OBox`, made by `obox_make` from the
 * [x1,y1,x2,y2,ry] rows in score order) at the start of `workspace`.  Saves the preparation launch; center_infer.hip's
 * selection kernel writes the records while it compacts its survivors. */
int rnms_batched_prepared(const float* boxes, const int64_t* order, const int32_t* counts, int32_t groups,
                          int64_t cap, const float* thresh, int64_t* keep, int64_t* num_keep,
                          void* workspace, void* stream);

/* rnms_batched with the score order taken inside the library (rank by counting, as rnms_scored), so the caller needs no
 * masked_fill / sum / sort passes:
 *   scores (groups, n) fp32;  valid (groups, n) bytes, nullable — which boxes take part in group g;  pre_max < 0: none.
 *   Group g runs NMS over its valid boxes by descending score (ties by ascending index), cut to cap = min(n, pre_max).
 *   keep (groups, cap) int64 indices into `boxes`; num_keep (groups) int64; thresh (groups) fp32, DEVICE.
 *   n <= rnms_scored_max_n(), else GD3D_E_TOOLARGE.  workspace: rnms_batched_scored_workspace_bytes(groups, n, cap). */
size_t rnms_batched_scored_workspace_bytes(int32_t groups, int64_t n, int64_t cap);
int rnms_batched_scored(int32_t mode, const float* boxes, const float* scores, const uint8_t* valid, int32_t groups,
                        int64_t n, int64_t pre_max, const float* thresh, int64_t* keep, int64_t* num_keep,
                        void* workspace, void* stream);

/* rnms_batched_scored over several box sets in one set of launches (ABI 4): `sets` x groups_per_set groups, group g working on the
 * n boxes of set g / groups_per_set = rows [set n, (set + 1) n) of boxes (sets n, 5) — the per-sample class problems of a whole
 * batch (box3d_multiclass_nms of every sample at once).  scores / valid (sets groups_per_set, n), thresh (sets groups_per_set) on the
 * device; keep holds indices into the flat box array (set n + i).  workspace: rnms_batched_scored_workspace_bytes(sets
 * groups_per_set, n, cap).  Each group's result equals rnms_batched_scored on its own set. */
int rnms_batched_scored_sets(int32_t mode, const float* boxes, const float* scores, const uint8_t* valid, int32_t sets,
                             int32_t groups_per_set, int64_t n, int64_t pre_max, const float* thresh, int64_t* keep,
                             int64_t* num_keep, void* workspace, void* stream);

/* The same for G problems that each own a CONTIGUOUS run of one flat box / score array (the per-sample x per-task NMS
 * calls of CenterHeadRev.get_bboxes, gd_centerpoint_head.py:233-345, concatenated): group g = boxes [seg[g], seg[g+1]).
 * Every group ranks only its own slice — O(sum n_g^2) key compares, where the dense (G, N) form above would compare every
 * key in every group.
 *   scores (N_total) fp32;  seg (groups+1) int32 on the DEVICE, ascending;  max_seg >= every group size (host value:
 *   the caller knows the sizes from its tensor shapes), <= rnms_scored_max_n();  cap = min(max_seg, pre_max).
 *   keep (groups, cap) int64 GLOBAL indices into `boxes`; num_keep (groups) int64.
 *   workspace: rnms_batched_scored_workspace_bytes(groups, max_seg, cap). */
int rnms_segmented_scored(int32_t mode, const float* boxes, const float* scores, const int32_t* seg, int32_t groups,
                          int64_t max_seg, int64_t pre_max, const float* thresh, int64_t* keep, int64_t* num_keep,
                          void* workspace, void* stream);

/* Circle NMS (mmdet3d `circle_nms(dets, thresh, post_max_size)`, numba, CPU; the reference copies the detections
 * D->H for it, gd_centerpoint_head.py:256-272): centres xy (rows, 2) fp32, order (n) by descending score; box j is
 * suppressed by a kept i before it iff (x_i-x_j)^2 + (y_i-y_j)^2 <= thresh (fp32 distance, float64 compare; note
 * the published code compares the SQUARED distance with the radius as given).  keep/num_keep as rnms_bev_ordered;
 * workspace: rnms_workspace_bytes(n). */
int rnms_circle_ordered(const float* xy, const int64_t* order, int64_t n, double thresh,
                        int64_t* keep, int64_t* num_keep, void* workspace, void* stream);

/* Pairwise rotated BEV IoU in the NMS box format (mmdet3d `boxes_iou_bev`):
 *   a (na,5), b (nb,5) [x1,y1,x2,y2,ry] -> iou (na,nb) fp32 row-major. */
int riou_bev_xyxyr(const float* a, int64_t na, const float* b, int64_t nb, float* iou,
                   void* stream);

/* Pairwise rotated IoU of 7-dof boxes (x,y,z,w,h,l,yaw), the reference's CPU eval helpers
 *   /root/reference/mmdet3d_gaussian/ops/eval/affinity.cpp:8-49  (iou_3d, z_offset)
 *   /root/reference/mmdet3d_gaussian/ops/eval/affinity.cpp:51-81 (iou_bev)
 * built on rotated_boxes_intersection (ops/eval/rbox_utils.hpp:280-302).
 *   det (nd,7), gt (ng,7) -> iou (nd,ng) fp32 row-major. */
int riou_eval_bev(const float* det, int64_t nd, const float* gt, int64_t ng, float* iou,
                  void* stream);

int riou_eval_3d(const float* det, int64_t nd, const float* gt, int64_t ng, float z_offset,
                 float* iou, void* stream);

/* BEV centre distance (affinity.cpp:83-105, `LidarCenterTransBEV`): det (nd, det_cols), gt (ng, gt_cols) row-major,
 * columns 0 and 1 are the centre -> dist (nd, ng) fp32 = sqrt(dx^2 + dy^2). */
int riou_eval_trans_bev(const float* det, int64_t nd, int32_t det_cols, const float* gt, int64_t ng,
                        int32_t gt_cols, float* dist, void* stream);

/* COCO-style greedy matcher (matcher.cpp:8-74, `MatcherCoCo`), all on the device:
 *   cost (nd, ng) fp32 row-major (e.g. the negated IoU matrix the kernels above wrote), cost_thrs (nt) fp32,
 *   is_ignore / is_crowd (ng) bytes (0/1)  ->  matched (nt, nd) int32: gt index or -1.
 * For every threshold the detections are visited in row order; a detection takes the cheapest gt with cost <= thr
 * that is still free (or a crowd gt), a non-ignore gt beating any ignore gt, ties going to the later gt.  Bit-exact
 * with the reference (integer output).  ng <= 1048576. */
int eval_match_coco(const float* cost, const float* cost_thrs, const uint8_t* is_ignore,
                    const uint8_t* is_crowd, int64_t nd, int64_t ng, int64_t nt, int32_t* matched,
                    void* stream);
/* `_cpu` twin (ABI 6): the same contract on HOST memory — the reference's matcher IS CPU code (matcher.cpp:8-74, numpy in
 * and out), so an evaluation without a GPU keeps working.  Thresholds are spread over `nthreads` std::threads (<= 0: hardware
 * concurrency).  Same integers as the kernel and as the reference. */
int eval_match_coco_cpu(const float* cost, const float* cost_thrs, const uint8_t* is_ignore,
                        const uint8_t* is_crowd, int64_t nd, int64_t ng, int64_t nt, int32_t* matched,
                        int32_t nthreads);

/* ------------------------------------------------------------------------------------
 * Flexible mAP: the records of a matcher result and the AP of every (group, threshold) over all records (an addition inside
 * ABI 6; csrc/eval_ap.hip).  Replaces, above eval_match_coco, what
 * /root/reference/mmdet3d_gaussian/core/evaluation/mean_ap_flexible.py does per frame (:98-126) and per dataset (:130-148, with
 * mmdet's average_precision(mode='area')).  A group is one (class, breakdown) pair; a record is one detection of one group.
 *
 * eval_tp_records: matched (T, D) int32 as eval_match_coco wrote it, or NULL: no match at all (the empty branch, :98-104);
 *   det_flag (D) and gt_flag (G >= 0) bytes: the detection / the gt lies in the breakdown; score (D) fp32; 1 <= T <= 32.
 *   Writes D rows of four columns, each pointer at the row where the caller's block starts:
 *     group = `group`, score = a copy, and with m = matched[t, d] (a value outside [-1, G) counts as -1; nothing is read out of range)
 *     bit t of tp_bits  = m > -1,
 *     bit t of msk_bits = (det_flag[d] && m == -1) || (m > -1 && gt_flag[m]).
 *   One launch.
 *
 * eval_ap_accumulate: n records (n <= 2^31 - 1) in four columns, num_gt (K) int64, 1 <= K <= 2^20, 1 <= T <= 32
 *   -> num_det (K, T) int64, recall (K, T) fp64, ap (K, T) fp64.
 *   Rank order inside a group: descending score; equal scores (-0 == +0) in ascending row index; NaN scores first, among
 *   themselves in ascending row index.  (numpy's reversed argsort with the ties made definite.)
 *   A row whose group is outside [0, K) counts for nothing: that is how a static record buffer is padded.
 *   For group g and threshold t take the rows of g whose msk bit t is set, in rank order, numbered j = 1..D:
 *     h_j = the row's tp bit t (a tp bit on a row whose msk bit is clear is ignored);   c_j = h_1 + ... + h_j;
 *     p_j = c_j / j, ONE IEEE fp64 division of the two integers;                        e_j = max over i >= j of p_i;
 *     den = num_gt[g] > 0 ? (double)num_gt[g] : 1e-7      (the reference's max(num_gt, 1e-7));
 *     num_det = D;   recall = D ? (double)c_D / den : 0;   ap = S / den,
 *   where S is the sum of e_j over the rows with h_j, taken EXACTLY and rounded to fp64 once, to nearest even: every such e_j is a
 *   fp64 in [2^-31, 1], a whole number of 2^-84, so the sum is an integer below 2^116 of those units; it is added in integers (the
 *   order is immaterial) and only the total is rounded.  ap therefore carries two roundings, whatever n is.
 *   No read-back, no float atomic, static shapes, capturable on one stream.  workspace: eval_ap_workspace_bytes(n, K, T) bytes,
 *   256-byte aligned (the same carve at address 0; 0 for arguments out of range).
 *   eval_ap_tile_rows(): sorted rows per workgroup of the scan kernels; eval_ap_scan_chunk_tiles(): tiles per iteration of the
 *   carry scans between tiles (a loop: no capacity, another trip every that many tiles). */
int eval_tp_records(const int32_t* matched, const uint8_t* det_flag, const uint8_t* gt_flag, const float* score, int32_t group,
                    int64_t D, int64_t G, int32_t T, int32_t* out_group, float* out_score, uint32_t* out_tp_bits,
                    uint32_t* out_msk_bits, void* stream);
int32_t eval_ap_tile_rows(void);
int32_t eval_ap_scan_chunk_tiles(void);
size_t eval_ap_workspace_bytes(int64_t n, int64_t K, int32_t T);
int eval_ap_accumulate(const int32_t* group, const float* score, const uint32_t* tp_bits, const uint32_t* msk_bits,
                       const int64_t* num_gt, int64_t n, int64_t K, int32_t T, int64_t* num_det, double* recall, double* ap,
                       void* workspace, void* stream);
/* `_cpu` twins (csrc/eval_ap_cpu.cpp): the same contracts on HOST memory, plain loops over a stable sort; the same bits in all three
 * outputs.  (group, threshold) pairs are spread over `nthreads` std::threads (<= 0: hardware concurrency). */
int eval_tp_records_cpu(const int32_t* matched, const uint8_t* det_flag, const uint8_t* gt_flag, const float* score, int32_t group,
                        int64_t D, int64_t G, int32_t T, int32_t* out_group, float* out_score, uint32_t* out_tp_bits,
                        uint32_t* out_msk_bits);
int eval_ap_accumulate_cpu(const int32_t* group, const float* score, const uint32_t* tp_bits, const uint32_t* msk_bits,
                           const int64_t* num_gt, int64_t n, int64_t K, int32_t T, int64_t* num_det, double* recall, double* ap,
                           int32_t nthreads);

/* Flexible mAP, a batch of frames: every record of every (frame, class) problem, breakdown row and threshold of a batch in a FIXED
 * number of launches (an addition inside ABI 6; csrc/eval_frames.hip).  What the affinity entry
 * (riou_eval_3d / riou_eval_bev / riou_eval_trans_bev), eval_match_coco and eval_tp_records give when they are called once per
 * problem and breakdown row, and the same bits.
 *
 * eval_frames_records:
 *   mode: 0 riou_eval_3d with z_offset, 1 riou_eval_bev, 2 riou_eval_trans_bev.  negate != 0: the matcher sees -affinity and -thrs
 *   (what BaseMatcher.__call__ does for LARGER_CLOSER affinities; the negation is exact).
 *   Problem p in [0, P) owns the detection rows [det_seg[p], det_seg[p+1]) of det (ND, 7) and score (ND), ALREADY in the problem's
 *   rank order, and the gt rows [gt_seg[p], gt_seg[p+1]) of gt (NG, 7): D_p and G_p rows.  det_seg, gt_seg (P + 1) int32 ascending from
 *   0 to ND / NG; pair_off (P + 1) int64: the prefix sums of D_p * G_p, pairs = pair_off[P]; max_gt >= every G_p.  These tables are
 *   DEVICE memory for the device entry; their contents are known to the host from shapes alone.
 *   gt_crowd (NG) bytes or NULL (no crowd gt).  det_flag (R, ND), gt_flag (R, NG) bytes: the box lies in breakdown row b (ignored gts
 *   already cleared).  group (P, R) int32: the record group of problem p's row b, or -1 where the row does not apply to the problem.
 *   thrs (T) fp32.  1 <= T <= 32, R >= 1, P >= 0.
 *   Writes R * ND rows of four columns, each pointer at the row where the caller's block starts; the row of (b, detection row i) is
 *   b * ND + i.  For i in problem p: group = group[p, b]; score = a copy of score[i]; and with
 *     matched = eval_match_coco(cost_p, thrs, is_ignore = !gt_flag[b, p's gts], is_crowd = gt_crowd or zeros)
 *   bit t of tp_bits and msk_bits is what eval_tp_records(matched, det_flag[b], gt_flag[b], ...) writes; G_p == 0 takes its no-match
 *   branch (matched NULL); D_p == 0 has no rows.  A row with group[p, b] == -1 gets group -1, the score copy and zero bits: nothing is
 *   matched for it.
 *   alias_tp != 0: the tp_bits of every row (b, i) of problem p with group[p, b] >= 0 are those of (b_last, i), b_last the largest b
 *   with group[p, b] >= 0 — the reference's one-cls_tp-array aliasing (mean_ap_flexible.py:90, :115-116, :124-126).  They are written
 *   from the last row's matcher result, never copied: no race.
 *   Limits: max_gt <= 2048, pairs, R * ND and P * R * T <= 2^31 - 1: GD3D_E_TOOLARGE beyond.  Null pointers with non-zero sizes, T
 *   or mode out of range, R < 1: GD3D_E_BADARG.  Whatever the tables hold, nothing is read or written out of range.
 *   THREE launches (pair affinities; matcher, one wave per (problem, row, threshold); records), whatever P, R, T and the frames are;
 *   a batch with pairs == 0 runs the records launch alone.  No host read, no atomic, static shapes, capturable on one stream.
 *   workspace: eval_frames_workspace_bytes(ND, pairs, R, T) bytes, 256-byte aligned (the same carve at address 0; 0 for arguments
 *   out of range); its contents need not be cleared between calls. */
int eval_frames_records(int32_t mode, float z_offset, int32_t negate, const float* det, const float* score, const int32_t* det_seg,
                        int64_t ND, const float* gt, const int32_t* gt_seg, int64_t NG, const uint8_t* gt_crowd,
                        const int64_t* pair_off, int64_t pairs, int64_t max_gt, const uint8_t* det_flag, const uint8_t* gt_flag,
                        const int32_t* group, const float* thrs, int32_t P, int32_t R, int32_t T, int32_t alias_tp, int32_t* out_group,
                        float* out_score, uint32_t* out_tp_bits, uint32_t* out_msk_bits, void* workspace, void* stream);
size_t eval_frames_workspace_bytes(int64_t ND, int64_t pairs, int32_t R, int32_t T);
/* `_cpu` twin (csrc/eval_frames_cpu.cpp): the same contract on HOST memory; the problems are spread over `nthreads` std::threads
 * (<= 0: hardware concurrency) and each runs the existing `_cpu` twins, so all four columns carry the same bits.  The tables are
 * host memory here, so tables that contradict ND, NG, pairs or max_gt are refused with GD3D_E_BADARG. */
int eval_frames_records_cpu(int32_t mode, float z_offset, int32_t negate, const float* det, const float* score, const int32_t* det_seg,
                            int64_t ND, const float* gt, const int32_t* gt_seg, int64_t NG, const uint8_t* gt_crowd,
                            const int64_t* pair_off, int64_t pairs, int64_t max_gt, const uint8_t* det_flag, const uint8_t* gt_flag,
                            const int32_t* group, const float* thrs, int32_t P, int32_t R, int32_t T, int32_t alias_tp,
                            int32_t* out_group, float* out_score, uint32_t* out_tp_bits, uint32_t* out_msk_bits, int32_t nthreads);

/* ------------------------------------------------------------------------------------
 * Dynamic point-to-voxel scatter-reduce.  Replaces
 * dynamic_point_to_voxel_scatter_reduce / dynamic_point_to_voxel_backward
 * (/root/reference/mmdet3d_gaussian/ops/voxel/src/voxelization.h:35-79,
 *  src/scatter_points_cuda.cu:183-321) behind ops/voxel/scatter.py:29-72.
 *   feats (n,c) fp32; map (n) int32 point->voxel (-1 = dropped point); count (v) int32 points per voxel;
 *   order (n_valid...) int32: point ids grouped by voxel in ascending point id (stable argsort of map, with the
 *   -1 entries skipped by seg[0]); seg (v+1) int32 segment bounds into `order`.
 *   reduce: GD3D_REDUCE_* = the reference's reduce_t (voxelization.h:4).
 * vox_scatter_reduce : out (v,c) = max | mean | sum over the voxel's points; argmax (v,c) int32 (max only,
 *                      nullable) receives the smallest point id attaining the max.
 * vox_scatter_backward: grad_feats (n,c): sum -> grad_vox[map[i]], mean -> / count, max -> routed to argmax,
 *                      0 elsewhere (the kernel zero-fills).  Deterministic, no float atomics.
 * ---------------------------------------------------------------------------------- */
enum { GD3D_REDUCE_SUM = 0, GD3D_REDUCE_MEAN = 1, GD3D_REDUCE_MAX = 2 };

int vox_scatter_reduce(const float* feats, const int32_t* order, const int32_t* seg, int64_t n,
                       int32_t c, int64_t v, int reduce, float* out, int32_t* argmax, void* stream);

int vox_scatter_backward(const float* grad_vox, const int32_t* map, const int32_t* count,
                         const int32_t* argmax, int64_t n, int32_t c, int64_t v, int reduce,
                         float* grad_feats, void* stream);

/* From point coordinates to the index structures above, in one stream-ordered call (ABI 3; replaces ~20 framework launches:
 * per-column extents, one mixed-radix int64 key per point, a stable radix sort of (key, point id), run heads -> voxel ids).
 *   coors (n, ndim) int32, ndim <= 8; a point with ANY negative coordinate is dropped (scatter_points_cuda.cu:236-246).
 * Outputs, caller-allocated at their UPPER bounds (every point a voxel of its own):
 *   point2voxel_map (n) int32 (-1 = dropped);  order (n) int32: point ids grouped by voxel, ascending inside a voxel, the
 *   dropped points first;  seg (n + 1) int32: seg[v] .. seg[v+1] = voxel v's run in `order` (seg[0] = dropped points);
 *   counts (n) int32;  voxel_coors (n, ndim) int32: the sorted unique rows (lexicographic = the reference's unique_dim order,
 *   samples in batch order);  num (2) int64 on the DEVICE: [number of voxels V, number of dropped points] — the one thing
 *   the host has to read back before it can cut voxel_coors / counts / seg to V rows.
 *   workspace: vox_index_workspace_bytes(n, ndim) bytes, 256-byte aligned (0 is returned if the query itself fails). */
size_t vox_index_workspace_bytes(int64_t n, int32_t ndim);
int vox_index_build(const int32_t* coors, int64_t n, int32_t ndim, void* workspace,
                    int32_t* point2voxel_map, int32_t* order, int32_t* seg, int32_t* counts,
                    int32_t* voxel_coors, int64_t* num, void* stream);

/* Same gradient, produced in VOXEL order from the forward's grouping (order, seg as in vox_scatter_reduce): each voxel's
 * gradient row is read once and streamed to its points, instead of being re-gathered once per point — about half the
 * HBM traffic of the map-ordered form.  Points in no voxel (the prefix order[0 .. seg[0])) receive zeros.
 * Any c <= 128 (rows staged through LDS and written as a flat dword stream), or c % 4 == 0, c <= 256 with 16-byte aligned
 * grad_vox / grad_feats / argmax; GD3D_E_BADARG otherwise: use vox_scatter_backward. */
int vox_scatter_backward_grouped(const float* grad_vox, const int32_t* order, const int32_t* seg,
                                 const int32_t* argmax, int64_t n, int32_t c, int64_t v, int reduce,
                                 float* grad_feats, void* stream);

/* ------------------------------------------------------------------------------------
 * Voxel-set-abstraction ops of PV-RCNN (an addition inside ABI 6): stacked ball query, point grouping forward / backward,
 * the two fused into one launch, and furthest point sampling.  Replace the reference's own CUDA extension
 *   /root/reference/mmdet3d_gaussian/ops/vsa/src/ball_query.cu:12-72 (ball_query_kernel),
 *   src/group_points.cu:14-49 (group_points_grad_kernel), :52-90 (group_points_kernel),
 *   src/sampling.cu:22-152 (furthest_point_sampling_kernel)
 * behind ops/vsa/group_points.py (BallQuery :7-39, GroupingOperation :42-94, QueryAndGroup :97-183) and
 * ops/vsa/sample_points.py:7-33.
 *
 * Stacked data: xyz (N,3) fp32 = the points of B samples one after another, xyz_batch_cnt (B) int32 their counts; new_xyz (M,3)
 * fp32 the query centres with new_xyz_batch_cnt (B) int32.  A query sees the points of its own sample only and every index is
 * LOCAL to the sample.  The kernels find the samples' start offsets from the count arrays themselves (no host prefix sum, no
 * host read).  Nothing validates the counts on the host; instead every count is clamped to [0, rows left in the array] and
 * every gathered index to [0, points of its sample), so inconsistent counts or indices cannot read or write outside the
 * buffers.  Query rows that the counts do not cover are empty balls (forward) and pass no gradient (backward).
 *
 * Ball query: radius2 = radius * radius (fp32); walking the sample's points in ascending index,
 *   d2 = (nx-x)*(nx-x) + (ny-y)*(ny-y) + (nz-z)*(nz-z)   fp32, left to right, no fma contraction;
 * the first nsample points with d2 < radius2 (strict) fill idx[m,:], the slots past the member count repeat the first member;
 * an empty ball gives idx[m,:] = 0 and empty_mask[m] = 1.  cnt[m] = min(members, nsample).  idx (M,nsample) int32; cnt (M)
 * int32 and empty_mask (M) bytes are nullable.  1 <= nsample <= 1024, else GD3D_E_TOOLARGE.
 * ---------------------------------------------------------------------------------- */
int gd3d_vsa_ball_query(const float* xyz, const int32_t* xyz_batch_cnt, const float* new_xyz,
                        const int32_t* new_xyz_batch_cnt, int32_t B, int64_t N, int64_t M, float radius,
                        int32_t nsample, int32_t* idx, int32_t* cnt, uint8_t* empty_mask, void* stream);

/* Grouping: out[m, c, s] = features[start_b + idx[m, s], c], features (N,C) fp32, out (M,C,nsample) (a sample without points
 * gives zeros).  Backward: grad_features[start_b + idx[m, s], c] += grad_out[m, c, s]; grad_features (N,C) is zero-filled
 * by the call.  The sums are float atomics: the last bits depend on the order of arrival, as with the reference's atomicAdd. */
int gd3d_vsa_group(const float* features, const int32_t* features_batch_cnt, const int32_t* idx,
                   const int32_t* idx_batch_cnt, int32_t B, int64_t N, int64_t M, int32_t C, int32_t nsample,
                   float* out, void* stream);
int gd3d_vsa_group_backward(const float* grad_out, const int32_t* idx, const int32_t* idx_batch_cnt,
                            const int32_t* features_batch_cnt, int32_t B, int64_t N, int64_t M, int32_t C,
                            int32_t nsample, float* grad_features, void* stream);

/* QueryAndGroup.forward in ONE launch: the ball query, then out (M, (use_xyz ? 3 : 0) + C, nsample) = [grouped xyz minus the
 * query centre (use_xyz), grouped features (features != NULL, C > 0)], every channel of an empty ball zero.  idx / cnt /
 * empty_mask as gd3d_vsa_ball_query (idx required).  Its backward wrt features reads grad_out (M, c_off + C, nsample) from
 * channel c_off (0 or 3) on; the padded slots s >= cnt[m] all name the first member and are summed before ONE add; rows with
 * cnt[m] == 0 pass nothing.  grad_features (N,C) is zero-filled by the call. */
int gd3d_vsa_query_and_group(const float* xyz, const int32_t* xyz_batch_cnt, const float* new_xyz,
                             const int32_t* new_xyz_batch_cnt, const float* features, int32_t B, int64_t N,
                             int64_t M, int32_t C, float radius, int32_t nsample, int32_t use_xyz, float* out,
                             int32_t* idx, int32_t* cnt, uint8_t* empty_mask, void* stream);
int gd3d_vsa_query_and_group_backward(const float* grad_out, const int32_t* idx, const int32_t* cnt,
                                      const int32_t* new_xyz_batch_cnt, const int32_t* xyz_batch_cnt, int32_t B,
                                      int64_t N, int64_t M, int32_t C, int32_t nsample, int32_t c_off,
                                      float* grad_features, void* stream);

/* Furthest point sampling, all samples in one launch (one workgroup per sample).  Pick 0 is index 0; pick j is the arg max over
 * the sample of the running min of the squared distances (expression above) to picks 0..j-1, and of exactly equal
 * distances the LOWEST index wins.  A sample with n < npoint points returns its n picks cyclically (out[j] = out[j % n]), one
 * with n == 0 zeros.
 *   gd3d_vsa_fps        : xyz (B,n,3) -> out (B,npoint) int32
 *   gd3d_vsa_fps_stacked: xyz (N,3) + xyz_batch_cnt (B) -> out (B,npoint) int64, indices local to the sample
 * workspace: gd3d_vsa_fps_workspace_bytes(N total rows) bytes (the running minimum of the points beyond the
 * gd3d_vsa_fps_register_points() = 16384 per sample that live in registers); needs no initialisation. */
int gd3d_vsa_fps_register_points(void);
size_t gd3d_vsa_fps_workspace_bytes(int64_t N);
int gd3d_vsa_fps(const float* xyz, int32_t B, int32_t n, int32_t npoint, int32_t* out, void* workspace,
                 void* stream);
int gd3d_vsa_fps_stacked(const float* xyz, const int32_t* xyz_batch_cnt, int32_t B, int64_t N, int32_t npoint,
                         int64_t* out, void* workspace, void* stream);

/* `_cpu` twins (csrc/vsa_cpu.cpp): the same contracts on HOST memory, plain loops over the same fp32 operation sequence
 * compiled with the same -ffp-contract=off, so idx, cnt, the mask and the FPS picks are BIT-IDENTICAL to the kernels' and the
 * grouped outputs (copies and one subtraction) too.  The backward twins add in ascending (m, s) order.  nthreads <= 0:
 * std::thread::hardware_concurrency(). */
int gd3d_vsa_ball_query_cpu(const float* xyz, const int32_t* xyz_batch_cnt, const float* new_xyz,
                            const int32_t* new_xyz_batch_cnt, int32_t B, int64_t N, int64_t M, float radius,
                            int32_t nsample, int32_t* idx, int32_t* cnt, uint8_t* empty_mask, int32_t nthreads);
int gd3d_vsa_group_cpu(const float* features, const int32_t* features_batch_cnt, const int32_t* idx,
                       const int32_t* idx_batch_cnt, int32_t B, int64_t N, int64_t M, int32_t C, int32_t nsample,
                       float* out, int32_t nthreads);
int gd3d_vsa_group_backward_cpu(const float* grad_out, const int32_t* idx, const int32_t* idx_batch_cnt,
                                const int32_t* features_batch_cnt, int32_t B, int64_t N, int64_t M, int32_t C,
                                int32_t nsample, float* grad_features);
int gd3d_vsa_query_and_group_cpu(const float* xyz, const int32_t* xyz_batch_cnt, const float* new_xyz,
                                 const int32_t* new_xyz_batch_cnt, const float* features, int32_t B, int64_t N,
                                 int64_t M, int32_t C, float radius, int32_t nsample, int32_t use_xyz, float* out,
                                 int32_t* idx, int32_t* cnt, uint8_t* empty_mask, int32_t nthreads);
int gd3d_vsa_query_and_group_backward_cpu(const float* grad_out, const int32_t* idx, const int32_t* cnt,
                                          const int32_t* new_xyz_batch_cnt, const int32_t* xyz_batch_cnt, int32_t B,
                                          int64_t N, int64_t M, int32_t C, int32_t nsample, int32_t c_off,
                                          float* grad_features);
int gd3d_vsa_fps_cpu(const float* xyz, int32_t B, int32_t n, int32_t npoint, int32_t* out, int32_t nthreads);
int gd3d_vsa_fps_stacked_cpu(const float* xyz, const int32_t* xyz_batch_cnt, int32_t B, int64_t N, int32_t npoint,
                             int64_t* out, int32_t nthreads);

/* ------------------------------------------------------------------------------------
 * Voxel query and the fused voxel query-and-group (an addition inside ABI 6; csrc/voxel_query.hip): a query looks
 * only at the cells of a window around its own cell instead of at every point of its sample.  Restated from the reference's
 * ops/vsa/src/voxel_query_gpu.cu:10-89 (voxel_query_kernel_stack; wrapper voxel_query.cpp:28-44), which ships without a Python
 * caller; the published op of that name is what Voxel R-CNN and PV-RCNN++ pool their RoI grids with.
 *
 * xyz (N,3) fp32: one point per row of coors (N,4) [b, z, y, x] on a grid (B, Z, Y, X) (every side <= 2^24, N <= 2^31 - 1);
 * new_xyz (M,3) fp32 the queries; new_coords (M,4) int32 [b, z, y, x] a query's cell on the same grid (any int32 value).
 * max_range: 3 HOST values (rz, ry, rx), each in [0, 16] (GD3D_E_TOOLARGE above).  1 <= nsample <= 1024 (GD3D_E_TOOLARGE above).
 *
 * Query m: radius2 = radius * radius (fp32).  The window is walked with dz slowest and dx fastest, each ascending from -r to +r.  A
 * cell outside [0,Z) x [0,Y) x [0,X) is skipped.  The cell's row i is looked up; no row: the cell is skipped, and so is a looked-up
 * row outside [0, N) (a caller's table may hold anything).
 *   d2 = (nx-x)*(nx-x) + (ny-y)*(ny-y) + (nz-z)*(nz-z)   fp32, left to right, no fma contraction (the ball query's expression)
 * The row is a member iff d2 <= radius2 — INCLUSIVE, where the ball query is strict; a NaN distance is no member (the reference's
 * `dist2 > radius2` rejection lets NaN in).  The first nsample members in window order fill idx[m,:] with GLOBAL rows of xyz (the ball
 * query's idx is local to the sample), the slots past the member count repeat the first member, cnt[m] = min(members, nsample).  An
 * empty query gives idx[m,:] = 0 and empty_mask[m] = 1 (the reference writes -1 into slot 0 and leaves the rest untouched).  A query
 * whose b is outside [0, B) is empty.  idx (M,nsample) int32; cnt (M) int32 and empty_mask (M) bytes are nullable.
 *
 * Two look-up forms; exactly one is handed in (table != NULL selects the table, skey / srow must then be NULL):
 *   sorted keys : skey (N) int64 ascending with srow (N) int32, as gd3d_vsa_voxel_index writes them.  key = ((b*Z + z)*Y + y)*X + x;
 *                 a row of coors with any coordinate outside the grid (the -1 tail of the static forms) gets the key B*Z*Y*X, sorts
 *                 last and is never found.  The sort is stable: of several rows in one cell the LOWEST is the cell's row.
 *   dense table : table (B,Z,Y,X) int32, the row of each cell or -1, as gd3d_vsa_voxel_table writes it (fill with -1, then the
 *                 lowest row of every cell): the reference's form, for callers who hold one; indexed in 64 bits.
 * gd3d_vsa_voxel_index: coors int32 (coors_is_int64 == 0) or int64; workspace: gd3d_vsa_voxel_index_workspace_bytes(N) bytes, 256-byte
 * aligned, no initialisation.  No host read: every call here is stream-ordered and can be captured.
 *
 * gd3d_vsa_voxel_coords: new_coords[m] = [b, z, y, x] of new_xyz[m] (x, y, z).  b comes from new_xyz_batch_cnt (B) (counts clamped to
 * the rows left, as everywhere in the stacked ops); a row past the counts' sum gets b = -1.  Per axis, in fp32:
 *   c = floor((p - lo) / cell)   one subtraction, one correctly rounded division, one floor (gd3d_hard_voxelize's sequence)
 * cell_size, range_min: 3 HOST values each, (x, y, z); cell_size > 0.  An axis for which -2^30 <= c < 2^30 does not hold (NaN, +-inf,
 * 1e30) gives b = -1 and the coordinate 0.  Cells outside the grid are NOT clamped: their window may still reach in.
 *
 * gd3d_vsa_voxel_query_and_group: the query, then out (M, (use_xyz ? 3 : 0) + C, nsample) = [grouped xyz minus the query centre
 * (use_xyz), grouped features (N,C)], every channel of an empty query zero: gd3d_vsa_query_and_group's block.  Its backward wrt
 * features is gd3d_vsa_query_and_group_backward called with B = 1 and the counts {N} and {M}: global rows are then local rows.
 * ---------------------------------------------------------------------------------- */
size_t gd3d_vsa_voxel_index_workspace_bytes(int64_t N);
int gd3d_vsa_voxel_index(const void* coors, int32_t coors_is_int64, int64_t N, int32_t B, int32_t Z, int32_t Y, int32_t X,
                         void* workspace, int64_t* skey, int32_t* srow, void* stream);
int gd3d_vsa_voxel_table(const void* coors, int32_t coors_is_int64, int64_t N, int32_t B, int32_t Z, int32_t Y, int32_t X,
                         int32_t* table, void* stream);
int gd3d_vsa_voxel_coords(const float* new_xyz, const int32_t* new_xyz_batch_cnt, int32_t B, int64_t M, const float* cell_size,
                          const float* range_min, int32_t* new_coords, void* stream);
int gd3d_vsa_voxel_query(const float* xyz, const float* new_xyz, const int32_t* new_coords, const int64_t* skey,
                         const int32_t* srow, const int32_t* table, int32_t B, int32_t Z, int32_t Y, int32_t X, int64_t N,
                         int64_t M, const int32_t* max_range, float radius, int32_t nsample, int32_t* idx, int32_t* cnt,
                         uint8_t* empty_mask, void* stream);
int gd3d_vsa_voxel_query_and_group(const float* xyz, const float* new_xyz, const int32_t* new_coords, const int64_t* skey,
                                   const int32_t* srow, const int32_t* table, const float* features, int32_t B, int32_t Z,
                                   int32_t Y, int32_t X, int64_t N, int64_t M, int32_t C, const int32_t* max_range,
                                   float radius, int32_t nsample, int32_t use_xyz, float* out, int32_t* idx, int32_t* cnt,
                                   uint8_t* empty_mask, void* stream);

/* `_cpu` twins (csrc/voxel_query_cpu.cpp): the same contracts on HOST memory, plain loops over the window in the stated order with
 * the same fp32 sequences, so every output is BIT-IDENTICAL to the kernels'.  The index twin ignores `workspace`.  nthreads <= 0:
 * std::thread::hardware_concurrency(). */
int gd3d_vsa_voxel_index_cpu(const void* coors, int32_t coors_is_int64, int64_t N, int32_t B, int32_t Z, int32_t Y, int32_t X,
                             void* workspace, int64_t* skey, int32_t* srow);
int gd3d_vsa_voxel_table_cpu(const void* coors, int32_t coors_is_int64, int64_t N, int32_t B, int32_t Z, int32_t Y, int32_t X,
                             int32_t* table);
int gd3d_vsa_voxel_coords_cpu(const float* new_xyz, const int32_t* new_xyz_batch_cnt, int32_t B, int64_t M,
                              const float* cell_size, const float* range_min, int32_t* new_coords);
int gd3d_vsa_voxel_query_cpu(const float* xyz, const float* new_xyz, const int32_t* new_coords, const int64_t* skey,
                             const int32_t* srow, const int32_t* table, int32_t B, int32_t Z, int32_t Y, int32_t X, int64_t N,
                             int64_t M, const int32_t* max_range, float radius, int32_t nsample, int32_t* idx, int32_t* cnt,
                             uint8_t* empty_mask, int32_t nthreads);
int gd3d_vsa_voxel_query_and_group_cpu(const float* xyz, const float* new_xyz, const int32_t* new_coords, const int64_t* skey,
                                       const int32_t* srow, const int32_t* table, const float* features, int32_t B, int32_t Z,
                                       int32_t Y, int32_t X, int64_t N, int64_t M, int32_t C, const int32_t* max_range,
                                       float radius, int32_t nsample, int32_t use_xyz, float* out, int32_t* idx,
                                       int32_t* cnt, uint8_t* empty_mask, int32_t nthreads);

/* ------------------------------------------------------------------------------------
 * Point-in-rotated-box ops (an addition inside ABI 6): mmdet3d 1.0's roiaware_pool3d `points_in_boxes_part` and
 * `points_in_boxes_all` (third party, CUDA only), PointwiseMaskHead.get_targets
 * (models/roi_heads/mask_heads/pointwise_mask_head.py:62-92) for a whole batch in one launch, and the dense RoI grid points of
 * Batch3DRoIGridExtractor.get_dense_grid_points (models/roi_heads/roi_extractors/batch_roigrid_extractor.py:56-71).
 *
 * Data: points (N,3) fp32 = the points of B samples one after another with pts_batch_cnt (B) int32; boxes (B,T,7) fp32 dense,
 * a box [x, y, z, dx, dy, dz, rz] with (x, y, z) the BOTTOM centre; box_cnt (B) int32 nullable: rows t >= box_cnt[b] of sample
 * b are ignored, NULL tests all T.  The kernels find the samples' start offsets from the count array themselves (no host
 * prefix sum, no host read).  Nothing validates counts on the host: every point count is clamped to [0, rows left in the
 * array] and every box count to [0, T].  Point rows beyond the counts' sum belong to no sample: they are in no box.
 *
 * Membership (mmdet3d's check_pt_in_box3d), every step ONE fp32 operation in this order, no fma contraction:
 *   hz = dz * 0.5f;  czm = z + hz;   |pz - czm| <= hz            (z faces INCLUSIVE)
 *   (s, c) = fixed-sequence sincos of -rz (the polynomial of the rotated NMS, no libm)
 *   sx = px - x;  sy = py - y;   lx = sx * c + sy * (-s);   ly = sx * s + sy * c
 *   lx > -hx && lx < hx && ly > -hy && ly < hy                   (hx = dx * 0.5f, hy = dy * 0.5f; x / y faces STRICT)
 * As the comparisons are written: zero or negative dx or dy, or negative dz, contain nothing (so do zero-padded rows); a
 * point with a NaN coordinate is in no box; boxes as tall as z = -1e8, dz = 2e8 work.
 *
 * gd3d_pib_part : box_idx (N) int32 = the LOWEST box index of the point's sample that contains it, -1 if none.
 * gd3d_pib_all  : flags (N,T) row-major, elem_size 1 (bytes 0 / 1) or 4 (int32 0 / 1); columns t >= box_cnt[b] are written
 *                 0: the call leaves no element unwritten.
 * gd3d_pib_mask_targets : per point i = first of the gt_boxes that contains it, e = first of the ENLARGED boxes
 *                 (z - extra_width, dx + 2 extra_width, dy + .., dz + .., each one fp32 operation) that does;
 *                 seg_targets (N) int64 = i >= 0 ? gt_labels[b, i] : num_classes, and -1 where (i >= 0) != (e >= 0) (the
 *                 reference's xor: a negative extra_width behaves as there).  gt_labels (B,T) int64.  box_idx (N) int32
 *                 nullable receives i.
 * gd3d_roi_grid_points : rois = R rows of roi_stride floats, the box at column first_col (as coder_roi_decode takes them);
 *                 out (R, G^3, 3) fp32, 1 <= G <= 16; point (i, j, k), k fastest:
 *                   u = (i + 0.5f) / G - 0.5f, v = (j + 0.5f) / G - 0.5f, w = (k + 0.5f) / G;  l = (u dx, v dy, w dz);
 *                   x' = lx c - ly s, y' = lx s + ly c  (sincos of rz; clockwise != 0: x' = lx c + ly s, y' = ly c - lx s,
 *                   the same sense and flag as coder_roi_decode);  out = (x' + x, y' + y, lz + z).
 * gd3d_pib_box_tile / gd3d_pib_workgroup_points : boxes per LDS tile and points per workgroup of the kernels (the sizes at
 *                 which they change path; for tests).
 * All stream-ordered, caller-allocated outputs.  `_cpu` twins (csrc/pib_cpu.cpp): the same contracts on HOST memory over the
 * same operation sequence, BIT-IDENTICAL results.  nthreads <= 0: std::thread::hardware_concurrency().
 * ---------------------------------------------------------------------------------- */
int gd3d_pib_box_tile(void);
int gd3d_pib_workgroup_points(void);
int gd3d_pib_part(const float* points, const int32_t* pts_batch_cnt, const float* boxes, const int32_t* box_cnt,
                  int32_t B, int64_t N, int32_t T, int32_t* box_idx, void* stream);
int gd3d_pib_all(const float* points, const int32_t* pts_batch_cnt, const float* boxes, const int32_t* box_cnt,
                 int32_t B, int64_t N, int32_t T, void* flags, int32_t elem_size, void* stream);
int gd3d_pib_mask_targets(const float* points, const int32_t* pts_batch_cnt, const float* gt_boxes,
                          const int64_t* gt_labels, const int32_t* box_cnt, int32_t B, int64_t N, int32_t T,
                          float extra_width, int32_t num_classes, int64_t* seg_targets, int32_t* box_idx,
                          void* stream);
int gd3d_roi_grid_points(const float* rois, int32_t roi_stride, int32_t first_col, int64_t R, int32_t G,
                         int32_t clockwise, float* out, void* stream);
int gd3d_pib_part_cpu(const float* points, const int32_t* pts_batch_cnt, const float* boxes, const int32_t* box_cnt,
                      int32_t B, int64_t N, int32_t T, int32_t* box_idx, int32_t nthreads);
int gd3d_pib_all_cpu(const float* points, const int32_t* pts_batch_cnt, const float* boxes, const int32_t* box_cnt,
                     int32_t B, int64_t N, int32_t T, void* flags, int32_t elem_size, int32_t nthreads);
int gd3d_pib_mask_targets_cpu(const float* points, const int32_t* pts_batch_cnt, const float* gt_boxes,
                              const int64_t* gt_labels, const int32_t* box_cnt, int32_t B, int64_t N, int32_t T,
                              float extra_width, int32_t num_classes, int64_t* seg_targets, int32_t* box_idx,
                              int32_t nthreads);
int gd3d_roi_grid_points_cpu(const float* rois, int32_t roi_stride, int32_t first_col, int64_t R, int32_t G,
                             int32_t clockwise, float* out, int32_t nthreads);

/* ------------------------------------------------------------------------------------
 * The RoI head's training slice (an addition inside ABI 6): PVRCNNBboxHead.get_targets / _get_target_single
 * (models/roi_heads/bbox_heads/pvrcnn_bbox_head.py:213-316, concat=True) as one launch, and loss with get_corner_loss_lidar
 * (:140-211, :318-351) — the three losses and their gradients — as one launch.  One workgroup each, no workspace, no atomics on
 * floats, no read-back: the same inputs give the same bits on every run.
 *
 * gd3d_roi_head_targets : pos_bboxes / pos_gt_bboxes (P,7) fp32 = the positives' RoIs and gt boxes of B samples one after
 *   another with pos_batch_cnt (B) int32; ious (R) fp32 = the sampled RoIs' IoUs with roi_batch_cnt (B) int32.  Every count
 *   is clamped to [0, rows left]; nothing is validated on the host.  B <= 1024, P, R <= 2^24 (GD3D_E_TOOLARGE).
 *     label (R) fp32         = iou > pos ? 1 : (iou < neg ? 0 : iou * 2 - 0.5)
 *     reg_mask (R) int64     = 1 for the first pos_batch_cnt[b] rows of sample b
 *     label_weights (R) fp32 = (label >= 0) / max(their number, 1);  bbox_weights (R) fp32 = reg_mask / max(its sum, 1)
 *     RoI rows past the counts' sum belong to no sample: label 0, mask 0, both weights 0.
 *     bbox_targets (P,7) fp32: with mod(a) = fmodf(a, 2 pi), + 2 pi when negative (the constants are the fp32 roundings of the
 *       doubles 2 pi, pi, pi / 2, 3 pi / 2):  ry = mod(roi[6]);  d = gt[0:3] - roi[0:3] turned about z by -ry
 *       (x' = dx cos ry + dy sin ry, y' = -dx sin ry + dy cos ry; clockwise != 0 flips the angle's sign);  r = mod(gt[6] - ry);
 *       pi / 2 < r < 3 pi / 2: r = mod(r + pi);  r > pi: r -= 2 pi;  r clamped to [-pi / 2, pi / 2];  then
 *       DeltaXYZWLHRBBoxCoder.encode of (x', y', d_z, gt dims, r) against the anchor (0, 0, 0, roi dims, 0).  Rows past the
 *       positive counts' sum are written 0.
 *     PRECONDITION, not checked (it would take a host read): pos_batch_cnt[b] <= roi_batch_cnt[b] for every sample.  A sample
 *       with more positives than RoIs gets more target rows than reg_mask has ones, and gd3d_roi_head_loss, which pairs the j-th
 *       mask positive with target row j, then pairs every later positive with the wrong target.
 * gd3d_roi_head_loss : cls_score (R), bbox_pred (R,7), rois = R rows of roi_stride floats with the box at column first_col (as
 *   coder_roi_decode takes them), labels / label_weights / bbox_weights (R) fp32, reg_mask (R) int64, bbox_targets /
 *   pos_gt_bboxes (P,7).  The j-th row with reg_mask > 0, in row order, pairs with row j of the two (P,7) arrays; positive rows
 *   past the P-th are ignored.  losses (3) fp32:
 *     [0] cls_weight  * sum_i label_weights[i] (max(x, 0) - x z + log1p(exp(-|x|)))         (sigmoid cross entropy, 'sum')
 *     [1] bbox_weight * sum over the paired rows and 7 columns of bbox_weights[row] * smooth_l1(pred - target; beta), beta > 0
 *     [2] with_corner_loss != 0: the mean over the paired rows of the mean over the 8 corners of Huber(min(|p - g|, |p - g'|), 1):
 *         p the corners of the box decoded from (roi, pred) by coder_roi_decode's math, g those of the gt, g' of the gt turned
 *         by pi; corners = centre + Rz(yaw) (dims * n), n_x, n_y = -+0.5, n_z = 0, 1.  Otherwise 0.
 *   grad_cls (R), grad_bbox (R,7) = d([1] + [2]) / d bbox_pred, grad_bbox_l1 = d[1] / d bbox_pred, grad_bbox_corner = d[2] / d
 *   bbox_pred; each nullable, each written in full (zeros for the rows without a pair).  A zero corner distance has a zero
 *   gradient; on an exact tie of the two distances the unflipped gt takes the whole gradient.  No pair at all: [1] = [2] = 0.
 *   clockwise != 0 flips the sense of the decode's and the corners' rotations, as in gd3d_roi_head_targets.
 * `_cpu` twins (csrc/roi_head_cpu.cpp): the same contracts on HOST memory on the calling thread; label, reg_mask and both
 * weight arrays BIT-IDENTICAL to the kernels', the other values equal up to the two math libraries' sin / cos / exp / log.
 * ---------------------------------------------------------------------------------- */
int gd3d_roi_head_targets(const float* pos_bboxes, const float* pos_gt_bboxes, const float* ious,
                          const int32_t* pos_batch_cnt, const int32_t* roi_batch_cnt, int32_t B, int64_t P, int64_t R,
                          float cls_pos_thr, float cls_neg_thr, int32_t clockwise, float* label, float* bbox_targets,
                          int64_t* reg_mask, float* label_weights, float* bbox_weights, void* stream);
int gd3d_roi_head_loss(const float* cls_score, const float* bbox_pred, const float* rois, int32_t roi_stride,
                       int32_t first_col, const float* labels, const float* bbox_targets, const float* pos_gt_bboxes,
                       const int64_t* reg_mask, const float* label_weights, const float* bbox_weights, int64_t R, int64_t P,
                       float beta, float cls_weight, float bbox_weight, int32_t with_corner_loss, int32_t clockwise,
                       float* losses, float* grad_cls, float* grad_bbox, float* grad_bbox_l1, float* grad_bbox_corner,
                       void* stream);
int gd3d_roi_head_targets_cpu(const float* pos_bboxes, const float* pos_gt_bboxes, const float* ious,
                              const int32_t* pos_batch_cnt, const int32_t* roi_batch_cnt, int32_t B, int64_t P, int64_t R,
                              float cls_pos_thr, float cls_neg_thr, int32_t clockwise, float* label, float* bbox_targets,
                              int64_t* reg_mask, float* label_weights, float* bbox_weights);
int gd3d_roi_head_loss_cpu(const float* cls_score, const float* bbox_pred, const float* rois, int32_t roi_stride,
                           int32_t first_col, const float* labels, const float* bbox_targets, const float* pos_gt_bboxes,
                           const int64_t* reg_mask, const float* label_weights, const float* bbox_weights, int64_t R,
                           int64_t P, float beta, float cls_weight, float bbox_weight, int32_t with_corner_loss,
                           int32_t clockwise, float* losses, float* grad_cls, float* grad_bbox, float* grad_bbox_l1,
                           float* grad_bbox_corner);

/* ------------------------------------------------------------------------------------
 * The RoI head's assign-and-sample stage (an addition inside ABI 6): PVRCNNROIHead._assign_and_sample
 * (models/roi_heads/pvrcnn_roi_head.py:225-297) — a MaxIoUAssigner per class on BboxOverlaps3D(coordinate='lidar') and the
 * IoUNegPiecewiseSampler — for a whole batch: one launch of one workgroup per sample and one single-workgroup launch that packs
 * the samples back to back.  No read-back, no allocation; given the keys the outputs are the same bits on every run and in the
 * `_cpu` twins (csrc/roi_sample_cpu.cpp, host memory, calling thread).  mmdet's assigner and sampler are third party, absent from
 * the reference and not pinned by it: the rules below are what is computed.
 *
 * gd3d_roi_iou3d : iou (n1, n2) fp32 of rows [x, y, z, dx, dy, dz, yaw], z the BOTTOM face.  Per pair, in fp32, one operation at
 *   a time (-ffp-contract=off, the NMS path's fixed sin / cos / atan2 sequences):
 *     ov_bev = the iou3d-family overlap (rnms_*'s pair test) of the rectangles [x - dx/2, y - dy/2, x + dx/2, y + dy/2, yaw]
 *     ov_h   = max(min(z1 + dz1, z2 + dz2) - max(z1, z2), 0);   ov = ov_bev * ov_h
 *     iou    = ov / max(dx1 dy1 dz1 + dx2 dy2 dz2 - ov, 1e-8)
 *   n1 * n2 < 2^31 (GD3D_E_TOOLARGE); an empty operand writes nothing.
 *
 * gd3d_roi_assign_sample : proposals (N,7) fp32 / proposal_labels (N) int64 / keys (N) fp32 of B samples one after another with
 *   prop_batch_cnt (B) int32; gt_bboxes (G,7) / gt_labels (G) int64 with gt_batch_cnt (B); fill_keys (B * num) fp32.  Counts are
 *   DEVICE memory, clamped to [0, rows left]; of a sample's segment the first 4096 proposals and 1024 gts take part.
 *   HOST arrays: pos_iou_thr / neg_iou_thr / min_pos_iou (C) fp32 and assign_flags (C) (bit 0 match_low_quality, bit 1
 *   gt_max_assign_all), one assigner per class; neg_piece_fractions (K) fp64 in [0, 1] and neg_iou_piece_thrs (K) fp32, positive
 *   and strictly descending.  C <= 16, num <= 1024, 0 <= npos <= num, K <= 8, B <= 1024.
 *   Assignment, per sample: a proposal with label c in [0, C) meets the gts with label c, under assigner c; any other label meets
 *   nothing.  An IoU that is NaN or negative counts as 0.  max_overlap[n] = the largest IoU over its class's gts (lowest gt on a
 *   tie); without one max_overlap = 0 and gt_ind = 0.  Otherwise, in this order: gt_ind = -1;  0 where 0 <= max < neg_iou_thr;
 *   argmax + 1 where max >= pos_iou_thr;  with match_low_quality, for each gt g of the class in ascending index with gt_max[g] >=
 *   min_pos_iou: every proposal of the class with iou[n, g] == gt_max[g] (gt_max_assign_all), or only the lowest-index one, gets
 *   g + 1, a later gt overwriting.  gt_ind numbers the sample's full gt list.
 *   Sampling, per sample; "draw k of S" = all of S when |S| <= k, else the k members with the smallest (key, proposal index); a
 *   key outside [0, 1) or NaN is clamped into it.  Positives {gt_ind > 0}: a draw of npos, output in ascending proposal index.
 *   Negatives {gt_ind == 0}, expected = num - positives drawn: piece i = {lo <= max_overlap < thr[i]}, lo = thr[i + 1], 0 for the
 *   last piece; piece i < K - 1 expects (int)(expected * fraction[i]) + carry, the last one expected - chosen so far; a piece with
 *   fewer members gives them all and ADDS its shortfall to the carry, another gives a draw and zeroes the carry; no piece gives
 *   more than what is left of expected; members leave a piece in (key, index) order.  A short last piece is followed by slots
 *   filled with replacement up to expected: the slot at position j of the sample's output takes member min(floor(fill_keys[b *
 *   num + j] * m), m - 1) of the last piece in ascending index order, or, that piece being empty, of the negatives chosen so far
 *   in output order; nothing chosen, nothing filled.
 *   Outputs, samples packed back to back (positives, then negatives), rows past the counts' sums written as batch id -1 / zeros:
 *   rois (B * num, 8) [batch id, box], ious (B * num) = max_overlap, inds (B * num) int64 = proposal index within its sample,
 *   pos_bboxes / pos_gt_bboxes (B * npos, 7), pos_assigned_gt_inds (B * npos) int64 = gt_ind - 1, pos_batch_cnt / roi_batch_cnt
 *   (B) int32; gt_inds / max_overlaps / labels (N) (labels = the assigned gt's label, -1 where gt_ind <= 0; rows of no sample or
 *   past a sample's limit: -1 / 0 / -1).  stage: B * (2 + num) int32 of scratch (per sample: positives drawn, rows, the chosen
 *   indices), written in full.
 * ---------------------------------------------------------------------------------- */
int gd3d_roi_iou3d(const float* bboxes1, int64_t n1, const float* bboxes2, int64_t n2, float* iou, void* stream);
int gd3d_roi_assign_sample(const float* proposals, const int64_t* proposal_labels, const int32_t* prop_batch_cnt, int64_t N,
                           const float* gt_bboxes, const int64_t* gt_labels, const int32_t* gt_batch_cnt, int64_t G, int32_t B,
                           const float* keys, const float* fill_keys, int32_t C, const float* pos_iou_thr,
                           const float* neg_iou_thr, const float* min_pos_iou, const int32_t* assign_flags, int32_t num,
                           int32_t npos, int32_t K, const double* neg_piece_fractions, const float* neg_iou_piece_thrs,
                           float* rois, float* ious, int64_t* inds, float* pos_bboxes, float* pos_gt_bboxes,
                           int64_t* pos_assigned_gt_inds, int32_t* pos_batch_cnt, int32_t* roi_batch_cnt, int64_t* gt_inds,
                           float* max_overlaps, int64_t* labels, int32_t* stage, void* stream);
int gd3d_roi_iou3d_cpu(const float* bboxes1, int64_t n1, const float* bboxes2, int64_t n2, float* iou);
int gd3d_roi_assign_sample_cpu(const float* proposals, const int64_t* proposal_labels, const int32_t* prop_batch_cnt, int64_t N,
                               const float* gt_bboxes, const int64_t* gt_labels, const int32_t* gt_batch_cnt, int64_t G,
                               int32_t B, const float* keys, const float* fill_keys, int32_t C, const float* pos_iou_thr,
                               const float* neg_iou_thr, const float* min_pos_iou, const int32_t* assign_flags, int32_t num,
                               int32_t npos, int32_t K, const double* neg_piece_fractions, const float* neg_iou_piece_thrs,
                               float* rois, float* ious, int64_t* inds, float* pos_bboxes, float* pos_gt_bboxes,
                               int64_t* pos_assigned_gt_inds, int32_t* pos_batch_cnt, int32_t* roi_batch_cnt,
                               int64_t* gt_inds, float* max_overlaps, int64_t* labels, int32_t* stage);

/* ------------------------------------------------------------------------------------
 * The keypoint segmentation slice (an addition inside ABI 6): PointwiseMaskHead.loss
 * (models/roi_heads/mask_heads/pointwise_mask_head.py:124-144) — the loss and its gradient — as one launch of one workgroup, and
 * the keypoint reweighting of PVRCNNROIHead._bbox_forward (models/roi_heads/pvrcnn_roi_head.py:211-212), forward and backward, as
 * one streaming launch each.  No workspace, no atomics on floats, no read-back: the same inputs give the same bits on every run.
 * mmdet's FocalLoss is third party, absent and not pinned by the reference: the math below (mmdet 2.x's published
 * py_sigmoid_focal_loss, reduction 'sum') is what is computed.
 *
 * gd3d_seg_head_loss : seg_preds (N,K) fp32, seg_targets (N) int64 = gd3d_pib_mask_targets' output (-1 ignore, 0..num_classes-1 a
 *   class, num_classes background).  K must be 1 with class_agnostic != 0, else num_classes; 1 <= K <= 255; gamma >= 0;
 *   0 <= alpha <= 1 (GD3D_E_BADARG); N <= 2^24 (GD3D_E_TOOLARGE; correct, but one workgroup: not meant to be fast beyond ~10^5).
 *   Per row i with c = seg_targets[i]:  pos = [0 <= c < num_classes], neg = [c == num_classes], n_pos = sum pos,
 *   w = (pos + neg) / max(n_pos, 1); a target above num_classes is neither: weight 0 (the reference's one_hot would raise).
 *   The label l is pos (class agnostic) or c with ignored rows at num_classes; per column k, t = [l == k], p = sigmoid(x):
 *     t = 1:  loss = -alpha (1-p)^gamma log p,       d/dx = alpha (1-p)^gamma (gamma p log p - (1-p))
 *     t = 0:  loss = -(1-alpha) p^gamma log(1-p),    d/dx = (1-alpha) p^gamma (p - gamma (1-p) log(1-p))
 *   with log p = -softplus(-x), log(1-p) = -softplus(x), softplus(x) = max(x, 0) + log1p(exp(-|x|)): finite at |x| = 100.
 *   Class agnostic, the positives carry label 1 and K = 1, so t = [l == 0]: the one column is trained towards 1 on the
 *   NON-positive rows — what the reference computes, restated, not repaired.
 *   out (2) fp32: [0] loss_weight * sum_i w_i sum_k loss (fp64 sum), [1] n_pos.  grad (N,K), nullable: loss_weight * w_i * d/dx,
 *   every element written (zeros on the rows of weight 0).  N == 0 writes out = (0, 0).
 * gd3d_keypoint_reweight : out (N,C) = feats (N,C) * s_i, s_i = max_k sigmoid(seg_preds[i,k]) with sigmoid(x) = 1 / (1 + exp(-x))
 *   in fp32; win (N) uint8, nullable: the winning column, the LOWEST on equal fp32 sigmoid values (as CPU torch's max(dim) routes
 *   its gradient).  1 <= K <= 255, C >= 1 (GD3D_E_BADARG); N == 0 launches nothing.
 * gd3d_keypoint_reweight_backward : grad_feats (N,C) = grad_out * s_i;  grad_seg (N,K): column win[i] =
 *   (sum_c grad_out[i,c] feats[i,c]) * s_i (1 - s_i), the others 0; each nullable, each written in full.  win is the forward's.
 *   The row sum is fp32 in a fixed order: a group of G lanes (the power of two covering ceil(C / 4), 64 at most) shares a row,
 *   lane l adds the columns of quads l, l + G, .. in order, and the lanes fold pairwise, l with l + G/2, then G/4, .. 1.
 *   Both reweight entry points use 16-byte accesses when C % 4 == 0 and the (N,C) base pointers are 16-byte aligned, 4-byte ones
 *   otherwise; the results are the same bits either way.
 * `_cpu` twins (csrc/seg_head_cpu.cpp): the same contracts on HOST memory on the calling thread; n_pos and win BIT-IDENTICAL to
 * the kernels', the other values equal up to the two math libraries' exp / log1p / pow.
 * ---------------------------------------------------------------------------------- */
int gd3d_seg_head_loss(const float* seg_preds, const int64_t* seg_targets, int64_t N, int32_t K, int32_t num_classes,
                       int32_t class_agnostic, float gamma, float alpha, float loss_weight, float* out, float* grad,
                       void* stream);
int gd3d_keypoint_reweight(const float* feats, const float* seg_preds, int64_t N, int64_t C, int32_t K, float* out,
                           uint8_t* win, void* stream);
int gd3d_keypoint_reweight_backward(const float* grad_out, const float* feats, const float* seg_preds, const uint8_t* win,
                                    int64_t N, int64_t C, int32_t K, float* grad_feats, float* grad_seg, void* stream);
int gd3d_seg_head_loss_cpu(const float* seg_preds, const int64_t* seg_targets, int64_t N, int32_t K, int32_t num_classes,
                           int32_t class_agnostic, float gamma, float alpha, float loss_weight, float* out, float* grad);
int gd3d_keypoint_reweight_cpu(const float* feats, const float* seg_preds, int64_t N, int64_t C, int32_t K, float* out,
                               uint8_t* win);
int gd3d_keypoint_reweight_backward_cpu(const float* grad_out, const float* feats, const float* seg_preds, const uint8_t* win,
                                        int64_t N, int64_t C, int32_t K, float* grad_feats, float* grad_seg);

/* ------------------------------------------------------------------------------------
 * The keypoint BEV interpolation and the voxel-centre sources (an addition inside ABI 6): the statements of
 * VoxelSetAbstraction.forward outside its MLPs that had no entry here — interpolate_from_bev_features
 * (models/middle_encoders/voxel_set_abstraction.py:153-177), get_voxel_centers (:179-193) and the per-sample count loop
 * (:303-305).  No workspace, no read-back.
 *
 * gd3d_vsa_bev_interp : out (B,M,C) fp32 contiguous = the bilinear sample of bev (B,C,H,W) fp32 at the keypoints' xy —
 *   F.grid_sample(align_corners=True, padding_mode='zeros') on the reference's normalised grid, squeezed and permuted.
 *   keypoints: element [b, m, d] at keypoints[b * kp_stride_b + m * kp_stride_m + d], d = 0 (x), 1 (y); nothing else is read.
 *   layout 0: bev is contiguous NCHW; layout 1: channels last (element [b,c,y,x] at ((b*H + y)*W + x)*C + c).  The map is read
 *   where it lies.  (tl_x, tl_y) / (br_x, br_y): the world xy of the centres of cell (0,0) / (H-1,W-1), computed by the caller.
 *   H, W >= 2, br > tl on both axes, C >= 1, strides >= 0 (GD3D_E_BADARG); H, W <= 2^24 (GD3D_E_TOOLARGE).  B == 0 or M == 0
 *   launches nothing.  Per keypoint, in fp32, one operation per step, no contraction, correctly rounded division:
 *     ix = ((x - tl_x) * (float)(W - 1)) / (br_x - tl_x),  iy = ((y - tl_y) * (float)(H - 1)) / (br_y - tl_y)
 *     reach = ix > -1 && ix < (float)W && iy > -1 && iy < (float)H      (false for NaN and +-inf: compared BEFORE any conversion)
 *     x0 = floor(ix), y0 = floor(iy) (converted to integers only when reach);  ax = ix - x0, ay = iy - y0, bx = 1 - ax, by = 1 - ay
 *     weights nw = bx*by, ne = ax*by, sw = bx*ay, se = ax*ay for the cells (y0,x0), (y0,x0+1), (y0+1,x0), (y0+1,x0+1)
 *     out[c] = ((v_nw*nw + v_ne*ne) + v_sw*sw) + v_se*se, the value of a cell outside the map being 0.
 *   Without reach (a cell or more outside, or a non-finite coordinate) the row is 0 — the reference's result for a non-finite
 *   coordinate is unspecified: restated, not matched.  No index leaves the map for any input; offsets are 64-bit.  Channels last
 *   with C % 4 == 0 and 16-byte aligned bev / out takes 16-byte accesses, everything else 4-byte ones: the same bits, and the same
 *   bits for both layouts.
 * gd3d_vsa_bev_interp_backward : grad_bev (B,C,H,W) in `layout` = sum over the keypoints of grad_out (B,M,C)[b,m,c] * weight into
 *   the (at most four) cells in the map; EVERY element of grad_bev is written (a fill kernel zeroes it first).  fp32 atomic adds,
 *   lanes along C: where several keypoints share a cell the last bits depend on the order of arrival.  No gradient for the
 *   keypoints (grid_sample would return one for its grid).  Same argument checks; B == 0 launches nothing, M == 0 only the fill.
 * gd3d_vsa_voxel_centers : coors (N,4) int32 (coors_is_int64 == 0) or int64, columns [b, z, y, x].  xyz (N,3) fp32:
 *     xyz[i][a] = (((float)coors[i][3 - a] * voxel_size[a]) * scale + range_min[a]) + add[a],   a = 0 (x), 1 (y), 2 (z)
 *   four fp32 operations left to right (the reference's `c * vs * scale + min` and its in-place add of (0.5*vs)*scale for 'half',
 *   0.5*vs for 'halfmin', which the caller passes as `add`); voxel_size, range_min and add are three floats each in HOST memory,
 *   read during the call.  xyz_batch_cnt (batch_size) int32: the rows whose b equals the index; zeroed by the entry point, then
 *   integer adds reduced per wave: exact in any order.  A row with b outside [0, batch_size) is counted nowhere; its centre is
 *   still written.  N == 0 writes the zero counts only.
 * `_cpu` twins (csrc/vsa_bev_cpu.cpp): the same contracts on HOST memory on the calling thread.  The forward, xyz and the counts
 * are BIT-IDENTICAL to the kernels'; the twin's backward is sequential (keypoints in order, neighbours nw, ne, sw, se).
 * ---------------------------------------------------------------------------------- */
int gd3d_vsa_bev_interp(const float* keypoints, int64_t kp_stride_b, int64_t kp_stride_m, const float* bev, int32_t layout,
                        int64_t B, int64_t M, int64_t C, int64_t H, int64_t W, float tl_x, float tl_y, float br_x, float br_y,
                        float* out, void* stream);
int gd3d_vsa_bev_interp_backward(const float* grad_out, const float* keypoints, int64_t kp_stride_b, int64_t kp_stride_m,
                                 int32_t layout, int64_t B, int64_t M, int64_t C, int64_t H, int64_t W, float tl_x, float tl_y,
                                 float br_x, float br_y, float* grad_bev, void* stream);
int gd3d_vsa_voxel_centers(const void* coors, int32_t coors_is_int64, int64_t N, const float* voxel_size, float scale,
                           const float* range_min, const float* add, int32_t batch_size, float* xyz, int32_t* xyz_batch_cnt,
                           void* stream);
int gd3d_vsa_bev_interp_cpu(const float* keypoints, int64_t kp_stride_b, int64_t kp_stride_m, const float* bev, int32_t layout,
                            int64_t B, int64_t M, int64_t C, int64_t H, int64_t W, float tl_x, float tl_y, float br_x,
                            float br_y, float* out);
int gd3d_vsa_bev_interp_backward_cpu(const float* grad_out, const float* keypoints, int64_t kp_stride_b, int64_t kp_stride_m,
                                     int32_t layout, int64_t B, int64_t M, int64_t C, int64_t H, int64_t W, float tl_x,
                                     float tl_y, float br_x, float br_y, float* grad_bev);
int gd3d_vsa_voxel_centers_cpu(const void* coors, int32_t coors_is_int64, int64_t N, const float* voxel_size, float scale,
                               const float* range_min, const float* add, int32_t batch_size, float* xyz,
                               int32_t* xyz_batch_cnt);

/* ------------------------------------------------------------------------------------
 * Hard voxelization, dynamic voxelization and the mean voxel encoder (an addition inside ABI 6): PVRCNN.voxelize and the
 * HardSimpleVFE call of extract_feat (models/detectors/pv_rcnn.py:43-49, 66-86) — mmdet3d's `Voxelization` op per sample, a cat, an
 * F.pad per sample and a host read of coors[-1, 0] — for the whole stacked batch in one stream-ordered call that reads nothing back.
 * mmdet3d is not pinned by the reference; its published `hard_voxelize` is restated here, in the DETERMINISTIC order of its CPU op
 * and of its deterministic=True GPU path (deterministic=False only means that its fast path returns some arbitrary order).
 *
 * Operands: points (N, >= C) fp32, row i at points + i * row_stride, columns 0, 1, 2 = x, y, z; points_batch_cnt (B) int32: the
 * stack's rows per sample, in order (negative counts count as 0; rows past the last sample belong to no sample and are dropped).
 * voxel_size, range_min (3 floats, x y z) and grid_size (3 int32, x y z) lie in HOST memory and are read during the call; the caller
 * computes grid_size = round((range_max - range_min) / voxel_size) in fp32 as mmdet3d's module does.
 * The cell of a point on axis j, in fp32, one operation per step, no contraction, correctly rounded division:
 *     f_j = floor((p_j - range_min_j) / voxel_size_j);   kept iff f_j >= 0 && f_j < (float)grid_j on all three axes,
 * compared as FLOATS before any conversion: NaN, +-inf and 1e30 are dropped and no conversion overflows.
 * gd3d_hard_voxelize : walk the kept points of each sample in index order: a cell not seen before becomes the sample's next voxel
 *   if fewer than max_voxels are numbered, else the point is skipped (a `continue`: later points of numbered voxels still join them);
 *   a point joins slot num_points[v] of its voxel if that is < max_num_points, else it is skipped.  Outputs, each of
 *   R = min(N, B * max_voxels) rows, the samples' voxels one after the other as torch.cat lays them:
 *     voxels (R, max_num_points, C) fp32, nullable: columns 0 .. C-1 of the point in each slot, unused slots 0;
 *     coors (R, 4) int32: (b, z, y, x);   num_points (R) int32;
 *     mean (R, num_features) fp32, nullable: HardSimpleVFE — per column, slots 0, 1, 2, .. of the voxel added IN SEQUENCE to +0 in
 *       fp32, then ONE division by num_points (the unused slots are zeros and are not added: the same bits);
 *     voxel_batch_cnt (B) int32: voxels per sample;   num (2) int64: [0] the total V, [1] the dropped points (outside the grid, non-
 *       finite or of no sample; points skipped by the two limits are not counted).
 *   Rows at and past V: coors -1, num_points 0, voxels and mean 0.  workspace: gd3d_hard_voxelize_workspace_bytes(N, B, max_voxels)
 *   bytes, 256-byte aligned.  C == 4 with row_stride % 4 == 0 and 16-byte aligned points / voxels / mean takes 16-byte row accesses,
 *   everything else 4-byte ones: the same bits.  max_num_points < 1, max_voxels < 1, C < 3, row_stride < C, num_features outside
 *   [1, C] with a mean: GD3D_E_BADARG; N > 2^31 - 1, a grid axis > 2^24, B * cells >= 2^62, B > 1024, C > 256: GD3D_E_TOOLARGE.
 *   N == 0 or B == 0 writes the zero counts only.
 * gd3d_dynamic_voxelize : coors (N, 4) int32 = (b, z, y, x) of every point, all -1 for a dropped one, in one launch: the `coors`
 *   operand of vox_index_build.
 * gd3d_voxel_mean : the encoder alone on caller-held voxels (V, P, C) and num_points (V) -> mean (V, num_features): the first
 *   min(max(num_points, 0), P) slots added in sequence as above (slots past num_points are not read); num_points == 0 gives 0.
 * `_cpu` twins (csrc/hard_voxel_cpu.cpp): the same contracts on HOST memory on the calling thread, the hard one as the sequential
 *   walk above over a hash map; `workspace` is ignored.  Every output is BIT-IDENTICAL to the kernels'.
 * ---------------------------------------------------------------------------------- */
size_t gd3d_hard_voxelize_workspace_bytes(int64_t N, int32_t B, int32_t max_voxels);
int gd3d_hard_voxelize(const float* points, int64_t N, int64_t row_stride, int32_t C, const int32_t* points_batch_cnt, int32_t B,
                       const float* voxel_size, const float* range_min, const int32_t* grid_size, int32_t max_num_points,
                       int32_t max_voxels, int32_t num_features, void* workspace, float* voxels, float* mean, int32_t* coors,
                       int32_t* num_points, int32_t* voxel_batch_cnt, int64_t* num, void* stream);
int gd3d_dynamic_voxelize(const float* points, int64_t N, int64_t row_stride, const int32_t* points_batch_cnt, int32_t B,
                          const float* voxel_size, const float* range_min, const int32_t* grid_size, int32_t* coors, void* stream);
int gd3d_voxel_mean(const float* voxels, const int32_t* num_points, int64_t V, int32_t P, int32_t C, int32_t num_features,
                    float* mean, void* stream);
int gd3d_hard_voxelize_cpu(const float* points, int64_t N, int64_t row_stride, int32_t C, const int32_t* points_batch_cnt, int32_t B,
                           const float* voxel_size, const float* range_min, const int32_t* grid_size, int32_t max_num_points,
                           int32_t max_voxels, int32_t num_features, void* workspace, float* voxels, float* mean, int32_t* coors,
                           int32_t* num_points, int32_t* voxel_batch_cnt, int64_t* num);
int gd3d_dynamic_voxelize_cpu(const float* points, int64_t N, int64_t row_stride, const int32_t* points_batch_cnt, int32_t B,
                              const float* voxel_size, const float* range_min, const int32_t* grid_size, int32_t* coors);
int gd3d_voxel_mean_cpu(const float* voxels, const int32_t* num_points, int64_t V, int32_t P, int32_t C, int32_t num_features,
                        float* mean);

/* ------------------------------------------------------------------------------------
 * The pillar encoders' point decoration (an addition inside ABI 6): what the pillar detectors run between voxelization and their
 * first nn.Linear.  No gradient (the inputs are raw points), no float atomics, no host read; every output element is written exactly
 * once.  Every multiply, add, subtract, divide and root below is ONE correctly rounded fp32 operation, never contracted.
 * voxel_size and offset (3 floats each, x y z) lie in HOST memory and are read during the call; the caller computes
 * offset_k = voxel_size_k / 2 + range_min_k in double and rounds it once.
 *
 * gd3d_point_voxel_stats : PointVoxelStatsCalculator.forward (models/voxel_encoders/utils.py:48-89) and the cat of
 *   DynamicPillarFeatureNet.forward (pillar_encoder.py:215-216), two launches (one when no flag needs the table).
 *   points (N, >= C) fp32, row i at points + i * row_stride, columns 0, 1, 2 = x, y, z.  coors (N, ndim) int32 or int64
 *   (coors_is_int64), 3 <= ndim <= 8: the last three columns are z, y, x.  map (N) / counts (V) / order (N) / seg (V + 1): what
 *   vox_index_build returns — the voxel of each point (-1, or anything outside [0, V): a dropped point), the points per voxel, the
 *   point ids grouped by voxel in ascending id, and the bounds of each voxel's run in `order`.
 *   Output row i at out + i * out_stride, the columns in this order, each group present iff its flag is set:
 *     3  always                    x, y, z
 *     3  GD3D_PVS_CLUSTER_CENTER   c = the mean of the xyz rows of the point's voxel: the voxel's points in ascending point index
 *                                  added IN SEQUENCE to +0, then ONE division by (float)count — the bits of vox_scatter_reduce's mean
 *     3  GD3D_PVS_CLUSTER_OFFSET   d = xyz - c
 *     9  GD3D_PVS_COVARIANCE       at 3a + b the mean, same sequence, of d_a * d_b, d taken from the ROUNDED c (two passes)
 *     3  GD3D_PVS_VOXEL_CENTER     ctr_k = (float)coor_k * voxel_size_k + offset_k, x y z from coors columns -1, -2, -3
 *     3  GD3D_PVS_VOXEL_OFFSET     xyz - ctr
 *     1  GD3D_PVS_POINT_COUNT      (float)count of the point's voxel
 *   C-3  GD3D_PVS_APPEND           columns 3 .. C-1 of the point copied through
 *   A dropped point gets c = +0, d = xyz - 0, covariance +0, count 0, and ctr from ITS OWN coors row, whatever it holds.  NaN and inf
 *   propagate as written: a NaN point poisons the means of its own voxel only.
 *   table: V * (12 with the covariance, else 3) floats of workspace (voxel row: mean xyz, then the covariance); NULL when neither of
 *   the first three flags is set.  16-byte stores where out is 16-byte aligned and either contiguous (out_stride == width) or both the
 *   width and out_stride are multiples of 4; 4-byte stores otherwise: the same bits.
 *   C < 3, row_stride < C, ndim < 3, out_stride < width, an unknown flag, V > N: GD3D_E_BADARG; N > 2^31 - 1, C > 256, ndim > 8:
 *   GD3D_E_TOOLARGE.
 * gd3d_pillar_decorate : the decoration of PillarFeatureNet.forward (pillar_encoder.py:105-153, legacy=False), one launch.
 *   features (V, P, C) fp32, num_points (V) int32, coors (V, 4) int32 = (b, z, y, x) -> out (V, P, width), width = C +
 *   3 (GD3D_PD_CLUSTER_CENTER) + 3 (GD3D_PD_VOXEL_CENTER) + 1 (GD3D_PD_DISTANCE).  For slots p < n = min(max(num_points, 0), P): the C
 *   columns copied; xyz - mean, the mean being slots 0, 1, 2, .. added in sequence to +0, then one division by (float)n
 *   (gd3d_voxel_mean's sequence); xyz - ((float)coor * voxel_size + offset) with x, y, z from coors columns 3, 2, 1;
 *   sqrt((x*x + y*y) + z*z).  Every other slot is written as +0 and its input is NOT read (the reference multiplies by a 0 / 1 mask:
 *   -0, or NaN for garbage and for voxels without points).  P < 1, C < 3, an unknown flag: GD3D_E_BADARG; V > 2^31 - 1, C > 256,
 *   P * (C + 7) > 2^30: GD3D_E_TOOLARGE.
 * `_cpu` twins (csrc/pillar_feat_cpu.cpp): the same contracts on HOST memory on the calling thread; every output is BIT-IDENTICAL to
 *   the kernels' (NaN payloads aside).
 * ---------------------------------------------------------------------------------- */
enum {
  GD3D_PVS_CLUSTER_CENTER = 1, GD3D_PVS_CLUSTER_OFFSET = 2, GD3D_PVS_COVARIANCE = 4, GD3D_PVS_VOXEL_CENTER = 8,
  GD3D_PVS_VOXEL_OFFSET = 16, GD3D_PVS_POINT_COUNT = 32, GD3D_PVS_APPEND = 64, GD3D_PVS_ALL = 127
};
enum { GD3D_PD_CLUSTER_CENTER = 1, GD3D_PD_VOXEL_CENTER = 2, GD3D_PD_DISTANCE = 4, GD3D_PD_ALL = 7 };
int gd3d_point_voxel_stats(const float* points, int64_t N, int64_t row_stride, int32_t C, const void* coors, int32_t coors_is_int64,
                           int32_t ndim, const int32_t* map, const int32_t* counts, const int32_t* order, const int32_t* seg,
                           int64_t V, const float* voxel_size, const float* offset, int32_t flags, float* table, float* out,
                           int64_t out_stride, void* stream);
int gd3d_pillar_decorate(const float* features, const int32_t* num_points, const int32_t* coors, int64_t V, int32_t P, int32_t C,
                         const float* voxel_size, const float* offset, int32_t flags, float* out, void* stream);
int gd3d_point_voxel_stats_cpu(const float* points, int64_t N, int64_t row_stride, int32_t C, const void* coors,
                               int32_t coors_is_int64, int32_t ndim, const int32_t* map, const int32_t* counts, const int32_t* order,
                               const int32_t* seg, int64_t V, const float* voxel_size, const float* offset, int32_t flags,
                               float* table, float* out, int64_t out_stride);
int gd3d_pillar_decorate_cpu(const float* features, const int32_t* num_points, const int32_t* coors, int64_t V, int32_t P, int32_t C,
                             const float* voxel_size, const float* offset, int32_t flags, float* out);

/* ------------------------------------------------------------------------------------
 * The multi-view pillar encoder's view ops (an addition inside ABI 6): PillarODCenterPoint.voxelize / voxelize_view with the
 * to_cylindrical / to_spherical transforms (models/detectors/pillar_od.py:24-70), mmdet3d's PointPillarsScatter (restated: mmdet3d is
 * not pinned) and the per-sample grid_sample loop of SingleViewNet.forward (models/voxel_encoders/pillar_mvf_encoder.py:88-105).  No
 * host read-back.  Every multiply, add, subtract, divide and root below is ONE correctly rounded fp32 operation, never contracted.
 *
 * gd3d_multi_view_voxelize : one launch; every point is read once and all views are written.
 *   points (N, >= C) fp32, row i at points + i * row_stride, columns 0, 1, 2 = x, y, z; points_batch_cnt (B) int32 as for
 *   gd3d_hard_voxelize.  Per view k < num_views (1 .. 4), in HOST memory, read during the call: view_kinds[k] = GD3D_VIEW_*,
 *   voxel_sizes / range_mins / grid_sizes (3 values per view: x y z of the TRANSFORMED coordinates; grid as for gd3d_hard_voxelize),
 *   view_points[k] (N, C) fp32 or NULL, view_coors[k] (N, 4) int32 or NULL (the three geometry arrays may be NULL when every
 *   view_coors[k] is).  The transformed point (t0, t1, t2):
 *     cartesian   : (x, y, z)
 *     cylindrical : s = x*x + y*y;  rho = sqrtf(s);  phi = fx_atan2f(y, x)                                -> (phi, z, rho)
 *     spherical   : s2 = x*x + y*y;  r2 = sqrtf(s2);  rho = sqrtf(s2 + z*z);  yaw = fx_atan2f(y, x);
 *                   pitch = fx_atan2f(z, r2)                                                               -> (yaw, pitch, rho)
 *   fx_atan2f is the library's fixed-sequence polynomial (csrc/rbox_device.h), the same on both targets; fx_atan2f(0, 0) = 0.  The
 *   reference's pitch is asin(z / rho) — the same angle, NaN at the origin where this form gives 0: restated, not matched.
 *   view_points row i = (t0, t1, t2, columns 3 .. C-1 of the point copied).  view_coors row i = [b, z, y, x] with b the row's sample
 *   and the cell f_j = floor((t_j - range_min_j) / voxel_size_j) of gd3d_hard_voxelize, kept iff 0 <= f_j < grid_j on all three axes,
 *   compared as floats before any conversion; a dropped point (outside the grid, or a non-finite transformed coordinate) is
 *   [b, -1, -1, -1] — the reference's F.pad writes the id into every row of a sample — and only a row of NO sample (past the counts'
 *   sum) is all -1.  NOT gd3d_dynamic_voxelize's layout, which is all -1 for every dropped point.  For a row with a non-finite input
 *   coordinate the three transformed values are unspecified, its coors are [b, -1, -1, -1], its trailing columns are copied.
 *   num_views outside [1, 4], an unknown kind, C < 3, row_stride < C: GD3D_E_BADARG; N > 2^31 - 1, C > 256, B > 1024, a grid axis >
 *   2^24: GD3D_E_TOOLARGE.  N == 0 launches nothing.
 * gd3d_pillar_scatter : canvas (B, C, ny, nx) fp32 in `layout` (0: contiguous NCHW, 1: channels last) = zeros, then
 *   canvas[b, :, y, x] = voxel_features (V, C)[v] for every row v of coors (V, coors_cols) int32 / int64: coors_cols 4 = [b, z, y, x],
 *   3 = [z, y, x] with b = 0 (B must be 0 or 1).  z is not read.  A row with b outside [0, B), y outside [0, ny) or x outside [0, nx)
 *   is skipped.  A fill and one launch; every element is written.  Rows must be unique per (b, y, x): the value at a duplicated cell
 *   is one of its rows (the twin: the last).  Channels last with C % 4 == 0 and 16-byte aligned bases takes 16-byte accesses,
 *   everything else 4-byte ones; NCHW stages 64 voxels x 64 channels through LDS.  The same values in every form.
 *   ny, nx >= 1, C >= 1 (GD3D_E_BADARG); V > 2^31 - 1, ny or nx > 2^24 (GD3D_E_TOOLARGE).  B == 0 launches nothing, V == 0 only the fill.
 * gd3d_pillar_scatter_backward : grad_features (V, C)[v] = grad_canvas[b, :, y, x], zeros for a skipped row: one launch, a gather, no
 *   atomics; every element is written.
 * gd3d_view_sample : out (N, C) fp32 contiguous = the bilinear sample of view_map (B, C, H, W) fp32 in `layout` at each point's xy —
 *   grid_sample(align_corners=False, padding_mode='zeros') on the reference's grid, for all samples in one launch.  Point n: x, y at
 *   pts_xyz[n * xyz_stride + 0 | 1]; its sample at ids[n * id_stride] (int32, or int64 with ids_is_int64) — column 0 of the (N, 4)
 *   coors with id_stride 4, or an id vector with id_stride 1.  half_x = (float)((hi_x - lo_x) / 2.0) computed by the caller in double
 *   and rounded once; likewise half_y.  Per point, per axis (n = W for x, H for y):
 *     g   = (v - lo) / half - 1
 *     pix = ((g + 1) * (float)n - 1) / 2
 *   reach = ix > -1 && ix < (float)W && iy > -1 && iy < (float)H && 0 <= id < B     (floats compared BEFORE any conversion)
 *     x0 = floor(ix), x1 = x0 + 1, y0 = floor(iy), y1 = y0 + 1
 *     w_nw = (x1 - ix) * (y1 - iy),  w_ne = (ix - x0) * (y1 - iy),  w_sw = (x1 - ix) * (iy - y0),  w_se = (ix - x0) * (iy - y0)
 *     out[c] = ((v_nw*w_nw + v_ne*w_ne) + v_sw*w_sw) + v_se*w_se, the value of a cell outside the map being 0.
 *   Without reach (outside, a non-finite coordinate, an id outside [0, B)) the row is 0 — for the id case the reference leaves
 *   uninitialised memory: restated, not matched.  No index leaves the map for any input.  H, W >= 1, half > 0 and finite, C >= 1,
 *   strides >= 0 (GD3D_E_BADARG); N > 2^31 - 1, H or W > 2^24 (GD3D_E_TOOLARGE).  Channels last with C % 4 == 0 and 16-byte aligned
 *   view_map / out takes 16-byte accesses, everything else 4-byte ones: the same bits, and the same bits for both layouts.
 * gd3d_view_sample_backward : grad_map (B, C, H, W) in `layout` = sum over the points of grad_out (N, C)[n, c] * weight into the (at
 *   most four) cells in the map; EVERY element is written.  A fill and one launch of fp32 atomic adds, lanes along C: where several
 *   points share a cell the last bits depend on the order of arrival.  workspace: NULL, or B*C*H*W floats; with layout 0 and a
 *   workspace the sums are made in the workspace in channels-last order (256 contiguous bytes per wave-instruction at C = 64) and one
 *   tiled transpose then writes every element of the NCHW gradient (three launches).  No gradient for the points.  B == 0 launches
 *   nothing, N == 0 only the fill.
 * `_cpu` twins (csrc/view_net_cpu.cpp): the same contracts on HOST memory on the calling thread; every output BIT-IDENTICAL to the
 *   kernels', except the sampling backward, which is sequential (points in order, neighbours nw, ne, sw, se); workspace is ignored.
 * ---------------------------------------------------------------------------------- */
enum { GD3D_VIEW_CARTESIAN = 0, GD3D_VIEW_CYLINDRICAL = 1, GD3D_VIEW_SPHERICAL = 2 };
int gd3d_multi_view_voxelize(const float* points, int64_t N, int64_t row_stride, int32_t C, const int32_t* points_batch_cnt, int32_t B,
                             int32_t num_views, const int32_t* view_kinds, const float* voxel_sizes, const float* range_mins,
                             const int32_t* grid_sizes, float* const* view_points, int32_t* const* view_coors, void* stream);
int gd3d_pillar_scatter(const float* voxel_features, const void* coors, int32_t coors_is_int64, int32_t coors_cols, int32_t layout,
                        int64_t V, int64_t C, int64_t B, int64_t ny, int64_t nx, float* canvas, void* stream);
int gd3d_pillar_scatter_backward(const float* grad_canvas, const void* coors, int32_t coors_is_int64, int32_t coors_cols,
                                 int32_t layout, int64_t V, int64_t C, int64_t B, int64_t ny, int64_t nx, float* grad_features,
                                 void* stream);
int gd3d_view_sample(const float* pts_xyz, int64_t xyz_stride, const void* ids, int32_t ids_is_int64, int64_t id_stride,
                     const float* view_map, int32_t layout, int64_t N, int64_t B, int64_t C, int64_t H, int64_t W, float lo_x,
                     float half_x, float lo_y, float half_y, float* out, void* stream);
int gd3d_view_sample_backward(const float* grad_out, const float* pts_xyz, int64_t xyz_stride, const void* ids, int32_t ids_is_int64,
                              int64_t id_stride, int32_t layout, int64_t N, int64_t B, int64_t C, int64_t H, int64_t W, float lo_x,
                              float half_x, float lo_y, float half_y, float* workspace, float* grad_map, void* stream);
int gd3d_multi_view_voxelize_cpu(const float* points, int64_t N, int64_t row_stride, int32_t C, const int32_t* points_batch_cnt,
                                 int32_t B, int32_t num_views, const int32_t* view_kinds, const float* voxel_sizes,
                                 const float* range_mins, const int32_t* grid_sizes, float* const* view_points,
                                 int32_t* const* view_coors);
int gd3d_pillar_scatter_cpu(const float* voxel_features, const void* coors, int32_t coors_is_int64, int32_t coors_cols, int32_t layout,
                            int64_t V, int64_t C, int64_t B, int64_t ny, int64_t nx, float* canvas);
int gd3d_pillar_scatter_backward_cpu(const float* grad_canvas, const void* coors, int32_t coors_is_int64, int32_t coors_cols,
                                     int32_t layout, int64_t V, int64_t C, int64_t B, int64_t ny, int64_t nx, float* grad_features);
int gd3d_view_sample_cpu(const float* pts_xyz, int64_t xyz_stride, const void* ids, int32_t ids_is_int64, int64_t id_stride,
                         const float* view_map, int32_t layout, int64_t N, int64_t B, int64_t C, int64_t H, int64_t W, float lo_x,
                         float half_x, float lo_y, float half_y, float* out);
int gd3d_view_sample_backward_cpu(const float* grad_out, const float* pts_xyz, int64_t xyz_stride, const void* ids,
                                  int32_t ids_is_int64, int64_t id_stride, int32_t layout, int64_t N, int64_t B, int64_t C, int64_t H,
                                  int64_t W, float lo_x, float half_x, float lo_y, float half_y, float* workspace, float* grad_map);

/* ------------------------------------------------------------------------------------
 * The SimOTA BEV assigner (an addition inside ABI 6): SimOTABEVAssigner.assign (core/bbox/assigners/sim_ota_3d_assigner.py:34-211)
 * for a whole batch as a fill and three launches — no host read, no data-dependent allocation, no priors x gts matrix in memory,
 * the same under graph capture and replay, independent of the workgroup schedule.  Every multiply, add, subtract, divide and root
 * below is ONE correctly rounded fp32 operation, never contracted; sin / cos / atan2 / log are the library's fixed polynomial
 * sequences (fx_sincosf, fx_atan2f: csrc/rbox_device.h; fx_logf: csrc/fx_log.h), the same on both targets.
 *   fx_logf: exponent extraction, s = f / (2 + f), a degree-4 polynomial in s^2.  Against fp64 log, correctly rounded, on 2^20
 *   log-uniform values of [1e-8, 2], every binade edge and the 4096 values next below 1: at most 0.80 ulp (measured 0.795; the host
 *   libm's logf on the same sample: 0.795).
 *
 * Stacked operands: pred_scores (P, C) probabilities, decoded_bboxes (P, 7), gt_bboxes (G, 7) rows [x, y, z, dx, dy, dz, yaw] with z
 * the BOTTOM face, gt_labels (G) int64; prior_batch_cnt / gt_batch_cnt (B) int32 on the device cut the rows into samples, every
 * count clamped to the rows left and never read back; rows past the counts' sum belong to no sample (all background).  priors:
 * row r at priors + r * prior_stride, columns 0 and 1 = x, y.  shared_priors 0: prior_rows == P, one row per stacked row;
 * shared_priors 1: ONE grid of prior_rows rows for every sample, prior n of a sample reads row n (a sample's rows past prior_rows
 * are background).  Of a sample's gts only the first G_cap take part.
 * Per sample, prior p (index within the sample) and gt g:
 *   1. in_gt = the x / y part of the points-in-boxes test (gd3d_pib_all) on the gt's BEV rectangle: sx = x - gx, sy = y - gy,
 *      (s, c) = fx_sincosf(-yaw), lx = sx*c + sy*(-s), ly = sx*s + sy*c, |lx| < dx/2 and |ly| < dy/2 STRICTLY; z is not read.
 *      in_ct = |x - gx| < center_radius and |y - gy| < center_radius.  A NaN coordinate is in nothing.  (A yaw of NaN or +-inf: in
 *      nothing, no overlap.  A finite |yaw| beyond 2^31 quarter turns leaves fx_sincosf's quadrant unspecified.)
 *      p is a CANDIDATE when some g has in_gt | in_ct; V = the sample's candidates.  both = in_gt & in_ct.
 *   2. iou = the bits of gd3d_roi_iou3d(decoded[p], gt[g]), NaN and negative values mapped to +0.
 *   3. cls = the sum over c = 0 .. C-1, ascending, into +0 of -(t*max(fx_logf(s), -100) + (1 - t)*max(fx_logf(1 - s), -100)),
 *      s = sqrtf(score clamped into [0, 1], NaN to 0), t = 1 if c == label[g] else 0 (a label outside [0, C): t = 0 throughout).
 *   4. cost = cls*cls_weight + (-fx_logf(iou + 1e-8f))*iou_weight; where `both`: cost < match_init ? cost : match_init (so a NaN
 *      cost becomes match_init there).
 *   5. K = min(candidate_topk, V); sum = the K largest iou of g over the candidates, added in descending order to +0;
 *      k = 1 if !(sum >= 1), K if sum >= K, else (int)sum.
 *   6. g takes the k candidates of smallest cost: costs ordered as fp32 values with -0 == +0 and NaN above everything, ties to the
 *      LOWER prior index.
 *   7. a prior taken by more than one gt goes to the gt of smallest cost over ALL (first G_cap) gts of the sample, ties to the LOWER
 *      gt index.
 * Outputs, EVERY element written by every call: gt_inds (P) int64 0 = background, g + 1 otherwise (g within the sample); labels (P)
 * int64 = label[g] or -1; max_overlaps (P) = iou with the assigned gt or -1e8; pos_cnt (B) int32; pos_inds / pos_gt_inds
 * (B, G_cap * candidate_topk) int64: the sample's positives in ascending prior index as ROWS of the stacked operands
 * (decoded_bboxes[pos_inds], gt_bboxes[pos_gt_inds]), padded with -1.  A sample without gts, priors or candidates is background.
 * workspace: gd3d_simota_workspace_bytes(P, B, G_cap, candidate_topk) bytes, O(P + B * G_cap * candidate_topk), from shapes alone;
 * the call writes nothing outside it.  B < 1, C < 1, candidate_topk < 1, prior_stride < 2, a NaN parameter, prior_rows != P
 * without shared_priors, a short workspace: GD3D_E_BADARG.  P, G > 2^24, B > 1024, C > 32, candidate_topk > 32, G_cap > 1024,
 * G_cap * candidate_topk > 16384: GD3D_E_TOOLARGE.
 * `_cpu` twin (csrc/simota_cpu.cpp): the same contract on HOST memory on the calling thread, every output BIT-IDENTICAL to the
 *   kernels'; workspace is ignored.
 * ---------------------------------------------------------------------------------- */
size_t gd3d_simota_workspace_bytes(int64_t P, int32_t B, int32_t G_cap, int32_t candidate_topk);
int gd3d_simota_assign(const float* pred_scores, const float* decoded_bboxes, const float* priors, int64_t prior_rows,
                       int64_t prior_stride, int32_t shared_priors, const int32_t* prior_batch_cnt, int64_t P, const float* gt_bboxes,
                       const int64_t* gt_labels, const int32_t* gt_batch_cnt, int64_t G, int32_t B, int32_t C, int32_t G_cap,
                       float center_radius, int32_t candidate_topk, float iou_weight, float cls_weight, float match_init,
                       int64_t* gt_inds, int64_t* labels, float* max_overlaps, int32_t* pos_cnt, int64_t* pos_inds,
                       int64_t* pos_gt_inds, void* workspace, size_t workspace_bytes, void* stream);
int gd3d_simota_assign_cpu(const float* pred_scores, const float* decoded_bboxes, const float* priors, int64_t prior_rows,
                           int64_t prior_stride, int32_t shared_priors, const int32_t* prior_batch_cnt, int64_t P,
                           const float* gt_bboxes, const int64_t* gt_labels, const int32_t* gt_batch_cnt, int64_t G, int32_t B,
                           int32_t C, int32_t G_cap, float center_radius, int32_t candidate_topk, float iou_weight, float cls_weight,
                           float match_init, int64_t* gt_inds, int64_t* labels, float* max_overlaps, int32_t* pos_cnt,
                           int64_t* pos_inds, int64_t* pos_gt_inds, void* workspace, size_t workspace_bytes);

/* ------------------------------------------------------------------------------------
 * Sparse 3D convolution (an addition inside ABI 6): spconv 1.x's SubMConv3d / SparseConv3d as mmdet3d's SparseEncoder and the
 * reference's MlvlSparseEncoder (models/middle_encoders/mlvl_sparse_encoder.py:11-32) use them, and SparseConvTensor.dense().
 * Neither mmdet3d nor spconv is pinned by the reference: the op is RESTATED here.  A sparse convolution equals the dense conv3d of
 * the densified input read at the active output sites; that is the oracle of the tests.  fp32 only, dilation 1 only.
 *
 * coors (N, 4) int32 rows [b, z, y, x]; spatial_shape, kernel_size, stride, padding: 3 HOST values each, (z, y, x), read during the
 * call.  K = kz*ky*kx <= 27; offset j = (a*ky + b)*kx + c with a over kz slowest: spconv 1.x's (kz, ky, kx, Cin, Cout) weight stored as
 * (K, Cin, Cout) fp32.  A row is INACTIVE when any entry is negative, b >= B, or a coordinate lies outside spatial_shape (the tail
 * rows of gd3d_hard_voxelize are such rows): it produces no output, is never a neighbour and gets a zero gradient.  Active rows
 * must be unique; with duplicates nothing faults and a look-up finds the LOWEST row of the cell.  Keys are 64-bit,
 * ((b*D + z)*H + y)*W + x, and a neighbour's coordinate is range-checked per axis BEFORE it is linearised: x = W-1 has no x+1
 * neighbour in the next row, the last cell of sample b none in sample b+1.
 *   subm = 1 : every kernel extent odd, stride 1, padding k/2 on every axis, else GD3D_E_BADARG.  R = N output rows,
 *     out_coors = coors (copied as they are), nbr[o, j] = the input row at (b, z - kz/2 + a, y - ky/2 + b', x - kx/2 + c) or -1 (all -1
 *     for an inactive row), num = {N, N}, out_batch_cnt[b] = the active rows of sample b.  nbr_t is not written (may be NULL): for
 *     unique rows nbr_t[i, j] = nbr[i, K-1-j].
 *   subm = 0 : out_shape = floor((n + 2p - k) / s) + 1 per axis (0 where the kernel does not fit: no output, every count zero).  The active outputs are the cells
 *     (b, oz, oy, ox) inside out_shape for which some active input and some offset satisfy in = o*s - p + off on every axis;
 *     out_coors (R, 4), R = max_out, holds them in ascending (b, z, y, x) order (samples stay grouped); num = {rows kept, true count},
 *     rows kept = min(true count, max_out): the LOWEST keys are kept.  Rows at and past the kept count: coors -1, nbr -1.
 *     nbr (R, K)[o, j] = the input row at o*s - p + off_j or -1; nbr_t (N, K)[i, j] = the kept output row o with nbr[o, j] == i, or -1
 *     (never a dropped row).  out_batch_cnt[b] = the kept rows of sample b.
 *   One stream-ordered run of launches, no host read: keys, rocPRIM's stable radix sort of (key, row), look-ups by lower bound; for
 *   subm = 0 also a sort of the N*K candidate output keys, head flags, a scan, a compaction.  workspace:
 *   gd3d_sparse_conv_index_workspace_bytes(N, K, subm) bytes, 256-byte aligned.  N == 0 writes the counts (zeros) and the tail rows.
 *   N*K and R*K > 2^31 - 1, an extent > 2^24, K > 27, B*D*H*W >= 2^62: GD3D_E_TOOLARGE.
 * gd3d_sparse_conv_forward : out (R, Cout)[o, :] = sum over j with nbr[o, j] >= 0 of features (N, Cin)[nbr[o, j], :] . weight[j]
 *   (+ bias), fp32 multiply-adds.  EVERY row of out is written; a row without a valid neighbour (an inactive row, a tail row) and a row
 *   at or past num[0] (num nullable, device) is ZERO, bias or not.  One launch, a workgroup per 64 rows x 16, 32 or 64 channels, no atomics: the
 *   same bits from run to run.  An entry of nbr outside [0, N) counts as -1.
 * gd3d_sparse_conv_backward_input : grad_features (N, Cin)[i, :] = sum over j with t[i, j] >= 0 of grad_out (R, Cout)[t[i, j], :] .
 *   weight[j]^T, t[i, j] = table[i, j] (flip = 0: table = nbr_t) or table[i, K-1-j] (flip = 1: table = nbr of a submanifold index,
 *   N == R).  The forward kernel over the transposed table and weight; every row is written.
 * gd3d_sparse_conv_backward_weight : grad_weight (K, Cin, Cout)[j] = sum over o < num[0] with nbr[o, j] >= 0 of
 *   features[nbr[o, j], :]^T . grad_out[o, :]; grad_bias (Cout, nullable) = the column sums of grad_out over the rows o < num[0]
 *   that have a valid neighbour.  Two stages: partial sums per chunk of rows in the workspace
 *   (gd3d_sparse_conv_backward_weight_workspace_bytes(R, K, Cin, Cout), 256-byte aligned, at most 64 chunks and 64 MiB), then one
 *   launch that adds the chunks in ascending order.  No atomics: the same bits from run to run.
 * gd3d_sparse_to_dense : dense (B, C, D, H, W) fp32 = zeros, then dense[b, :, z, y, x] = features (N, C)[row] for every active row: a
 *   fill and one launch (gd3d_pillar_scatter's 3D sibling).  _backward: grad_features[row] = grad_dense[b, :, z, y, x], zeros for an
 *   inactive row: one gather, every element written.
 * Cin, Cout, C, K >= 1 (GD3D_E_BADARG); Cin, Cout, C <= 256, K <= 27, N, R <= 2^31 - 1 (GD3D_E_TOOLARGE).  R == 0 (forward), N == 0
 * (backward_input) launch nothing.
 * `_cpu` twins (csrc/sparse_conv_cpu.cpp): the same contracts on HOST memory on the calling thread; workspace is ignored.  Every
 *   INTEGER output is bit-identical to the kernels'; the values are summed offset by offset, channel by channel — another order than
 *   the kernels' tiles — and agree with them to fp32 rounding, not to the bit.
 * ---------------------------------------------------------------------------------- */
size_t gd3d_sparse_conv_index_workspace_bytes(int64_t N, int32_t K, int32_t subm);
int gd3d_sparse_conv_index(const int32_t* coors, int64_t N, int32_t B, const int32_t* spatial_shape, const int32_t* kernel_size,
                           const int32_t* stride, const int32_t* padding, int32_t subm, int64_t max_out, void* workspace,
                           int32_t* out_coors, int32_t* nbr, int32_t* nbr_t, int64_t* num, int32_t* out_batch_cnt, void* stream);
int gd3d_sparse_conv_forward(const float* features, const float* weight, const float* bias, const int32_t* nbr, const int64_t* num,
                             int64_t N, int64_t R, int32_t K, int32_t Cin, int32_t Cout, float* out, void* stream);
int gd3d_sparse_conv_backward_input(const float* grad_out, const float* weight, const int32_t* table, int32_t flip, int64_t N,
                                    int64_t R, int32_t K, int32_t Cin, int32_t Cout, float* grad_features, void* stream);
size_t gd3d_sparse_conv_backward_weight_workspace_bytes(int64_t R, int32_t K, int32_t Cin, int32_t Cout);
int gd3d_sparse_conv_backward_weight(const float* features, const float* grad_out, const int32_t* nbr, const int64_t* num, int64_t N,
                                     int64_t R, int32_t K, int32_t Cin, int32_t Cout, void* workspace, float* grad_weight,
                                     float* grad_bias, void* stream);
int gd3d_sparse_to_dense(const float* features, const int32_t* coors, int64_t N, int32_t C, int32_t B, int32_t D, int32_t H, int32_t W,
                         float* dense, void* stream);
int gd3d_sparse_to_dense_backward(const float* grad_dense, const int32_t* coors, int64_t N, int32_t C, int32_t B, int32_t D, int32_t H,
                                  int32_t W, float* grad_features, void* stream);
int gd3d_sparse_conv_index_cpu(const int32_t* coors, int64_t N, int32_t B, const int32_t* spatial_shape, const int32_t* kernel_size,
                               const int32_t* stride, const int32_t* padding, int32_t subm, int64_t max_out, void* workspace,
                               int32_t* out_coors, int32_t* nbr, int32_t* nbr_t, int64_t* num, int32_t* out_batch_cnt);
int gd3d_sparse_conv_forward_cpu(const float* features, const float* weight, const float* bias, const int32_t* nbr, const int64_t* num,
                                 int64_t N, int64_t R, int32_t K, int32_t Cin, int32_t Cout, float* out);
int gd3d_sparse_conv_backward_input_cpu(const float* grad_out, const float* weight, const int32_t* table, int32_t flip, int64_t N,
                                        int64_t R, int32_t K, int32_t Cin, int32_t Cout, float* grad_features);
int gd3d_sparse_conv_backward_weight_cpu(const float* features, const float* grad_out, const int32_t* nbr, const int64_t* num, int64_t N,
                                         int64_t R, int32_t K, int32_t Cin, int32_t Cout, void* workspace, float* grad_weight,
                                         float* grad_bias);
int gd3d_sparse_to_dense_cpu(const float* features, const int32_t* coors, int64_t N, int32_t C, int32_t B, int32_t D, int32_t H,
                             int32_t W, float* dense);
int gd3d_sparse_to_dense_backward_cpu(const float* grad_dense, const int32_t* coors, int64_t N, int32_t C, int32_t B, int32_t D,
                                      int32_t H, int32_t W, float* grad_features);

/* ------------------------------------------------------------------------------------
 * Sparse 3D convolution on fp16 / bf16 operands (an addition inside ABI 6; csrc/sparse_conv_16.hip): the entries
 * above for half-precision training and inference, over the SAME tables of gd3d_sparse_conv_index.  dtype: GD3D_DTYPE_F16 (IEEE
 * binary16) or GD3D_DTYPE_BF16; anything else is GD3D_E_BADARG.  Every 16-bit pointer must be 2-byte aligned (GD3D_E_BADARG).
 * gd3d_sparse_conv_forward_16 : features (N, Cin), weight (K, Cin, Cout) and out (R, Cout) in `dtype`; bias (Cout) fp32, nullable.
 *   out = rn16(sum + bias): the products of the 16-bit operands are accumulated in fp32 (v_mfma_f32_16x16x32_{f16,bf16} on the
 *   device), the fp32 bias is added, and the result is rounded to nearest even ONCE.  The contract of gd3d_sparse_conv_forward:
 *   EVERY row of out is written; a row without a valid neighbour and a row at or past num[0] (num nullable, device) is ZERO, bias
 *   or not; an entry of nbr outside [0, N) counts as -1.  NaN and inf pass through; a sum beyond the type's range is inf, never
 *   saturated.  One launch, a workgroup per 128 rows x 16, 32 or 64 channels, no atomics: the same bits from run to run.  Every
 *   channel count 1..256 is accepted; Cin % 8 == 0 with a 16-byte aligned `features` takes 16-byte gathers, Cout % 8 == 0 with a
 *   16-byte aligned `out` 16-byte stores, anything else the element-wise form of the same arithmetic.
 * gd3d_sparse_conv_backward_input_16 : grad_out (R, Cout), weight and grad_features (N, Cin) in `dtype`; the forward kernel over the
 *   transposed table and weight (table, flip as in gd3d_sparse_conv_backward_input); every row is written.
 * gd3d_sparse_conv_backward_weight_16 : features and grad_out in `dtype`; grad_weight (K, Cin, Cout) and grad_bias (Cout, nullable)
 *   are FP32 — master weights receive unrounded gradients.  The operands are widened (their products are exact in fp32) and summed
 *   by gd3d_sparse_conv_backward_weight's two stages in its order; workspace:
 *   gd3d_sparse_conv_backward_weight_workspace_bytes(R, K, Cin, Cout) bytes, 256-byte aligned.
 * gd3d_sparse_conv_backward_weight_16_mfma (csrc/sparse_conv_wgrad_16.hip) : the same call — arguments, workspace,
 *   argument checks in the same order with the same codes, empty cases, fp32 outputs — with the per-chunk partial sums X^T gY taken on
 *   v_mfma_f32_16x16x32_{f16,bf16}: 32 rows a step, each of a workgroup's four waves on its own steps, the waves' sums added in
 *   ascending wave order, the chunks' in ascending chunk order by the same second stage.  A row without the neighbour at offset j, a
 *   row at or past num[0] and the channels past Cin / Cout enter as zeros on BOTH operands: a NaN in a row that offset j does not use
 *   does not reach grad_weight[j].  grad_bias is gd3d_sparse_conv_backward_weight_16's, bit for bit.  grad_weight has another order of
 *   addition than that entry: it agrees with it to the bound of DESIGN.md §3.29, and bit for bit wherever every partial sum is exact
 *   in fp32.  No atomics, no host read: the same bits from run to run and under graph replay.  Cin % 8 == 0 with a 16-byte aligned
 *   `features` (Cout, `grad_out`) takes 16-byte gathers, anything else the element-wise form of the same arithmetic.  Opt-in: nothing
 *   else calls it, and it has no `_cpu` twin.
 * gd3d_sparse_to_dense_16 / _backward_16 : gd3d_sparse_to_dense and its backward for 2-byte elements of either type (a fill and a
 *   copy: no dtype argument); dense (B, C, D, H, W) and grad_features (N, C) in the features' type.
 * Limits, error codes and the empty cases (R == 0, N == 0) are those of the fp32 entries.
 * `_cpu` twins (csrc/sparse_conv_16_cpu.cpp): the operands widened to fp32, the fp32 twin's loops, one rounding to nearest even;
 *   another summation order than the device's: the values agree to the tests' bound, not to the bit.
 * ---------------------------------------------------------------------------------- */
#define GD3D_DTYPE_F16 1
#define GD3D_DTYPE_BF16 2
int gd3d_sparse_conv_forward_16(const void* features, const void* weight, const float* bias, const int32_t* nbr, const int64_t* num,
                                int64_t N, int64_t R, int32_t K, int32_t Cin, int32_t Cout, int32_t dtype, void* out, void* stream);
int gd3d_sparse_conv_backward_input_16(const void* grad_out, const void* weight, const int32_t* table, int32_t flip, int64_t N,
                                       int64_t R, int32_t K, int32_t Cin, int32_t Cout, int32_t dtype, void* grad_features,
                                       void* stream);
int gd3d_sparse_conv_backward_weight_16(const void* features, const void* grad_out, const int32_t* nbr, const int64_t* num, int64_t N,
                                        int64_t R, int32_t K, int32_t Cin, int32_t Cout, int32_t dtype, void* workspace,
                                        float* grad_weight, float* grad_bias, void* stream);
int gd3d_sparse_conv_backward_weight_16_mfma(const void* features, const void* grad_out, const int32_t* nbr, const int64_t* num, int64_t N,
                                             int64_t R, int32_t K, int32_t Cin, int32_t Cout, int32_t dtype, void* workspace,
                                             float* grad_weight, float* grad_bias, void* stream);
int gd3d_sparse_to_dense_16(const void* features, const int32_t* coors, int64_t N, int32_t C, int32_t B, int32_t D, int32_t H, int32_t W,
                            void* dense, void* stream);
int gd3d_sparse_to_dense_backward_16(const void* grad_dense, const int32_t* coors, int64_t N, int32_t C, int32_t B, int32_t D, int32_t H,
                                     int32_t W, void* grad_features, void* stream);
int gd3d_sparse_conv_forward_16_cpu(const void* features, const void* weight, const float* bias, const int32_t* nbr, const int64_t* num,
                                    int64_t N, int64_t R, int32_t K, int32_t Cin, int32_t Cout, int32_t dtype, void* out);
int gd3d_sparse_conv_backward_input_16_cpu(const void* grad_out, const void* weight, const int32_t* table, int32_t flip, int64_t N,
                                           int64_t R, int32_t K, int32_t Cin, int32_t Cout, int32_t dtype, void* grad_features);
int gd3d_sparse_conv_backward_weight_16_cpu(const void* features, const void* grad_out, const int32_t* nbr, const int64_t* num,
                                            int64_t N, int64_t R, int32_t K, int32_t Cin, int32_t Cout, int32_t dtype, void* workspace,
                                            float* grad_weight, float* grad_bias);
int gd3d_sparse_to_dense_16_cpu(const void* features, const int32_t* coors, int64_t N, int32_t C, int32_t B, int32_t D, int32_t H,
                                int32_t W, void* dense);
int gd3d_sparse_to_dense_backward_16_cpu(const void* grad_dense, const int32_t* coors, int64_t N, int32_t C, int32_t B, int32_t D,
                                         int32_t H, int32_t W, void* grad_features);

/* ------------------------------------------------------------------------------------
 * Sparse 3D convolution with a fused epilogue (an addition inside ABI 6; csrc/sparse_conv.hip, csrc/sparse_conv_16.hip, DESIGN.md
 * §3.20): an eval-mode BatchNorm folded to a per-channel scale and shift, the residual add of a basic block and a ReLU inside the
 * forward launch, over the SAME tables.  The plain entries above are untouched: their launches keep their code and their bits.
 * gd3d_sparse_conv_forward_fused : features, weight, nbr, num, N, R, K, Cin, Cout, out as gd3d_sparse_conv_forward.  scale and shift:
 *   fp32 (Cout), each nullable.  residual: (R, Cout), nullable; it must not share a byte with out (GD3D_E_BADARG).  act: GD3D_ACT_NONE or
 *   GD3D_ACT_RELU, anything else GD3D_E_BADARG (nothing is written).  With acc the accumulated sum of gd3d_sparse_conv_forward,
 *   unchanged, every element of a row that has a valid neighbour is ONE fixed fp32 sequence:
 *     t = scale ? fmaf(acc, scale[c], shift ? shift[c] : 0) : acc + (shift ? shift[c] : 0)
 *     t = residual ? t + residual[o][c] : t
 *     t = act == GD3D_ACT_RELU ? (t < 0 ? 0 : t) : t            (a NaN passes, as torch.relu)
 *   A row without a valid neighbour (an inactive row, a row at or past num[0]) is ZERO whatever shift and residual hold; its residual
 *   row is not read.  scale == NULL, residual == NULL, GD3D_ACT_NONE gives gd3d_sparse_conv_forward's bits with bias = shift; so does
 *   a scale of ones.  One launch, no atomics: the same bits from run to run.
 * gd3d_sparse_conv_forward_fused_16 : features, weight, residual and out in `dtype`, scale and shift fp32.  The same sequence on the fp32
 *   accumulator with the residual widened, then ONE rounding to nearest even.  The residual is read 16 bytes a lane where Cout % 8 == 0 and
 *   its base is 16-byte aligned, element by element otherwise, whichever way out is stored: the same bits on every path.
 * Limits, error codes and the empty case (R == 0) are those of gd3d_sparse_conv_forward[_16].
 * `_cpu` twins: the twins' loops of the plain entries, then the sequence above (fmaf included; the 16-bit twin rounds once).
 * ---------------------------------------------------------------------------------- */
#define GD3D_ACT_NONE 0
#define GD3D_ACT_RELU 1
int gd3d_sparse_conv_forward_fused(const float* features, const float* weight, const float* scale, const float* shift, const float* residual,
                                   const int32_t* nbr, const int64_t* num, int64_t N, int64_t R, int32_t K, int32_t Cin, int32_t Cout,
                                   int32_t act, float* out, void* stream);
int gd3d_sparse_conv_forward_fused_16(const void* features, const void* weight, const float* scale, const float* shift, const void* residual,
                                      const int32_t* nbr, const int64_t* num, int64_t N, int64_t R, int32_t K, int32_t Cin, int32_t Cout,
                                      int32_t act, int32_t dtype, void* out, void* stream);
int gd3d_sparse_conv_forward_fused_cpu(const float* features, const float* weight, const float* scale, const float* shift,
                                       const float* residual, const int32_t* nbr, const int64_t* num, int64_t N, int64_t R, int32_t K,
                                       int32_t Cin, int32_t Cout, int32_t act, float* out);
int gd3d_sparse_conv_forward_fused_16_cpu(const void* features, const void* weight, const float* scale, const float* shift,
                                          const void* residual, const int32_t* nbr, const int64_t* num, int64_t N, int64_t R, int32_t K,
                                          int32_t Cin, int32_t Cout, int32_t act, int32_t dtype, void* out);

/* ------------------------------------------------------------------------------------
 * Batch normalisation over the LIVE rows of a sparse tensor, with the residual add and the ReLU of a basic block in the same pass (an
 * addition inside ABI 6; csrc/sparse_bn.hip, csrc/sparse_bn_common.h).  features, residual (nullable), out, grad_out,
 * grad_features, grad_residual (nullable): (R, C) in `dtype` — 0: fp32, GD3D_DTYPE_F16, GD3D_DTYPE_BF16 (widened on load, rounded to
 * nearest even once on store); every statistic, weight, bias and parameter gradient is fp32 (C).  coors (R, 4) int32 [b, z, y, x]: row i is
 * LIVE when all four entries are >= 0, b < B and (z, y, x) lies inside (D, H, W) — gd3d_sparse_conv_index's rule, read on the device;
 * n is the number of live rows, never read back.  1 <= C <= 256 (GD3D_E_TOOLARGE above), R < 2^31; act: GD3D_ACT_NONE / GD3D_ACT_RELU.
 * gd3d_sparse_bn_forward, training != 0: per channel mean and biased var over the live rows (per-tile mean and centred sums merged by
 *   Chan's formula in ascending tile order; never E[x^2] - E[x]^2), invstd = 1 / sqrt(var + eps), written to save_mean / save_invstd;
 *     out = act((x - mean) * (invstd * weight) + bias + residual)   on live rows (weight NULL: 1, bias NULL: 0),
 *     out = 0                                                         on dead rows, whatever features and residual hold there (a select).
 *   When n >= 2 and the pointer is not NULL: running_mean = (1 - momentum) running_mean + momentum mean, running_var likewise with
 *   var n / (n - 1), *num_batches_tracked += 1 — written by the finishing launch.  n < 2 leaves the three untouched (n = 0: out is all zero;
 *   n = 1: out = act(bias + residual) on the live row).  At most 3 launches, `workspace` of gd3d_sparse_bn_workspace_bytes(R, C) bytes.
 *   training == 0: out = act(x * scale + shift + residual) on live rows, scale = weight / sqrt(running_var + eps), shift = bias -
 *   running_mean * scale; 0 on dead rows; ONE launch; nothing else is written, workspace and save_* may be NULL.
 *   residual must not share a byte with out (GD3D_E_BADARG).  R == 0: save_mean = 0, save_invstd = 1 / sqrt(eps), nothing else.
 * gd3d_sparse_bn_backward: g = grad_out where the row is live and (act == GD3D_ACT_RELU) the saved `out` is > 0, else 0.
 *   grad_residual = g; grad_bias = sum g; grad_weight = sum g xhat, xhat = (x - mean) * invstd (each nullable);
 *   training != 0 (mean, invstd_or_var = save_mean, save_invstd): grad_features = weight invstd (g - sum g / n - xhat sum(g xhat) / n);
 *   training == 0 (mean, invstd_or_var = running_mean, running_var; a frozen BatchNorm): grad_features = g scale.
 *   Dead rows of grad_features and grad_residual are zero.  At most 3 launches (one in eval without parameter gradients).
 * No atomics, and the order of every sum depends on (R, C) and dtype alone: the same bits from run to run and under graph replay,
 * whatever the dead rows hold.  An operand whose base is 16-byte aligned, with C % 4 == 0 (fp32) or C % 8 == 0 (16 bits), is read and
 * written 16 bytes a lane; anything else element by element, with the same bits.
 * `_cpu` twins (csrc/sparse_bn_cpu.cpp): the same element sequences; the sums in fp64 per tile, rounded once — the tests' bound, not the bit.
 * ---------------------------------------------------------------------------------- */
size_t gd3d_sparse_bn_workspace_bytes(int64_t R, int32_t C);
int gd3d_sparse_bn_forward(const void* features, const int32_t* coors, const void* residual, const float* weight, const float* bias,
                           float* running_mean, float* running_var, int64_t* num_batches_tracked, int64_t R, int32_t C, int32_t B, int32_t D,
                           int32_t H, int32_t W, int32_t training, float momentum, float eps, int32_t act, int32_t dtype, void* workspace,
                           void* out, float* save_mean, float* save_invstd, void* stream);
int gd3d_sparse_bn_backward(const void* grad_out, const void* features, const void* out, const int32_t* coors, const float* weight,
                            const float* mean, const float* invstd_or_var, int64_t R, int32_t C, int32_t B, int32_t D, int32_t H, int32_t W,
                            int32_t training, float eps, int32_t act, int32_t dtype, void* workspace, void* grad_features, void* grad_residual,
                            float* grad_weight, float* grad_bias, void* stream);
int gd3d_sparse_bn_forward_cpu(const void* features, const int32_t* coors, const void* residual, const float* weight, const float* bias,
                               float* running_mean, float* running_var, int64_t* num_batches_tracked, int64_t R, int32_t C, int32_t B,
                               int32_t D, int32_t H, int32_t W, int32_t training, float momentum, float eps, int32_t act, int32_t dtype,
                               void* workspace, void* out, float* save_mean, float* save_invstd);
int gd3d_sparse_bn_backward_cpu(const void* grad_out, const void* features, const void* out, const int32_t* coors, const float* weight,
                                const float* mean, const float* invstd_or_var, int64_t R, int32_t C, int32_t B, int32_t D, int32_t H,
                                int32_t W, int32_t training, float eps, int32_t act, int32_t dtype, void* workspace, void* grad_features,
                                void* grad_residual, float* grad_weight, float* grad_bias);

/* ------------------------------------------------------------------------------------
 * Max pooling over the tables of gd3d_sparse_conv_index (spconv 1.x's SparseMaxPool3d; an addition inside ABI 6; csrc/sparse_pool.hip,
 * csrc/sparse_pool_common.h).  features, grad_features: (N, C); out, grad_out: (R, C), all in `dtype` — 0: fp32,
 * GD3D_DTYPE_F16, GD3D_DTYPE_BF16.  nbr (R, K), nbr_t (N, K) int32: the tables of a strided (not submanifold) index.  1 <= C <= 256,
 * 1 <= K <= 27 (GD3D_E_TOOLARGE above), N, R < 2^31.
 * gd3d_sparse_max_pool_forward: out[o, c] = max over the offsets j with 0 <= nbr[o, j] < N of features[nbr[o, j], c].  Every row is
 *   written; a row at or past num[0] (num nullable: every row counts) and a row without a valid neighbour are ZERO, not -inf.  The
 *   comparison is written out — a candidate replaces the maximum when it is greater or is a NaN — so a NaN in the window gives NaN
 *   (torch's max_pool3d rule; fmaxf would drop it) and a window of -inf gives -inf.  The output element is a COPY of an input element: no
 *   rounding in any type.
 * gd3d_sparse_max_pool_backward: grad_features[i, c] = the sum, in ascending j, over the offsets with o = nbr_t[i, j] in [0, R) and
 *   features[i, c] == out[o, c] of grad_out[o, c] — spconv 1.x's equality rule: EVERY tied input of a window receives the gradient; a NaN
 *   window compares unequal and passes none.  The sum is accumulated in fp32 and rounded once to a 16-bit dtype.  Every row is written;
 *   an inactive row, and one whose outputs were all dropped, is zero.
 * One launch each way, a gather in both directions: no atomics, the same bits from run to run and under graph replay.  An operand whose
 * base is 16-byte aligned, with C % 4 == 0 (fp32) or C % 8 == 0 (16 bits), is read and written 16 bytes a lane; anything else element by
 * element, with the same bits.  `_cpu` twins (csrc/sparse_pool_cpu.cpp): the same sequence per element, the same bits.
 * ---------------------------------------------------------------------------------- */
int gd3d_sparse_max_pool_forward(const void* features, const int32_t* nbr, const int64_t* num, int64_t N, int64_t R, int32_t K, int32_t C,
                                 int32_t dtype, void* out, void* stream);
int gd3d_sparse_max_pool_backward(const void* grad_out, const void* features, const void* out, const int32_t* nbr_t, int64_t N, int64_t R,
                                  int32_t K, int32_t C, int32_t dtype, void* grad_features, void* stream);
int gd3d_sparse_max_pool_forward_cpu(const void* features, const int32_t* nbr, const int64_t* num, int64_t N, int64_t R, int32_t K,
                                     int32_t C, int32_t dtype, void* out);
int gd3d_sparse_max_pool_backward_cpu(const void* grad_out, const void* features, const void* out, const int32_t* nbr_t, int64_t N,
                                      int64_t R, int32_t K, int32_t C, int32_t dtype, void* grad_features);

/* ------------------------------------------------------------------------------------
 * PV-RCNN's RPN proposal stage (an addition inside ABI 6): `rpn_head.get_bboxes(*rpn_outs, img_metas, proposal_cfg)` of
 * PVRCNN.forward_train / simple_test (models/detectors/pv_rcnn.py:115-125, :143-146), where rpn_head is mmdet3d's PartA2RPNHead
 * (get_bboxes_single + class_agnostic_nms; third party, absent, RESTATED from the published 0.x text, parity unpinned), for a
 * whole batch as a fill, nine launches and the batched NMS — no host read, static shapes, the same under graph capture and replay,
 * independent of the workgroup schedule.  Every multiply, add, subtract, divide and root below is ONE correctly rounded fp32
 * operation, never contracted; exp is the library's fixed sequence, the same on both targets.
 *   fx_expf (csrc/fx_exp.h): k = trunc(x * (1 / ln 2) +- 0.5), r = (x - k * LN2_HI) - k * LN2_LO, c = r - r^2 (P1 + r^2 P2),
 *   1 + (hi - (lo - r c / (2 - c))), scaled by 2^k on the bit pattern.  NaN -> NaN; x > 88.7228317 (0x42b17217) -> +inf; a result
 *   below the normal range (x < -87.3365402, 0xc2aeac4f) -> +0 EXACTLY, never a subnormal.  Against fp64 exp, correctly rounded,
 *   on 2^20 uniform arguments of the finite-result range, every multiple of ln 2 / 2 there +- 4 neighbours and the 4096 values
 *   either side of 0: at most 0.90 ulp (measured 0.880; the host libm's expf on the same sample: 0.502).
 *   sigmoid(x) = 1 / (1 + fx_expf(-x)).
 *
 * One level, sigmoid classification, box code size 7.  cls_score (B, A*C, H, W), bbox_pred (B, A*7, H, W), dir_cls_pred
 * (B, A*2, H, W) fp32 contiguous NCHW; anchors (N, 7), N = H*W*A, anchor n = (h*W + w)*A + a; the channel of class c is a*C + c
 * (likewise a*7 + k and a*2 + d).  cap = min(nms_pre, N) (nms_pre <= 0: N), M = min(nms_post, max_num).  Per sample:
 *   1. per anchor: best = the maximum of its C logits, label = the LOWEST class attaining it, dir = 1 iff dir_pred[1] >
 *      dir_pred[0].  An anchor with a NaN class logit is never a candidate.
 *   2. the candidates: the cap anchors (all, where fewer are without NaN) with the largest best, in descending order, equal
 *      logits (-0 == +0) by ASCENDING anchor index — a per-sample radix select on order-preserving 32-bit keys of the LOGIT, the
 *      boundary key's holders taken by ascending index, the survivors ordered by counting.  (The reference ranks the sigmoid
 *      VALUES with an unspecified tie order: the two orders differ only among logits whose sigmoid rounds to the same fp32.)
 *   3. per candidate: score = sigmoid(best); the box is DeltaXYZWLHRBBoxCoder.decode: za = az + ah / 2, diagonal =
 *      sqrt(al * al + aw * aw), x = t0 * diagonal + ax, y = t1 * diagonal + ay, z = t2 * ah + za, l = fx_expf(t4) * al,
 *      w = fx_expf(t3) * aw, h = fx_expf(t5) * ah, r = t6 + ar, z = z - h / 2, box = [x, y, z, w, l, h, r]; the NMS box is
 *      xywhr2xyxyr of [x, y, w, l, r]: [x - w / 2, y - l / 2, x + w / 2, y + l / 2, r].
 *   4. the candidates with score > score_thr, STRICTLY, take part in the NMS: their number cnt is counted on the device and the
 *      first cnt candidates of the order are taken (the passing candidates are a prefix of the order wherever the sigmoid's
 *      rounding is monotone).  use_rotate_nms != 0: rnms_batched mode 0 (rotated BEV IoU), else mode 1 (axis-aligned), at
 *      nms_thr, greedy in the selection order.
 *   5. the first min(num_keep, M) kept candidates are the sample's rows (the reference's "sort by score and cut to max_num" is
 *      the identity on a list that is already non-increasing); num_keep == -1 (the scan gave up) gives batch_cnt -1 and no row.
 *   6. on the kept rows: yaw = (v - floor(v / pi + dir_limit_offset) * pi) + dir_offset + pi * dir, v = yaw - dir_offset, pi the
 *      fp32 value; cls_preds[c] = sigmoid(logit_c) — the sigmoid scores in EVERY case.
 * Outputs, EVERY element written by every call, the samples packed back to back: boxes_3d (B*M, 7), scores_3d (B*M), labels_3d
 * (B*M) int64, cls_preds (B*M, C), rois (B*M, 8) = [batch id, box], batch_cnt (B) int32; rows past the counts' sum: batch id -1,
 * label -1, zeros (gd3d_roi_assign_sample's convention).  Optional (NULL: not written): cand_inds (B, cap) int64 the candidates'
 * anchor indices in the selection order, -1 past them; cand_cnt (B) int32 = cnt.
 * workspace: gd3d_rpn_proposal_workspace_bytes(B, A, C, H, W, nms_pre) bytes, from shapes alone (0: the shapes are refused).
 * B, A, C, H, W, nms_post or max_num < 1, a NaN parameter, a NULL operand, a short workspace: GD3D_E_BADARG.  C > 16, B > 1024,
 * N >= 2^30, cap > 16384: GD3D_E_TOOLARGE.
 * `_cpu` twin (csrc/rpn_proposal_cpu.cpp): the same contract on HOST memory on the calling thread, a stable sort and
 *   rnms_bev_cpu / rnms_normal_bev_cpu; every output BIT-IDENTICAL to the kernels'; workspace is ignored.
 * ---------------------------------------------------------------------------------- */
size_t gd3d_rpn_proposal_workspace_bytes(int32_t B, int32_t A, int32_t C, int32_t H, int32_t W, int32_t nms_pre);
int gd3d_rpn_proposals(const float* cls_score, const float* bbox_pred, const float* dir_cls_pred, const float* anchors, int32_t B,
                       int32_t A, int32_t C, int32_t H, int32_t W, int32_t nms_pre, int32_t nms_post, int32_t max_num, float nms_thr,
                       float score_thr, int32_t use_rotate_nms, float dir_offset, float dir_limit_offset, float* boxes_3d,
                       float* scores_3d, int64_t* labels_3d, float* cls_preds, float* rois, int32_t* batch_cnt, int64_t* cand_inds,
                       int32_t* cand_cnt, void* workspace, size_t workspace_bytes, void* stream);
int gd3d_rpn_proposals_cpu(const float* cls_score, const float* bbox_pred, const float* dir_cls_pred, const float* anchors, int32_t B,
                           int32_t A, int32_t C, int32_t H, int32_t W, int32_t nms_pre, int32_t nms_post, int32_t max_num,
                           float nms_thr, float score_thr, int32_t use_rotate_nms, float dir_offset, float dir_limit_offset,
                           float* boxes_3d, float* scores_3d, int64_t* labels_3d, float* cls_preds, float* rois, int32_t* batch_cnt,
                           int64_t* cand_inds, int32_t* cand_cnt, void* workspace, size_t workspace_bytes);

/* Library identification: returns GD3D_ABI_VERSION; *arch (if non-NULL) receives a static
 * string naming the code-object target, e.g. "gfx950". */
int gd3d_abi_version(const char** arch);

#ifdef __cplusplus
}
#endif
#endif /* GD3D_H_ */
