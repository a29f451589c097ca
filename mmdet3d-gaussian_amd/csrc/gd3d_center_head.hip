// gd3d_center_head.hip — the CenterGDHead regression losses of all tasks for gfx950: the staging kernel, the two
// deterministic gradient-accumulation kernels, the scaling kernel, and their C-ABI entry points (include/gd3d.h,
// gd3d_center_head_*).
#include "gd3d_loss_common.h"

namespace gd3d {

// CenterGDHead regression losses of ALL tasks in one launch (gd_centerpoint_head.py:402-441):
//   per task: pred = cat(reg, height, dim, yaw, dir[, vel])[b, :, y, x] gathered at the positives (:416-420, the cat and
//   the gather never materialise: a thread reads its 9/11 values straight from the NCHW head maps), pred_gd =
//   coder.decode(locs, pred)[:7] (:422-423), target = coder.encode(anno) (:409-411: [anno[:7], sin yaw, cos yaw, vel]),
//   loss_gd = GDLoss(pred_gd, target[:7], avg_factor) (:433-434), loss_l1 = L1Loss(pred[7:], target[7:], code_weights,
//   avg_factor) (:426-432).  Two objects of a task may share a cell (the reference's index backward accumulates), so the
//   gradient takes two steps, deterministic and without float atomics: this kernel stages every object's 11 gradient
//   values and counts the objects per cell (integer atomics); center_accum_kernel then writes single-object cells
//   directly and lets the lowest-index object of a shared cell add the cell's contributions in ascending object order.
// blockIdx.y = task; partials[(task * 2 + term) * pstride + block], term 0 = l1, 1 = gd.
constexpr int CENTER_MAX_TASKS = 8;
struct CenterTask {
  const float* maps[6];  // reg(2) height(1) dim(3) yaw(1) dir(2) vel(2); reg / vel nullable
  float* grads[6];       // nullable
  const long long* pos_ind;
  const float* anno;
  int* count;            // (B*H*W) objects per cell, zero-filled by the caller; nullptr = no gradient wanted
  int* keys;             // (n) workspace: cell index of object i, -1 = not live
  float* og;             // (n, 11) workspace: object i's gradient contributions, map order reg|height|dim|yaw|dir|vel
  long long n;
  int B, H, W, anno_cols;
  float gd_scale, l1_scale;
  // device-resident form (nullable): the task's rows are [rows_dev[0], rows_dev[1]) of pos_ind / anno (n is then the
  // capacity the grid was sized for) and the scales are weight / max(*avg_dev, 1): nothing about the task's size or its
  // normaliser has to pass through the host
  const long long* rows_dev;
  const float* avg_dev;
  double gd_weight, l1_weight;
};
struct CenterDyn {
  long long row0, n;
  float gd_scale, l1_scale;
};
GD_DEV CenterDyn center_dyn(const CenterTask& T) {
  CenterDyn d;
  d.row0 = 0;
  d.n = T.n;
  d.gd_scale = T.gd_scale;
  d.l1_scale = T.l1_scale;
  if (T.rows_dev != nullptr) {
    d.row0 = T.rows_dev[0];
    long long m = T.rows_dev[1] - d.row0;
    m = m < 0 ? 0 : m;
    d.n = m < T.n ? m : T.n;
  }
  if (T.avg_dev != nullptr) {     // the host form divides two Python floats and rounds once: the same here
    const double avg = (double)fmaxf(*T.avg_dev, 1.0f);
    d.gd_scale = (float)(T.gd_weight / avg);
    d.l1_scale = (float)(T.l1_weight / avg);
  }
  return d;
}
struct CenterArgs {
  CenterTask t[CENTER_MAX_TASKS];
  int num_tasks, n_l1, norm_bbox;
  float osf, vs0, vs1, pc0, pc1;
  float alpha, ia2, tau, c0, c1, c2;
  float cw[4];
  float* partials;
  long long pstride;
  long long max_n;       // keys rows are max_n long: entries past a task's own n are set to -1 (not live)
};

template <int LOSS, int FUN, bool FLAG>
__global__ __launch_bounds__(HEAD_T) void head_center_kernel(const CenterArgs a) {
  __shared__ float swave[2][HEAD_T / 64];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ti = blockIdx.y;
  const CenterTask& T = a.t[ti];
  const CenterDyn D = center_dyn(T);
  const long long i = (long long)blockIdx.x * HEAD_T + tid;
  if ((long long)blockIdx.x * HEAD_T >= D.n) {  // uniform: this task has fewer positives than the largest one
    if (T.count != nullptr && i < a.max_n) T.keys[i] = -1;   // the rest of its key row: not live (the sorted finish reads whole rows)
    return;
  }
  float fgd = 0.0f, fl1 = 0.0f;
  bool live = i < D.n;
  int key = -1;
  long long b = 0, x = 0, y = 0;
  const long long row = D.row0 + i;
  if (live) {
    b = T.pos_ind[row * 3];
    x = T.pos_ind[row * 3 + 1];
    y = T.pos_ind[row * 3 + 2];
    if (b < 0 || b >= T.B || x < 0 || x >= T.W || y < 0 || y >= T.H) {
      // an index outside the head map (the reference would fault in its gather): no memory is touched for it and both
      // losses of the task come out NaN, so the error is loud without a host-side range check (= a sync per task)
      live = false;
      fgd = fl1 = __builtin_nanf("");
    }
  }
  if (live) {
    const long long plane = (long long)T.H * T.W;
    const long long off = y * T.W + x;
    // channel k of head h at this cell: maps[h][(b * ch_h + k) * plane + off]
    float enc[7];
    enc[0] = T.maps[0] != nullptr ? T.maps[0][(b * 2 + 0) * plane + off] : 0.5f;  // no 'reg' head: 0.5 (:377-378)
    enc[1] = T.maps[0] != nullptr ? T.maps[0][(b * 2 + 1) * plane + off] : 0.5f;
    enc[2] = T.maps[1][b * plane + off];
#pragma unroll
    for (int k = 0; k < 3; ++k) enc[3 + k] = T.maps[2][(b * 3 + k) * plane + off];
    enc[6] = T.maps[3][b * plane + off];
    float tv[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) tv[k] = T.anno[row * T.anno_cols + k];
    // decode (centerpoint_bbox_yaw_coders.py:18-31, correct_yaw=False)
    float pv[7], jac[7];
    pv[0] = (enc[0] + (float)x) * a.osf * a.vs0 + a.pc0;
    pv[1] = (enc[1] + (float)y) * a.osf * a.vs1 + a.pc1;
    pv[2] = enc[2];
#pragma unroll
    for (int k = 3; k < 6; ++k) {
      pv[k] = a.norm_bbox ? expf(enc[k]) : enc[k];
      jac[k] = a.norm_bbox ? pv[k] : 1.0f;
    }
    pv[6] = enc[6];
    jac[0] = a.osf * a.vs0; jac[1] = a.osf * a.vs1; jac[2] = 1.0f; jac[6] = 1.0f;
    const float c[3] = {a.c0, a.c1, a.c2};
    float g1[7], g2[7];
    const float L = pair_loss<LOSS, FUN, FLAG, false>(pv, tv, c, a.alpha, a.ia2, a.tau, D.gd_scale, g1, g2);
    fgd = D.gd_scale * L;
    // L1 on the remaining channels: dir (sin, cos) and velocity
    float sy, cy;
    sincos_f(tv[6], sy, cy);
    float gl1[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k < a.n_l1) {
        const float p = k < 2 ? T.maps[4][(b * 2 + k) * plane + off] : T.maps[5][(b * 2 + (k - 2)) * plane + off];
        const float t = k == 0 ? sy : (k == 1 ? cy : T.anno[row * T.anno_cols + 7 + (k - 2)]);
        const float d = p - t;
        fl1 += fabsf(d) * a.cw[k];
        gl1[k] = (d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f)) * a.cw[k] * D.l1_scale;  // torch abs'(0) = 0
      }
    }
    fl1 *= D.l1_scale;
    // stage: GD gradient -> reg / height / dim / yaw slots, L1 gradient -> dir / vel slots
    if (T.count != nullptr) {
      float* o = T.og + i * 11;
#pragma unroll
      for (int k = 0; k < 7; ++k) o[k] = g1[k] * jac[k];
#pragma unroll
      for (int k = 0; k < 4; ++k) o[7 + k] = gl1[k];
      key = (int)(b * plane + off);
      atomicAdd(&T.count[key], 1);
    }
  }
  if (T.count != nullptr && i < a.max_n) T.keys[i] = key;   // -1 for rows that are not live and past the task's n
  const float w0 = wave_sum(fl1), w1 = wave_sum(fgd);
  if (lane == 0) {
    swave[0][wave] = w0;
    swave[1][wave] = w1;
  }
  __syncthreads();
  if (tid < 2)
    a.partials[((long long)ti * 2 + tid) * a.pstride + blockIdx.x] =
        (swave[tid][0] + swave[tid][1]) + (swave[tid][2] + swave[tid][3]);
}

// Second step of the CenterGDHead launch pair.  grid = (pstride, tasks), same geometry as head_center_kernel.
//  (1) gradient: thread i owns object i.  count[cell] == 1: its 11 staged values go straight to the maps.  Shared cells:
//      one such lane at a time, the wave scans the task's keys in ascending object order (64 per step, ballot); the lane
//      is the cell's OWNER iff the first match is itself, and then lanes 0..10 add the matching objects' staged values
//      in that order and write the cell.  Sums are in ascending object index whatever the launch geometry.
//  (2) block (0, task): fixed-order fp64 sum of the task's loss partials -> losses[task * 2 + {l1, gd}].
GD_DEV float* center_slot(const CenterTask& T, int k, long long b, long long off, long long plane, int n_l1) {
  // slot k of the staged row -> address in the gradient maps (nullptr: that map wants no gradient)
  if (k < 2) return T.grads[0] != nullptr ? T.grads[0] + (b * 2 + k) * plane + off : nullptr;
  if (k == 2) return T.grads[1] != nullptr ? T.grads[1] + b * plane + off : nullptr;
  if (k < 6) return T.grads[2] != nullptr ? T.grads[2] + (b * 3 + (k - 3)) * plane + off : nullptr;
  if (k == 6) return T.grads[3] != nullptr ? T.grads[3] + b * plane + off : nullptr;
  if (k < 9) return (T.grads[4] != nullptr && n_l1 >= 2) ? T.grads[4] + (b * 2 + (k - 7)) * plane + off : nullptr;
  return (T.grads[5] != nullptr && n_l1 > 2) ? T.grads[5] + (b * 2 + (k - 9)) * plane + off : nullptr;
}

// block (0, task): fixed-order fp64 sum of the task's loss partials -> losses[task * 2 + {l1, gd}]
GD_DEV void center_loss_sums(const CenterArgs& a, int ti, long long n, double* sd, float* __restrict__ losses) {
  const int tid = threadIdx.x;
  const long long nb = (n + HEAD_T - 1) / HEAD_T;
  for (int term = 0; term < 2; ++term) {
    const float* p = a.partials + ((long long)ti * 2 + term) * a.pstride;
    double acc = 0.0;
    for (long long k = tid; k < nb; k += HEAD_T) acc += (double)p[k];
    __syncthreads();
    sd[tid] = acc;
    __syncthreads();
#pragma unroll
    for (int s2 = HEAD_T / 2; s2 > 0; s2 >>= 1) {
      if (tid < s2) sd[tid] += sd[tid + s2];
      __syncthreads();
    }
    if (tid == 0) losses[ti * 2 + term] = (float)sd[0];
  }
}

__global__ __launch_bounds__(HEAD_T) void center_accum_kernel(const CenterArgs a, float* __restrict__ losses) {
  __shared__ double sd[HEAD_T];
  const int tid = threadIdx.x, lane = tid & 63;
  const int ti = blockIdx.y;
  const CenterTask& T = a.t[ti];
  const long long Tn = center_dyn(T).n;
  const long long plane = (long long)T.H * T.W;
  if (T.count != nullptr && (long long)blockIdx.x * HEAD_T < Tn) {  // uniform
    const long long i = (long long)blockIdx.x * HEAD_T + tid;
    const int key = i < Tn ? T.keys[i] : -1;
    const int c = key >= 0 ? T.count[key] : 0;
    if (c == 1) {
      const long long b = key / plane, off = key - b * plane;
#pragma unroll
      for (int k = 0; k < 11; ++k) {
        float* dst = center_slot(T, k, b, off, plane, a.n_l1);
        if (dst != nullptr) *dst = T.og[i * 11 + k];
      }
    }
    unsigned long long dup = __builtin_amdgcn_ballot_w64(c > 1);
    while (dup != 0ull) {                                             // wave-uniform
      const int L = __builtin_ctzll(dup);
      dup &= dup - 1;
      const int kL = __builtin_amdgcn_readlane(key, L);
      const long long iL = i - lane + L;
      float acc = 0.0f;
      bool owner = true, first = true;
      for (long long j0 = 0; j0 < Tn && owner; j0 += 64) {
        const long long j = j0 + lane;
        unsigned long long m = __builtin_amdgcn_ballot_w64(j < Tn && T.keys[j] == kL);
        while (m != 0ull) {
          const long long jj = j0 + __builtin_ctzll(m);
          m &= m - 1;
          if (first) {
            first = false;
            if (jj != iL) {                                           // an earlier object owns this cell
              owner = false;
              break;
            }
          }
          if (lane < 11) acc += T.og[jj * 11 + lane];
        }
      }
      if (owner && lane < 11) {
        const long long b = kL / plane, off = kL - b * plane;
        float* dst = center_slot(T, lane, b, off, plane, a.n_l1);
        if (dst != nullptr) *dst = acc;
      }
    }
  }
  if (blockIdx.x != 0) return;
  center_loss_sums(a, ti, Tn, sd, losses);
}

// The same second step when the caller hands in, per task, the positions of the key row sorted by key (STABLE: objects of
// one cell stay in ascending index; order is (tasks, max_n) int64 — torch.sort(keys, dim=1, stable=True) on the rows that
// head_center_kernel left).  Thread s owns sorted position s: the first entry of a run of equal keys adds the run's staged
// rows in that order and writes the cell.  O(n) whatever the number of objects per cell: the scan form above costs
// O(shared-cell objects x n / 64) wave steps, fine for a detection batch (n = 4000, a few shared cells) and quadratic when
// tens of thousands of objects fall into few cells.
__global__ __launch_bounds__(HEAD_T) void center_accum_sorted_kernel(const CenterArgs a, float* __restrict__ losses,
                                                                     const long long* __restrict__ order) {
  __shared__ double sd[HEAD_T];
  const int tid = threadIdx.x;
  const int ti = blockIdx.y;
  const CenterTask& T = a.t[ti];
  const long long plane = (long long)T.H * T.W;
  const long long s = (long long)blockIdx.x * HEAD_T + tid;
  if (T.count != nullptr && s < a.max_n) {
    const long long* ord = order + (long long)ti * a.max_n;
    const long long i = ord[s];
    const int key = (i >= 0 && i < a.max_n) ? T.keys[i] : -1;
    const long long ip = s > 0 ? ord[s - 1] : -1;
    const int prev = (ip >= 0 && ip < a.max_n) ? T.keys[ip] : -2;   // (a malformed order must not read outside the row)
    if (key >= 0 && key != prev) {  // run start: this thread owns the cell
      float acc[11];
#pragma unroll
      for (int k = 0; k < 11; ++k) acc[k] = T.og[i * 11 + k];
      for (long long e = s + 1; e < a.max_n; ++e) {
        const long long j = ord[e];
        if (j < 0 || j >= a.max_n || T.keys[j] != key) break;
#pragma unroll
        for (int k = 0; k < 11; ++k) acc[k] += T.og[j * 11 + k];
      }
      const long long b = key / plane, off = key - b * plane;
#pragma unroll
      for (int k = 0; k < 11; ++k) {
        float* dst = center_slot(T, k, b, off, plane, a.n_l1);
        if (dst != nullptr) *dst = acc[k];
      }
    }
  }
  if (blockIdx.x != 0) return;
  center_loss_sums(a, ti, center_dyn(T).n, sd, losses);
}

// backward of the same call when the upstream gradient is not all ones: grads of task t are scaled by
// gout[t*2 + 1] (reg / height / dim / yaw: the GD term) or gout[t*2] (dir / vel: the L1 term); a (task, map) slice whose
// factor is exactly 1 exits after one scalar load.  blockIdx.y = task * 6 + map.
__global__ __launch_bounds__(256) void center_scale_kernel(const CenterArgs a, const float* __restrict__ gout) {
  const int ti = blockIdx.y / 6, m = blockIdx.y - ti * 6;
  const CenterTask& T = a.t[ti];
  float* gmap = T.grads[m];
  if (gmap == nullptr) return;
  const float gs = gout[ti * 2 + (m < 4 ? 1 : 0)];
  if (gs == 1.0f) return;
  const int ch = (m == 0 || m >= 4) ? 2 : (m == 2 ? 3 : 1);
  const long long nflt = (long long)T.B * ch * T.H * T.W;
  for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < nflt; k += (long long)gridDim.x * 256) gmap[k] *= gs;
}

}  // namespace gd3d

using namespace gd3d;

extern "C" {

static size_t center_partial_bytes(int32_t num_tasks, int64_t max_n) {
  const int64_t nb = (max_n + HEAD_T - 1) / HEAD_T;
  return (size_t)((2 * (int64_t)num_tasks * nb * 4 + 15) / 16 * 16);
}

static int center_fill(const gd3d_params* p, const gd3d_prologue* coder, const gd3d_center_task* tasks, int32_t num_tasks,
                       const float* code_weights, int32_t n_l1, void* workspace, CenterArgs& a, long long& max_n) {
  if (p == nullptr || coder == nullptr || tasks == nullptr || num_tasks <= 0 || num_tasks > CENTER_MAX_TASKS)
    return GD3D_E_BADARG;
  if (n_l1 != 0 && n_l1 != 2 && n_l1 != 4) return GD3D_E_BADARG;
  if (n_l1 > 0 && code_weights == nullptr) return GD3D_E_BADARG;
  a.num_tasks = num_tasks;
  a.n_l1 = n_l1;
  a.norm_bbox = coder->norm_bbox;
  a.osf = coder->out_size_factor;
  a.vs0 = coder->voxel_size[0];
  a.vs1 = coder->voxel_size[1];
  a.pc0 = coder->pc_range[0];
  a.pc1 = coder->pc_range[1];
  a.alpha = p->alpha;
  a.ia2 = gd3d_inv_alpha2(p->alpha);
  a.tau = p->tau;
  a.c0 = p->center_offset[0];
  a.c1 = p->center_offset[1];
  a.c2 = p->center_offset[2];
  for (int k = 0; k < 4; ++k) a.cw[k] = k < n_l1 ? code_weights[k] : 0.0f;
  max_n = 0;
  for (int t = 0; t < num_tasks; ++t) {
    const gd3d_center_task& s = tasks[t];
    if (s.n < 0 || s.B <= 0 || s.H <= 0 || s.W <= 0) return GD3D_E_BADARG;
    if (s.n > 0) {
      if (s.pos_ind == nullptr || s.anno == nullptr || s.anno_cols < 7 + (n_l1 > 2 ? 2 : 0)) return GD3D_E_BADARG;
      for (int m = 1; m <= 3; ++m)
        if (s.maps[m] == nullptr) return GD3D_E_BADARG;
      if (n_l1 >= 2 && s.maps[4] == nullptr) return GD3D_E_BADARG;
      if (n_l1 == 4 && s.maps[5] == nullptr) return GD3D_E_BADARG;
    }
    CenterTask& d = a.t[t];
    for (int m = 0; m < 6; ++m) {
      d.maps[m] = s.maps[m];
      d.grads[m] = s.grads[m];
    }
    d.pos_ind = (const long long*)s.pos_ind;
    d.anno = s.anno;
    bool wants = false;
    for (int m = 0; m < 6; ++m) wants |= s.grads[m] != nullptr;
    if (wants && s.cell_count == nullptr) return GD3D_E_BADARG;
    d.count = wants ? (int*)s.cell_count : nullptr;
    d.keys = nullptr;
    d.og = nullptr;
    d.n = s.n;
    d.B = s.B;
    d.H = s.H;
    d.W = s.W;
    d.anno_cols = s.anno_cols;
    d.gd_scale = s.gd_scale;
    d.l1_scale = s.l1_scale;
    d.rows_dev = (const long long*)s.rows_dev;
    d.avg_dev = s.avg_dev;
    d.gd_weight = s.gd_weight;
    d.l1_weight = s.l1_weight;
    if (s.n > max_n) max_n = s.n;
  }
  a.partials = (float*)workspace;
  a.pstride = (max_n + HEAD_T - 1) / HEAD_T;
  a.max_n = max_n;
  // workspace: partials (2 * tasks * pstride floats, padded to 16 B) | per task: keys (max_n int32) | og (max_n * 11 fp32)
  if (workspace != nullptr) {
    char* base = (char*)workspace + center_partial_bytes(num_tasks, max_n);
    for (int t = 0; t < num_tasks; ++t) {
      a.t[t].keys = (int*)(base + (size_t)t * 48 * (size_t)max_n);
      a.t[t].og = (float*)(base + (size_t)t * 48 * (size_t)max_n + 4 * (size_t)max_n);
    }
  }
  return 0;
}

size_t gd3d_center_head_workspace_bytes(int32_t num_tasks, int64_t max_n) {
  if (num_tasks <= 0 || max_n <= 0) return 16;
  return center_partial_bytes(num_tasks, max_n) + (size_t)num_tasks * 48 * (size_t)max_n;
}

static int center_stage(const gd3d_params* p, const gd3d_prologue* coder, const gd3d_center_task* tasks, int32_t num_tasks,
                        const float* code_weights, int32_t n_l1, float* losses, void* workspace, void* stream, CenterArgs& a,
                        long long& max_n, bool launch) {
  const int rc = center_fill(p, coder, tasks, num_tasks, code_weights, n_l1, workspace, a, max_n);
  if (rc != 0) return rc;
  if (losses == nullptr) return GD3D_E_BADARG;
  if (check_instance(p->loss_type, p->fun) != 0) return GD3D_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  if (max_n == 0) return launch ? fill_words(losses, sizeof(float) * 2 * (size_t)num_tasks, 0u, s) : 0;
  if (workspace == nullptr) return GD3D_E_BADARG;
  if (a.pstride > 0x7fffffffLL) return GD3D_E_TOOLARGE;
  if (!launch) return 0;
  const dim3 grid((unsigned)a.pstride, (unsigned)num_tasks);
  with_instance(p->loss_type, p->fun, p->flag != 0, [&](auto inst) {
    using I = decltype(inst);
    hipLaunchKernelGGL((head_center_kernel<I::loss, I::fun, I::flag>), grid, dim3(HEAD_T), 0, s, a);
  });
  return (int)hipGetLastError();
}

static int center_finish(const CenterArgs& a, int32_t num_tasks, long long max_n, float* losses, const int64_t* order,
                         void* stream) {
  if (max_n == 0) return 0;   // the stage call already zeroed the losses
  const dim3 grid((unsigned)a.pstride, (unsigned)num_tasks);
  // second step: gradient accumulation (deterministic) + the loss sums.  Tasks without positives: their partial slices
  // are never written; the sum reads nb = 0 entries -> 0
  if (order != nullptr)
    hipLaunchKernelGGL(center_accum_sorted_kernel, grid, dim3(HEAD_T), 0, (hipStream_t)stream, a, losses, (const long long*)order);
  else
    hipLaunchKernelGGL(center_accum_kernel, grid, dim3(HEAD_T), 0, (hipStream_t)stream, a, losses);
  return (int)hipGetLastError();
}

int gd3d_center_head_loss(const gd3d_params* p, const gd3d_prologue* coder, const gd3d_center_task* tasks, int32_t num_tasks,
                          const float* code_weights, int32_t n_l1, float* losses, void* workspace, void* stream) {
  CenterArgs a;
  long long max_n = 0;
  const int rc = center_stage(p, coder, tasks, num_tasks, code_weights, n_l1, losses, workspace, stream, a, max_n, true);
  if (rc != 0) return rc;
  return center_finish(a, num_tasks, max_n, losses, nullptr, stream);
}

int gd3d_center_head_stage(const gd3d_params* p, const gd3d_prologue* coder, const gd3d_center_task* tasks, int32_t num_tasks,
                           const float* code_weights, int32_t n_l1, float* losses, void* workspace, void* stream) {
  CenterArgs a;
  long long max_n = 0;
  return center_stage(p, coder, tasks, num_tasks, code_weights, n_l1, losses, workspace, stream, a, max_n, true);
}

int gd3d_center_head_finish(const gd3d_params* p, const gd3d_prologue* coder, const gd3d_center_task* tasks, int32_t num_tasks,
                            const float* code_weights, int32_t n_l1, float* losses, void* workspace, const int64_t* order,
                            void* stream) {
  CenterArgs a;
  long long max_n = 0;
  const int rc = center_stage(p, coder, tasks, num_tasks, code_weights, n_l1, losses, workspace, stream, a, max_n, false);
  if (rc != 0) return rc;
  return center_finish(a, num_tasks, max_n, losses, order, stream);
}

int gd3d_center_head_keys(int32_t num_tasks, int64_t max_n, int64_t* byte_offset, int64_t* byte_stride) {
  if (num_tasks <= 0 || max_n < 0 || byte_offset == nullptr || byte_stride == nullptr) return GD3D_E_BADARG;
  *byte_offset = (int64_t)center_partial_bytes(num_tasks, max_n);
  *byte_stride = 48 * max_n;
  return 0;
}

int gd3d_center_head_scale(const gd3d_center_task* tasks, int32_t num_tasks, const float* grad_losses, void* stream) {
  if (tasks == nullptr || num_tasks <= 0 || num_tasks > CENTER_MAX_TASKS || grad_losses == nullptr) return GD3D_E_BADARG;
  CenterArgs a;
  a.num_tasks = num_tasks;
  for (int t = 0; t < num_tasks; ++t) {
    for (int m = 0; m < 6; ++m) {
      a.t[t].maps[m] = nullptr;
      a.t[t].grads[m] = tasks[t].grads[m];
    }
    if (tasks[t].B <= 0 || tasks[t].H <= 0 || tasks[t].W <= 0) return GD3D_E_BADARG;
    a.t[t].B = tasks[t].B;
    a.t[t].H = tasks[t].H;
    a.t[t].W = tasks[t].W;
    a.t[t].n = 0;
    a.t[t].count = nullptr;
    a.t[t].keys = nullptr;
    a.t[t].og = nullptr;
  }
  hipLaunchKernelGGL(center_scale_kernel, dim3(64, 6 * (unsigned)num_tasks), dim3(256), 0, (hipStream_t)stream, a,
                     grad_losses);
  return (int)hipGetLastError();
}

}  // extern "C"
