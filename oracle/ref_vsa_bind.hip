// ref_vsa_bind.hip — TEST INFRASTRUCTURE.  C entries (ours) around the REFERENCE's own voxel-set-abstraction kernels, which are
// compiled from where they lie (-I$(REF)/mmdet3d_gaussian/ops/vsa/src):
//   ball_query.cu       ball_query_kernel :12-74 and its host wrapper `ball_query` :76-106
//   group_points.cu     group_points_kernel_stack, group_points_grad_kernel_stack and the wrappers `group_points`, `group_points_grad`
//   sampling.cu         furthest_point_sampling_kernel<block> and `furthest_point_sampling` (block = 2^floor(log2 n), at most 1024)
//   voxel_query_gpu.cu  voxel_query_kernel_stack and `voxel_query_kernel_launcher_stack` (raw pointers already; voxel_query.cpp, which
//                       needs THCState, is not compiled)
// oracle/ref_shim/ (ours) stands in for the CUDA and torch headers those files include.  Compiled with -ffp-contract=off: the
// arithmetic is then what the source states, one rounding per operation (oracle/README.md).  Output: oracle/_ref/ref_vsa.so
// (git-ignored).  The kernels check no bounds and the wrappers exit(-1) on a launch error: oracle/ref_kernels.py validates every
// argument on the host before it calls in here, and is the only caller.
#include "ball_query.cu"
#include "group_points.cu"
#include "sampling.cu"
#include "voxel_query_gpu.cu"

using at::Tensor;

extern "C" {

int ref_vsa_ball_query(float radius, int nsample, int B, int M, const float *new_xyz, const int *new_xyz_batch_cnt, const float *xyz,
                       const int *xyz_batch_cnt, int *idx, void *stream) {
  ref_shim_stream() = static_cast<hipStream_t>(stream);
  Tensor idx_t(idx, M, nsample);   // the wrapper reads B off xyz_batch_cnt and M off new_xyz, and no size of xyz
  return ball_query(radius, nsample, Tensor(new_xyz, M, 3), Tensor(new_xyz_batch_cnt, B, 1), Tensor(xyz, 0, 3),
                    Tensor(xyz_batch_cnt, B, 1), idx_t);
}

int ref_vsa_group_points(const float *features, const int *features_batch_cnt, const int *idx, const int *idx_batch_cnt, int B, int N,
                         int C, int M, int nsample, float *out, void *stream) {
  ref_shim_stream() = static_cast<hipStream_t>(stream);
  Tensor out_t(out, M, C);
  return group_points(Tensor(features, N, C), Tensor(features_batch_cnt, B, 1), Tensor(idx, M, nsample), Tensor(idx_batch_cnt, B, 1),
                      out_t);
}

int ref_vsa_group_points_grad(const float *grad_out, const int *idx, const int *idx_batch_cnt, const int *features_batch_cnt, int B,
                              int N, int C, int M, int nsample, float *grad_features, void *stream) {
  ref_shim_stream() = static_cast<hipStream_t>(stream);
  Tensor grad_t(grad_features, N, C);
  return group_points_grad(Tensor(grad_out, M, C), Tensor(idx, M, nsample), Tensor(idx_batch_cnt, B, 1),
                           Tensor(features_batch_cnt, B, 1), grad_t);
}

int ref_vsa_furthest_point_sampling(const float *points, float *temp, int *idx, int b, int n, int m, void *stream) {
  ref_shim_stream() = static_cast<hipStream_t>(stream);
  Tensor temp_t(temp, b, n), idx_t(idx, b, m);
  return furthest_point_sampling(Tensor(points, b, n), temp_t, idx_t);
}

// The block size `furthest_point_sampling` will launch for n points (the reference's own opt_n_threads).
int ref_vsa_fps_block(int n) { return opt_n_threads(n); }

// Launches on the null stream, as the reference's launcher does.
int ref_vsa_voxel_query(int M, int R1, int R2, int R3, int nsample, float radius, int z_range, int y_range, int x_range,
                        const float *new_xyz, const float *xyz, const int *new_coords, const int *point_indices, int *idx) {
  voxel_query_kernel_launcher_stack(M, R1, R2, R3, nsample, radius, z_range, y_range, x_range, new_xyz, xyz, new_coords, point_indices,
                                    idx);
  return 1;
}

}  // extern "C"
