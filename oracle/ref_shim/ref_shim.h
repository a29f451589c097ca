// ref_shim.h — TEST INFRASTRUCTURE.  The one stub behind every header the reference's ops/vsa/src/*.cu include
// (cuda.h, cuda_runtime_api.h, THC/THC.h, torch/serialize/tensor.h, ATen/cuda/CUDAContext.h): just enough of the CUDA runtime
// names and of at::Tensor for those files to compile with hipcc, unchanged and from where they lie, WITHOUT torch.
// Nothing here restates a reference kernel.  oracle/ref_vsa_bind.hip is the only translation unit that uses it.
#ifndef GD3D_ORACLE_REF_SHIM_H
#define GD3D_ORACLE_REF_SHIM_H

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

typedef hipError_t cudaError_t;
#define cudaSuccess hipSuccess
#define cudaGetLastError hipGetLastError
#define cudaGetErrorString hipGetErrorString

// The stream the reference's host wrappers launch on (`at::cuda::getCurrentCUDAStream()`); the binding sets it per call.
inline hipStream_t &ref_shim_stream() {
  static hipStream_t stream = nullptr;
  return stream;
}

namespace at {

struct Device {
  bool is_cuda() const { return true; }   // the driver (oracle/ref_kernels.py) checks the device before it builds a Tensor
};

// A raw device pointer and two sizes: what the reference's wrappers read of a tensor.  Contiguity, dtype and device are the
// driver's to assert; this class cannot see them.
struct Tensor {
  void *ptr;
  int64_t sizes[2];
  Tensor(const void *p, int64_t s0, int64_t s1) : ptr(const_cast<void *>(p)), sizes{s0, s1} {}
  template <typename T> T *data_ptr() const { return static_cast<T *>(ptr); }
  template <typename T> T *data() const { return static_cast<T *>(ptr); }
  int64_t size(int i) const { return sizes[i]; }
  Device device() const { return Device(); }
  bool is_contiguous() const { return true; }
};

namespace cuda {
inline hipStream_t getCurrentCUDAStream() { return ref_shim_stream(); }
}  // namespace cuda

}  // namespace at

#endif
