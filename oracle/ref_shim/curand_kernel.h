// Stub (ours).  voxel_query_gpu.cu's random replacement is commented out in the reference; only the state and its init call remain.
#ifndef GD3D_ORACLE_REF_SHIM_CURAND_H
#define GD3D_ORACLE_REF_SHIM_CURAND_H
#include "ref_shim.h"
struct curandState {};
__device__ inline void curand_init(unsigned long long, unsigned long long, unsigned long long, curandState *) {}
#endif
