// device_sort.h — the library primitives of the indexed ops (csrc/voxel_index.hip, hard_voxel.hip, sparse_conv.hip): rocPRIM's device
// radix sort and scans, instantiated in exactly one translation unit, csrc/device_sort.hip; every other unit reaches them through
// these plain functions and includes no rocPRIM header.  Not exported (gd3d.map).
// Every primitive is a pair: *_temp_bytes, the scratch `n` items need (it launches nothing), and the run on stream `s`, which is
// handed that scratch.  Keys are sorted ascending over bits [0, end_bit), stable.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace gd3d {

int key_bits(long long sentinel);   // the bits of the largest key: the end_bit of a sort whose keys are <= sentinel

hipError_t sort_pairs_temp_bytes(size_t n, size_t& bytes);
hipError_t sort_pairs(void* temp, size_t temp_bytes, const long long* keys_in, long long* keys_out, const int* vals_in, int* vals_out,
                      size_t n, unsigned end_bit, hipStream_t s);

hipError_t sort_keys_temp_bytes(size_t n, size_t& bytes);
hipError_t sort_keys(void* temp, size_t temp_bytes, const long long* keys_in, long long* keys_out, size_t n, unsigned end_bit,
                     hipStream_t s);

hipError_t inclusive_sum_temp_bytes(size_t n, size_t& bytes);
hipError_t inclusive_sum(void* temp, size_t temp_bytes, const int* in, int* out, size_t n, hipStream_t s);

hipError_t inclusive_max_temp_bytes(size_t n, size_t& bytes);
hipError_t inclusive_max(void* temp, size_t temp_bytes, const int* in, int* out, size_t n, hipStream_t s);

hipError_t exclusive_sum_temp_bytes(size_t n, size_t& bytes);   // from 0
hipError_t exclusive_sum(void* temp, size_t temp_bytes, const int* in, int* out, size_t n, hipStream_t s);

}  // namespace gd3d
