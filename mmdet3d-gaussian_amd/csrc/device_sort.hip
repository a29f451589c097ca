// device_sort.hip — the one translation unit that includes rocPRIM (csrc/device_sort.h): the device radix sort of (int64 key, int32
// value) pairs and of int64 keys, and the int32 scans, for gfx950.  A kernel of the library lives in one code object once: the
// voxel index, hard voxelization and the sparse conv index build all run these instances.  Integer code only: no flag of its own.
#include "device_sort.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

namespace gd3d {

int key_bits(long long sentinel) {
  int bits = 1;
  while (bits < 63 && (sentinel >> bits) != 0) ++bits;
  return bits;
}

hipError_t sort_pairs_temp_bytes(size_t n, size_t& bytes) {
  bytes = 0;
  return rocprim::radix_sort_pairs(nullptr, bytes, (const long long*)nullptr, (long long*)nullptr, (const int*)nullptr, (int*)nullptr, n, 0,
                                   64, (hipStream_t)0);
}

hipError_t sort_pairs(void* temp, size_t temp_bytes, const long long* keys_in, long long* keys_out, const int* vals_in, int* vals_out,
                      size_t n, unsigned end_bit, hipStream_t s) {
  return rocprim::radix_sort_pairs(temp, temp_bytes, keys_in, keys_out, vals_in, vals_out, n, 0, end_bit, s);
}

hipError_t sort_keys_temp_bytes(size_t n, size_t& bytes) {
  bytes = 0;
  return rocprim::radix_sort_keys(nullptr, bytes, (const long long*)nullptr, (long long*)nullptr, n, 0, 64, (hipStream_t)0);
}

hipError_t sort_keys(void* temp, size_t temp_bytes, const long long* keys_in, long long* keys_out, size_t n, unsigned end_bit,
                     hipStream_t s) {
  return rocprim::radix_sort_keys(temp, temp_bytes, keys_in, keys_out, n, 0, end_bit, s);
}

hipError_t inclusive_sum_temp_bytes(size_t n, size_t& bytes) {
  bytes = 0;
  return rocprim::inclusive_scan(nullptr, bytes, (const int*)nullptr, (int*)nullptr, n, rocprim::plus<int>(), (hipStream_t)0);
}

hipError_t inclusive_sum(void* temp, size_t temp_bytes, const int* in, int* out, size_t n, hipStream_t s) {
  return rocprim::inclusive_scan(temp, temp_bytes, in, out, n, rocprim::plus<int>(), s);
}

hipError_t inclusive_max_temp_bytes(size_t n, size_t& bytes) {
  bytes = 0;
  return rocprim::inclusive_scan(nullptr, bytes, (const int*)nullptr, (int*)nullptr, n, rocprim::maximum<int>(), (hipStream_t)0);
}

hipError_t inclusive_max(void* temp, size_t temp_bytes, const int* in, int* out, size_t n, hipStream_t s) {
  return rocprim::inclusive_scan(temp, temp_bytes, in, out, n, rocprim::maximum<int>(), s);
}

hipError_t exclusive_sum_temp_bytes(size_t n, size_t& bytes) {
  bytes = 0;
  return rocprim::exclusive_scan(nullptr, bytes, (const int*)nullptr, (int*)nullptr, 0, n, rocprim::plus<int>(), (hipStream_t)0);
}

hipError_t exclusive_sum(void* temp, size_t temp_bytes, const int* in, int* out, size_t n, hipStream_t s) {
  return rocprim::exclusive_scan(temp, temp_bytes, in, out, 0, n, rocprim::plus<int>(), s);
}

}  // namespace gd3d
