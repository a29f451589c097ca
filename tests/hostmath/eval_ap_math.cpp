// TEST INFRASTRUCTURE (tests/test_cpu_eval_ap.py): the shared arithmetic of csrc/eval_ap_common.h compiled for the host, one array call
// per function, so that the test can hold it to Python's integers — in particular limbs_to_double on UN-normalised limb sums, which
// only the device's finish kernel passes it (the `_cpu` twin normalises first).
//   c++ -O1 -std=c++17 -ffp-contract=off -shared -fPIC tests/hostmath/eval_ap_math.cpp -o libevalapmath.so
#define GD3D_HOST_TWIN 1
#include "../../mmdet3d-gaussian_amd/csrc/eval_ap_common.h"

using namespace eval_ap;

extern "C" {

// e (n) -> limbs (n, 4)
void hostmath_limbs_of(const double* e, long n, uint32_t* limbs) {
  for (long i = 0; i < n; ++i) {
    const Limbs q = limbs_of(e[i]);
    for (int k = 0; k < 4; ++k) limbs[i * 4 + k] = q.l[k];
  }
}

// limb sums (n, 4), each below 2^53 -> the rounded totals (n)
void hostmath_limbs_to_double(const uint64_t* limbs, long n, double* out) {
  for (long i = 0; i < n; ++i) out[i] = limbs_to_double(limbs[i * 4], limbs[i * 4 + 1], limbs[i * 4 + 2], limbs[i * 4 + 3]);
}

void hostmath_score_key(const float* score, long n, uint32_t* key) {
  for (long i = 0; i < n; ++i) key[i] = score_key(score[i]);
}

void hostmath_record_key(const int32_t* group, const float* score, long n, int32_t K, uint64_t* key) {
  for (long i = 0; i < n; ++i) key[i] = record_key(group[i], score[i], K);
}

}  // extern "C"
