// gd3d_instances.h — which pair_loss<LOSS, FUN, FLAG, ·> instances (csrc/gd3d_device.h) exist, and how the runtime
// gd3d_params select one.  Every launcher (fused kernel, anchor head, CenterPoint head), the `_cpu` twin and the host-math
// test library go through the two functions below; nothing else lists loss types or funs.
//
// Plain C++17, no HIP: device and host translation units include it alike.
//
// NOT part of the instance: GT (gradient with respect to the target) and the fused kernel's PLAIN variant are properties
// of one call site and stay two-way branches there.
#pragma once
#include "../../include/gd3d.h"

namespace gd3d {

// One compiled instance, handed to with_instance()'s callable as a value: `[&](auto inst) { using I = decltype(inst); ... }`.
template <int LOSS, int FUN, bool FLAG>
struct Instance {
  static constexpr int loss = LOSS;
  static constexpr int fun = FUN;
  static constexpr bool flag = FLAG;
};

// The validity rule: loss type in range and fun in the loss type's domain, as GDLoss.__init__ asserts
// (gaussian_distance_loss.py:267-270).  kfiou3d: none / expm1 / nlog; every other loss: none / log1p.
inline int check_instance(int loss_type, int fun) {
  if (loss_type < 0 || loss_type >= GD3D_NUM_LOSS_TYPES) return GD3D_E_BADARG;
  const bool ok = loss_type == GD3D_KFIOU3D ? (fun == GD3D_FUN_NONE || fun == GD3D_FUN_EXPM1 || fun == GD3D_FUN_NLOG)
                                            : (fun == GD3D_FUN_NONE || fun == GD3D_FUN_LOG1P);
  return ok ? 0 : GD3D_E_BADARG;
}

// The fun and flag columns of one loss type.  kfiou3d_loss accepts `sqrt` and ignores it (ref :228): its flag is pinned
// to false here, at compile time, so that its flag-on instances are never named and never compiled.
template <int LOSS, class F>
decltype(auto) with_fun_flag(int fun, bool flag, F&& f) {
  if constexpr (LOSS == GD3D_KFIOU3D) {
    switch (fun) {
      case GD3D_FUN_EXPM1: return f(Instance<LOSS, GD3D_FUN_EXPM1, false>{});
      case GD3D_FUN_NLOG: return f(Instance<LOSS, GD3D_FUN_NLOG, false>{});
      default: return f(Instance<LOSS, GD3D_FUN_NONE, false>{});
    }
  } else if (fun == GD3D_FUN_LOG1P) {
    return flag ? f(Instance<LOSS, GD3D_FUN_LOG1P, true>{}) : f(Instance<LOSS, GD3D_FUN_LOG1P, false>{});
  } else {
    return flag ? f(Instance<LOSS, GD3D_FUN_NONE, true>{}) : f(Instance<LOSS, GD3D_FUN_NONE, false>{});
  }
}

// The table: calls f(Instance<LOSS, FUN, FLAG>{}) for the instance that (loss_type, fun, flag) select and returns what it
// returns (the same type for every instance).  27 instances: 6 loss types x {none, log1p} x {flag off, on} + kfiou3d x
// {none, expm1, nlog}.  The arguments must have passed check_instance().
template <class F>
decltype(auto) with_instance(int loss_type, int fun, bool flag, F&& f) {
  switch (loss_type) {
    case GD3D_GWD3D: return with_fun_flag<GD3D_GWD3D>(fun, flag, f);
    case GD3D_KLD3D: return with_fun_flag<GD3D_KLD3D>(fun, flag, f);
    case GD3D_BD3D: return with_fun_flag<GD3D_BD3D>(fun, flag, f);
    case GD3D_JD3D: return with_fun_flag<GD3D_JD3D>(fun, flag, f);
    case GD3D_KLD3D_SYMMAX: return with_fun_flag<GD3D_KLD3D_SYMMAX>(fun, flag, f);
    case GD3D_KLD3D_SYMMIN: return with_fun_flag<GD3D_KLD3D_SYMMIN>(fun, flag, f);
    default: return with_fun_flag<GD3D_KFIOU3D>(fun, flag, f);
  }
}

// The instances the multi-loss fused kernel (gd3d_loss.hip: fused_multi_kernel) is compiled for: the first MULTI_LOSSES loss
// types, each with MULTI_FUN and MULTI_FLAG — what a training step runs side by side on one target.  The kernel exists for
// every non-decreasing tuple of 2 or 3 of them (16 kernels); the launcher sorts a call's losses into that order.
constexpr int MULTI_LOSSES = 3;   // gwd3d, kld3d, bd3d
constexpr int MULTI_FUN = GD3D_FUN_LOG1P;
constexpr bool MULTI_FLAG = true;
constexpr int MULTI_MAX = 3;      // losses per launch

inline bool multi_marked(int loss_type, int fun, bool flag) {
  return loss_type >= 0 && loss_type < MULTI_LOSSES && fun == MULTI_FUN && flag == MULTI_FLAG;
}

// Calls f(std::integral_constant-like tags) for the sorted tuple (l0 <= l1 [<= l2]); count 2 passes l2 = -1.
template <int L0, int L1, int L2>
struct MultiTuple {
  static constexpr int l0 = L0, l1 = L1, l2 = L2;
  static constexpr int count = L2 < 0 ? 2 : 3;
};
template <int L0, int L1, class F>
decltype(auto) with_multi_third(int l2, F&& f) {
  if (l2 < 0) return f(MultiTuple<L0, L1, -1>{});
  if constexpr (L1 <= 0) { if (l2 == 0) return f(MultiTuple<L0, L1, 0>{}); }
  if constexpr (L1 <= 1) { if (l2 == 1) return f(MultiTuple<L0, L1, 1>{}); }
  return f(MultiTuple<L0, L1, 2>{});
}
template <int L0, class F>
decltype(auto) with_multi_second(int l1, int l2, F&& f) {
  if constexpr (L0 <= 0) { if (l1 == 0) return with_multi_third<L0, 0>(l2, f); }
  if constexpr (L0 <= 1) { if (l1 == 1) return with_multi_third<L0, 1>(l2, f); }
  return with_multi_third<L0, 2>(l2, f);
}
// l0 <= l1 (<= l2 unless l2 < 0), all marked
template <class F>
decltype(auto) with_multi_tuple(int l0, int l1, int l2, F&& f) {
  static_assert(MULTI_LOSSES == 3, "the three-way chains above list the marked loss types");
  if (l0 == 0) return with_multi_second<0>(l1, l2, f);
  if (l0 == 1) return with_multi_second<1>(l1, l2, f);
  return with_multi_second<2>(l1, l2, f);
}

}  // namespace gd3d
