// In-kernel time stamps of the diagnostic builds (tools/kernel_stamps.py): one facility for every kernel file.
//
// A SET is a named __device__ array of clock values and its read-back entry rcb_debug_stamps_<SET>.  It exists only in a
// build with -DRCB_STAMPS_<SET>=1 (python -m recombiner_amd.build --variant ... --only FILE -DRCB_STAMPS_<SET>=1); in the
// library every macro below expands to nothing (RCB_STAMPS_BARRIER: to __syncthreads()).  The sets are independent.
//   RCB_STAMPS_BUFFER(SET, n)           file scope, outside any namespace: the array g_stamps_<SET>[n] and its entry
//   RCB_STAMP(SET, who, slot, clock)    if (who) g_stamps_<SET>[slot] = the clock now; clock: memtime (shader clock) or
//                                       memrealtime (100 MHz wall clock)
//   RCB_STAMPS_PHASES(SET)              declares the phase sums ph_[8] and starts the phase clock (memtime)
//   RCB_STAMPS_PHASE(SET, k)            ph_[k] += the time since the previous phase boundary
//   RCB_STAMPS_PHASES_STORE(SET, who, at)  if (who) g_stamps_<SET>[at .. at + 7] = ph_[0 .. 7]
//   RCB_STAMPS_BARRIER(SET, acc)        __syncthreads() with the shader-clock time spent in it added to acc
//   RCB_STAMPS_ONLY(SET, code)          code of the stamps build alone (declarations, wall-clock slots, the store of ph_)
#pragma once
#include <hip/hip_runtime.h>

// RCB_STAMPS_IF(SET)(code): code where RCB_STAMPS_<SET> is 1, nothing where it is 0 or not defined -- what `#if` decides,
// inside a macro: only the flag's value 1 pastes to RCB_STAMPS_IS_1, whose comma moves the 1 into the place that is picked
#define RCB_STAMPS_CAT_(a, b) a##b
#define RCB_STAMPS_CAT(a, b) RCB_STAMPS_CAT_(a, b)
#define RCB_STAMPS_IS_1 ~, 1
#define RCB_STAMPS_SECOND(a, b, ...) b
#define RCB_STAMPS_PICK(...) RCB_STAMPS_SECOND(__VA_ARGS__)
#define RCB_STAMPS_ON(flag) RCB_STAMPS_PICK(RCB_STAMPS_CAT(RCB_STAMPS_IS_, flag), 0, ~)
#define RCB_STAMPS_IF(set) RCB_STAMPS_CAT(RCB_STAMPS_IF_, RCB_STAMPS_ON(RCB_STAMPS_##set))
#define RCB_STAMPS_IF_0(...)
#define RCB_STAMPS_IF_1(...) __VA_ARGS__

#define RCB_STAMPS_ONLY(set, ...) RCB_STAMPS_IF(set)(__VA_ARGS__)
#define RCB_STAMPS_BUFFER(set, n)                                                                                        \
  RCB_STAMPS_ONLY(set, __device__ unsigned long long g_stamps_##set[n];                                                  \
                  extern "C" int rcb_debug_stamps_##set(unsigned long long* dst, int count) {                            \
                    if (count > (n)) count = (n);                                                                        \
                    return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_stamps_##set), sizeof(unsigned long long) * count); \
                  })
#define RCB_STAMP(set, who, slot, clock) RCB_STAMPS_ONLY(set, if (who) g_stamps_##set[slot] = __builtin_amdgcn_s_##clock())
#define RCB_STAMPS_PHASES(set) \
  RCB_STAMPS_ONLY(set, unsigned long long ph_[8] = {0, 0, 0, 0, 0, 0, 0, 0}, last_ = __builtin_amdgcn_s_memtime())
#define RCB_STAMPS_PHASE(set, k)                                                  \
  RCB_STAMPS_ONLY(set, {                                                          \
    const unsigned long long now_ = __builtin_amdgcn_s_memtime();                 \
    ph_[k] += now_ - last_;                                                       \
    last_ = now_;                                                                 \
  })
#define RCB_STAMPS_PHASES_STORE(set, who, at) \
  RCB_STAMPS_ONLY(set, if (who) for (int k_ = 0; k_ < 8; ++k_) g_stamps_##set[(at) + k_] = ph_[k_])
#define RCB_STAMPS_BARRIER(set, acc)                                              \
  do {                                                                            \
    RCB_STAMPS_ONLY(set, const unsigned long long tb_ = __builtin_amdgcn_s_memtime();) \
    __syncthreads();                                                              \
    RCB_STAMPS_ONLY(set, acc += __builtin_amdgcn_s_memtime() - tb_;)              \
  } while (0)
