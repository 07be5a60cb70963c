// CTC recursion helpers shared by ctc.hip (srf_ctc_loss) and mwer.hip (srf_mwer_loss):
// the log-sum-exp forms and the wave-resident alpha / beta recursions over the extended
// label.  Both alpha_t(s) and beta_t(s) include the emission at t.
#pragma once
#include <cmath>

#include "srf_common.h"

namespace srf_ctc {

__device__ __forceinline__ float lse2(float a, float b) {
  const float m = fmaxf(a, b);
  if (m == -INFINITY) return -INFINITY;
  return m + __logf(__expf(a - m) + __expf(b - m));
}

// Branch-free log(e^a + e^b) for the serial recursions: with m = max(a, b) taken as
// 0 when both are -inf, e^(a-m) + e^(b-m) is 0 there and v_log_f32 returns -inf; the
// sum lies in [1, 2] otherwise, so the raw exp2/log2 instructions need no range fix-up.
__device__ __forceinline__ float lse2f(float a, float b) {
  constexpr float kLog2e = 1.4426950408889634f, kLn2 = 0.6931471805599453f;
  const float m = fmaxf(a, b);
  const float ms = m == -INFINITY ? 0.f : m;
  const float z = __builtin_amdgcn_exp2f((a - ms) * kLog2e) + __builtin_amdgcn_exp2f((b - ms) * kLog2e);
  return ms + __builtin_amdgcn_logf(z) * kLn2;
}

// log(e^a + e^b + e^c) in one step (one max3, three exp, one log; the sum lies in
// [1, 3], or is 0 when all three are -inf), so a recursion step has one
// log-sum-exp on its serial chain instead of two nested ones.
__device__ __forceinline__ float lse3(float a, float b, float c) {
  constexpr float kLog2e = 1.4426950408889634f, kLn2 = 0.6931471805599453f;
  const float m = fmaxf(fmaxf(a, b), c);
  const float ms = m == -INFINITY ? 0.f : m;
  const float z = __builtin_amdgcn_exp2f((a - ms) * kLog2e) + __builtin_amdgcn_exp2f((b - ms) * kLog2e) +
                  __builtin_amdgcn_exp2f((c - ms) * kLog2e);
  return ms + __builtin_amdgcn_logf(z) * kLn2;
}

// Wave-resident recursions (KM > 0, S <= 64*KM): wave 0 holds states
// s = lane + 64k in registers; the s-1 / s-2 (alpha) or s+1 / s+2 (beta)
// neighbours come from DPP whole-wave shifts (wave_shr:1 / wave_shl:1, a VALU
// move instead of an LDS-crossbar shuffle on the serial path), the lanes at a
// 64-state boundary taking the neighbouring group's values (v_readlane), so a
// time step needs no barrier.
__device__ __forceinline__ float dpp_wave_shr1(float old, float src) {   // lane l <- src[l-1], lane 0 <- old
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(src), 0x138, 0xF, 0xF, false));
}
__device__ __forceinline__ float dpp_wave_shl1(float old, float src) {   // lane l <- src[l+1], lane 63 <- old
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(src), 0x130, 0xF, 0xF, false));
}
__device__ __forceinline__ float read_lane(float v, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
// The emission row of step t + 1 is read while step t's log-sum-exps run.
template <int KM>
__device__ __forceinline__ float alpha_wave(const int* __restrict__ ext, const float* __restrict__ lp, int C, int S,
                                            int Tb, int Smax, int blank, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const auto ors = __builtin_amdgcn_make_buffer_rsrc(out, 0, Tb * Smax * 4, 0x00020000);
  float a[KM], em[KM];
  int e[KM];
  bool sk[KM], live[KM];
#pragma unroll
  for (int k = 0; k < KM; ++k) {
    const int s = lane + 64 * k;
    live[k] = s < S;
    e[k] = live[k] ? ext[s] : blank;
    sk[k] = live[k] && s >= 2 && ext[s] != blank && ext[s] != ext[s - 2];
    a[k] = -INFINITY;
    em[k] = Tb > 0 ? lp[e[k]] : 0.f;
  }
  for (int t = 0; t < Tb; ++t) {
    float emn[KM];
    const int tn = min(t + 1, Tb - 1);
#pragma unroll
    for (int k = 0; k < KM; ++k) emn[k] = lp[(size_t)tn * C + e[k]];
    float na[KM];
#pragma unroll
    for (int k = 0; k < KM; ++k) {
      const int s = lane + 64 * k;
      float v;
      if (t == 0) {
        v = s < 2 ? 0.f : -INFINITY;
      } else {
        const float l63 = k > 0 ? read_lane(a[k - 1], 63) : -INFINITY;
        const float l62 = k > 0 ? read_lane(a[k - 1], 62) : -INFINITY;
        const float p1 = dpp_wave_shr1(l63, a[k]);    // state s - 1
        const float p2 = dpp_wave_shr1(l62, p1);      // state s - 2
        v = lse3(a[k], p1, sk[k] ? p2 : -INFINITY);
      }
      v = live[k] ? v + em[k] : -INFINITY;            // -inf stays -inf
      na[k] = v;
      // no exec branch on the serial path: dead lanes store out of the buffer's range
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), ors, live[k] ? (uint32_t)(t * Smax + s) * 4 : 0x80000000u,
                                            0, 0);
    }
#pragma unroll
    for (int k = 0; k < KM; ++k) {
      a[k] = na[k];
      em[k] = emn[k];
    }
  }
  // log-likelihood: the last two states at t = Tb-1
  float loc = -INFINITY;
#pragma unroll
  for (int k = 0; k < KM; ++k) {
    const int s = lane + 64 * k;
    if (Tb > 0 && (s == S - 1 || s == S - 2)) loc = lse2(loc, a[k]);
  }
  float m = loc;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if (m == -INFINITY) return -INFINITY;
  const float z = wave_sum(loc == -INFINITY ? 0.f : __expf(loc - m));
  return m + __logf(z);
}

template <int KM>
__device__ __forceinline__ void beta_wave(const int* __restrict__ ext, const float* __restrict__ lp, int C, int S,
                                          int Tb, int Smax, int blank, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const auto ors = __builtin_amdgcn_make_buffer_rsrc(out, 0, Tb * Smax * 4, 0x00020000);
  float a[KM], em[KM];
  int e[KM];
  bool sk[KM], live[KM];
#pragma unroll
  for (int k = 0; k < KM; ++k) {
    const int s = lane + 64 * k;
    live[k] = s < S;
    e[k] = live[k] ? ext[s] : blank;
    sk[k] = s + 2 < S && ext[s] != blank && ext[s] != ext[s + 2];
    a[k] = -INFINITY;
    em[k] = Tb > 0 ? lp[(size_t)(Tb - 1) * C + e[k]] : 0.f;
  }
  for (int t = Tb - 1; t >= 0; --t) {
    float emn[KM];
    const int tn = max(t - 1, 0);
#pragma unroll
    for (int k = 0; k < KM; ++k) emn[k] = lp[(size_t)tn * C + e[k]];
    float na[KM];
#pragma unroll
    for (int k = 0; k < KM; ++k) {
      const int s = lane + 64 * k;
      float v;
      if (t == Tb - 1) {
        v = s >= S - 2 ? 0.f : -INFINITY;
      } else {
        const float h0 = k + 1 < KM ? read_lane(a[k + 1], 0) : -INFINITY;
        const float h1 = k + 1 < KM ? read_lane(a[k + 1], 1) : -INFINITY;
        const float q1 = dpp_wave_shl1(h0, a[k]);     // state s + 1
        const float q2 = dpp_wave_shl1(h1, q1);       // state s + 2
        v = lse3(a[k], q1, sk[k] ? q2 : -INFINITY);
      }
      v = live[k] ? v + em[k] : -INFINITY;
      na[k] = v;
      // no exec branch on the serial path: dead lanes store out of the buffer's range
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), ors, live[k] ? (uint32_t)(t * Smax + s) * 4 : 0x80000000u,
                                            0, 0);
    }
#pragma unroll
    for (int k = 0; k < KM; ++k) {
      a[k] = na[k];
      em[k] = emn[k];
    }
  }
}

}  // namespace srf_ctc
