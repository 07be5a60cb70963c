// CTC forced alignment: the best path of a given labelling through an utterance's
// frames (Viterbi), the max-plus counterpart of ctc.hip's alpha recursion plus a
// backtrace.  One workgroup per utterance:
//   lp       = log_softmax(logits[b, t, :])                t < T_b
//   v_t(s)   = max(v_{t-1}(s), v_{t-1}(s-1), [skip] v_{t-1}(s-2)) + lp[t, l'_s]
//   score_b  = max(v_{T_b-1}(S-2), v_{T_b-1}(S-1))
// over the extended label l' (|l'| = S = 2L+1, even states blank), the skip allowed
// into a label state whose label differs from the one two states back.  Ties: among
// equal predecessors the lowest source state wins (s-2 before s-1 before s); at the
// last frame S-2 unless S-1 is strictly larger.  An infeasible utterance yields
// score = -inf, states / tok_start / tok_end = -1 and tok_logp = 0.
//
// Wave 0 runs the recursion with the states in registers (KM groups of 64, as
// alpha_wave); every lane packs its states' two-bit choices, 16 frames to a word, and
// stores the words to LDS (workspace when ceil(T / 16) * KM * 256 bytes do not fit).
// Lane 0 walks them back, then the workgroup fills the outputs in parallel.  S > 512: a
// workgroup loop with byte back-pointers in the workspace.
#include <cmath>

#include "srf_common.h"
#include "../../include/srf.h"

namespace {

constexpr size_t kAlignLds = 96 * 1024;

__device__ __forceinline__ float dpp_wave_shr1(float old, float src) {   // lane l <- src[l-1], lane 0 <- old
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(src), 0x138, 0xF, 0xF, false));
}
__device__ __forceinline__ float read_lane(float v, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// LDS head shared by both kernels: ext[Smax] | path[Tmax] | tok_start[Lmax] | tok_end[Lmax]
// | fin[4] (int), padded to 16 bytes.
__host__ __device__ inline size_t align_head_bytes(int Tmax, int Lmax) {
  return (((size_t)(2 * Lmax + 1) + Tmax + 2 * (size_t)Lmax + 4) * 4 + 15) & ~(size_t)15;
}

// Per-utterance workspace: lp[Tmax][C] | back-pointers (the wave recursion's words at
// KM = 8, or one byte per frame and state for the workgroup loop), each padded to 16 bytes.
__host__ __device__ inline size_t align_lp_bytes(int Tmax, int C) { return ((size_t)Tmax * C * 4 + 15) & ~(size_t)15; }
// bytes of the wave recursion's back-pointer words: 16 frames per word, 64 KM states
__host__ __device__ inline size_t align_bp_word_bytes(int Tmax, int KM) {
  return (size_t)((Tmax + 15) / 16) * 64 * KM * 4;
}
__host__ __device__ inline size_t align_bp_bytes(int Tmax, int Lmax) {
  const size_t words = align_bp_word_bytes(Tmax, 8), bytes = (size_t)Tmax * (2 * Lmax + 1);
  return ((words > bytes ? words : bytes) + 15) & ~(size_t)15;
}

// log_softmax of the utterance's rows into lp: LDS (rows staged coalesced, then one
// thread per row, as ctc_recursion_kernel) or workspace (one wave per row).
template <bool LPLDS>
__device__ __forceinline__ void stage_log_softmax(const float* __restrict__ lg, float* __restrict__ lp, int Tb, int C) {
  if constexpr (LPLDS) {
    const int n = Tb * C;
    for (int i0 = threadIdx.x; i0 < n; i0 += 8 * 256) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = lg[min(i0 + u * 256, n - 1)];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (i0 + u * 256 < n) lp[i0 + u * 256] = v[u];
    }
    __syncthreads();
    for (int t = threadIdx.x; t < Tb; t += blockDim.x) {
      float* r = lp + (size_t)t * C;
      float m = -INFINITY;
#pragma unroll 8
      for (int c = 0; c < C; ++c) m = r[c] > m ? r[c] : m;
      float z = 0.f;
#pragma unroll 8
      for (int c = 0; c < C; ++c) z += __expf(r[c] - m);
      const float lz = m + __logf(z);
#pragma unroll 8
      for (int c = 0; c < C; ++c) r[c] -= lz;
    }
  } else {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63, nw = blockDim.x >> 6;
    for (int t = w; t < Tb; t += nw) {
      float m = -INFINITY;
      for (int c = l; c < C; c += 64) m = fmaxf(m, lg[(size_t)t * C + c]);
      m = wave_max(m);
      float z = 0.f;
      for (int c = l; c < C; c += 64) z += __expf(lg[(size_t)t * C + c] - m);
      z = wave_sum(z);
      const float lz = m + __logf(z);
      for (int c = l; c < C; c += 64) lp[(size_t)t * C + c] = lg[(size_t)t * C + c] - lz;
    }
    __threadfence();   // the rows are read by other waves of this workgroup
  }
  __syncthreads();
}

// The choice among the three predecessors: 2 (s-2) before 1 (s-1) before 0 (stay) on
// equal values; p2 is -inf where the skip is not allowed.
__device__ __forceinline__ float max3_choice(float a, float p1, float p2, bool skip, bool& c1, bool& c2) {
  c2 = skip && p2 >= p1 && p2 >= a;
  c1 = !c2 && p1 >= a;
  return fmaxf(fmaxf(a, p1), p2);
}

// Wave-resident Viterbi recursion (S <= 64 * KM), called by wave 0.  Every lane packs the
// choices of its own states, two bits per frame (0 stay, 1 from s-1, 2 from s-2), 16
// frames to a word, the frame's code at bits 2 * (15 - t % 16); word bp[(t / 16) * 64 KM
// + s] is stored after every 16th frame and after the last.  Lanes past S - 1 carry
// values that no live state reads (the recursion only looks down).  Returns the score in
// every lane (-inf: infeasible) and the final state.
template <int KM>
__device__ __forceinline__ float viterbi_wave(const int* __restrict__ ext, const float* __restrict__ lp, int C, int S,
                                              int Tb, int blank, unsigned* __restrict__ bp, int& final_state) {
  const int lane = threadIdx.x & 63;
  float a[KM], em[KM];
  int e[KM];
  unsigned hist[KM];
  bool sk[KM];
#pragma unroll
  for (int k = 0; k < KM; ++k) {
    const int s = lane + 64 * k;
    const bool live = s < S;
    e[k] = live ? ext[s] : blank;
    sk[k] = live && s >= 2 && ext[s] != blank && ext[s] != ext[s - 2];
    a[k] = -INFINITY;
    em[k] = Tb > 0 ? lp[e[k]] : 0.f;
    hist[k] = 0;
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
      unsigned code = 0;
      if (t == 0) {
        v = s < 2 ? 0.f : -INFINITY;
      } else {
        const float l63 = k > 0 ? read_lane(a[k - 1], 63) : -INFINITY;
        const float l62 = k > 0 ? read_lane(a[k - 1], 62) : -INFINITY;
        const float p1 = dpp_wave_shr1(l63, a[k]);                        // state s - 1
        const float q2 = dpp_wave_shr1(l62, p1);                          // state s - 2 (every lane takes part)
        const float p2 = sk[k] ? q2 : -INFINITY;                          // -inf where the skip is not allowed
        // lowest source state first: s-2 if it is no smaller than both others, else s-1 if no
        // smaller than s (all -inf: the state is unreachable and its code is never read)
        // (selects on the comparisons, not fmaxf: no NaN can occur and none needs quieting)
        const bool c1 = p1 >= a[k];
        const float m1 = c1 ? p1 : a[k];
        const bool c2 = p2 >= m1;
        v = c2 ? p2 : m1;
        code = c2 ? 2u : c1 ? 1u : 0u;
      }
      na[k] = v + em[k];                                                  // -inf stays -inf
      hist[k] = (hist[k] << 2) | code;
    }
    if ((t & 15) == 15 || t == Tb - 1) {
      const int sh = 2 * (15 - (t & 15));
#pragma unroll
      for (int k = 0; k < KM; ++k) bp[(size_t)(t >> 4) * (64 * KM) + lane + 64 * k] = hist[k] << sh;
    }
#pragma unroll
    for (int k = 0; k < KM; ++k) {
      a[k] = na[k];
      em[k] = emn[k];
    }
  }
  // the last two states at t = Tb-1: S-2 unless S-1 is strictly larger
  float vl = -INFINITY, vp = -INFINITY;
#pragma unroll
  for (int k = 0; k < KM; ++k) {
    const int s = lane + 64 * k;
    if (s == S - 1) vl = a[k];
    if (s == S - 2) vp = a[k];
  }
  vl = wave_max(vl);
  vp = wave_max(vp);
  if (Tb <= 0) {
    final_state = 0;
    return S == 1 ? 0.f : -INFINITY;
  }
  const bool last = S < 2 || vl > vp;
  final_state = last ? S - 1 : S - 2;
  return last ? vl : vp;
}

// After the backtrace: states, the labels' frame runs and their log-probability sums, by
// the whole workgroup.  fin[0]: the utterance is feasible (path[0 .. Tb) is then valid).
__device__ __forceinline__ void fill_outputs(int b, int Tb, int Tmax, int C, int Lmax, const int* __restrict__ ext,
                                             const int* __restrict__ path, int* __restrict__ tst,
                                             int* __restrict__ ten, const int* __restrict__ fin,
                                             const float* __restrict__ lp, int* __restrict__ states,
                                             int* __restrict__ tok_start, int* __restrict__ tok_end,
                                             float* __restrict__ tok_logp) {
  for (int k = threadIdx.x; k < Lmax; k += blockDim.x) {
    tst[k] = -1;
    ten[k] = -1;
  }
  __syncthreads();
  const bool ok = fin[0] != 0;
  for (int t = threadIdx.x; t < Tmax; t += blockDim.x) {
    const int s = ok && t < Tb ? path[t] : -1;
    states[(size_t)b * Tmax + t] = s;
    if (s >= 0 && (s & 1)) {
      if (t == 0 || path[t - 1] != s) tst[s >> 1] = t;
      if (t == Tb - 1 || path[t + 1] != s) ten[s >> 1] = t + 1;
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < Lmax; k += blockDim.x) {
    const int t0 = tst[k], t1 = ten[k];
    float acc = 0.f;
    if (t0 >= 0) {
      const int c = ext[2 * k + 1];
      for (int t = t0; t < t1; ++t) acc += lp[(size_t)t * C + c];
    }
    tok_start[(size_t)b * Lmax + k] = t0;
    tok_end[(size_t)b * Lmax + k] = t1;
    tok_logp[(size_t)b * Lmax + k] = acc;
  }
}

// The extended label into LDS; label values are clamped to [0, C), so that no label can
// make the recursion read outside a row of lp.
__device__ __forceinline__ void build_ext(int* __restrict__ ext, const int* __restrict__ lab, int S, int C, int blank) {
  for (int s = threadIdx.x; s < S; s += blockDim.x) ext[s] = (s & 1) ? max(0, min(lab[s >> 1], C - 1)) : blank;
}

// Dynamic LDS: head | back-pointers [ceil(Tmax / 16)][64 KM] words (BPLDS) | lp[Tmax * C] (LPLDS).
template <int KM, bool LPLDS, bool BPLDS>
__global__ __launch_bounds__(256) void ctc_align_kernel(const float* __restrict__ logits,
                                                        const int* __restrict__ labels,
                                                        const int* __restrict__ label_len,
                                                        const int* __restrict__ logit_len, int Tmax, int C, int Lmax,
                                                        int blank, int* __restrict__ states,
                                                        int* __restrict__ tok_start, int* __restrict__ tok_end,
                                                        float* __restrict__ tok_logp, float* __restrict__ score,
                                                        char* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int Smax = 2 * Lmax + 1;
  int* ext = reinterpret_cast<int*>(smem_raw);
  int* path = ext + Smax;
  int* tst = path + Tmax;
  int* ten = tst + Lmax;
  int* fin = ten + Lmax;
  const size_t head = align_head_bytes(Tmax, Lmax);
  const int b = blockIdx.x;
  const int L = max(0, min(label_len[b], Lmax));
  const int Tb = max(0, min(logit_len[b], Tmax));
  const int S = 2 * L + 1;
  char* wsb = ws + (size_t)b * (align_lp_bytes(Tmax, C) + align_bp_bytes(Tmax, Lmax));
  unsigned* bp = reinterpret_cast<unsigned*>(BPLDS ? smem_raw + head : wsb + align_lp_bytes(Tmax, C));
  float* lp = reinterpret_cast<float*>(LPLDS ? smem_raw + head + align_bp_word_bytes(Tmax, KM) : wsb);
  const float* lg = logits + (size_t)b * Tmax * C;
  build_ext(ext, labels + (size_t)b * Lmax, S, C, blank);
  stage_log_softmax<LPLDS>(lg, lp, Tb, C);   // ends with a barrier: ext is complete too
  if (threadIdx.x < 64) {
    int fs;
    const float sc = viterbi_wave<KM>(ext, lp, C, S, Tb, blank, bp, fs);
    if constexpr (!BPLDS) __threadfence();   // lane 0 reads what every lane stored
    if (threadIdx.x == 0) {
      score[b] = sc;
      fin[0] = sc > -INFINITY;
      if (sc > -INFINITY && Tb > 0) {
        int s = fs;
        for (int t = Tb - 1; t >= 1; --t) {
          path[t] = s;
          s -= (int)(bp[(size_t)(t >> 4) * (64 * KM) + s] >> (2 * (15 - (t & 15))) & 3u);
        }
        path[0] = s;
      }
    }
  }
  __syncthreads();
  fill_outputs(b, Tb, Tmax, C, Lmax, ext, path, tst, ten, fin, lp, states, tok_start, tok_end, tok_logp);
}

// S > 512: the workgroup walks the states, two rows of values in LDS, one byte per frame
// and state (0, 1, 2: how far back the predecessor lies) in the workspace.
// Dynamic LDS: head | row[2][Smax].
__global__ __launch_bounds__(256) void ctc_align_loop_kernel(const float* __restrict__ logits,
                                                             const int* __restrict__ labels,
                                                             const int* __restrict__ label_len,
                                                             const int* __restrict__ logit_len, int Tmax, int C,
                                                             int Lmax, int blank, int* __restrict__ states,
                                                             int* __restrict__ tok_start, int* __restrict__ tok_end,
                                                             float* __restrict__ tok_logp, float* __restrict__ score,
                                                             char* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int Smax = 2 * Lmax + 1;
  int* ext = reinterpret_cast<int*>(smem_raw);
  int* path = ext + Smax;
  int* tst = path + Tmax;
  int* ten = tst + Lmax;
  int* fin = ten + Lmax;
  float* row = reinterpret_cast<float*>(smem_raw + align_head_bytes(Tmax, Lmax));
  const int b = blockIdx.x;
  const int L = max(0, min(label_len[b], Lmax));
  const int Tb = max(0, min(logit_len[b], Tmax));
  const int S = 2 * L + 1;
  char* wsb = ws + (size_t)b * (align_lp_bytes(Tmax, C) + align_bp_bytes(Tmax, Lmax));
  float* lp = reinterpret_cast<float*>(wsb);
  unsigned char* bp = reinterpret_cast<unsigned char*>(wsb + align_lp_bytes(Tmax, C));
  const float* lg = logits + (size_t)b * Tmax * C;
  build_ext(ext, labels + (size_t)b * Lmax, S, C, blank);
  stage_log_softmax<false>(lg, lp, Tb, C);
  for (int t = 0; t < Tb; ++t) {
    const float* ap = row + ((t + 1) & 1) * Smax;
    float* an = row + (t & 1) * Smax;
    for (int s = threadIdx.x; s < S; s += blockDim.x) {
      float v;
      bool c1 = false, c2 = false;
      if (t == 0) {
        v = s < 2 ? 0.f : -INFINITY;
      } else {
        const bool skip = s >= 2 && ext[s] != blank && ext[s] != ext[s - 2];
        v = max3_choice(ap[s], s >= 1 ? ap[s - 1] : -INFINITY, skip ? ap[s - 2] : -INFINITY, skip, c1, c2);
      }
      an[s] = v + lp[(size_t)t * C + ext[s]];
      bp[(size_t)t * Smax + s] = c2 ? 2 : c1 ? 1 : 0;
    }
    __syncthreads();
  }
  __threadfence();   // thread 0 reads every thread's back-pointers
  __syncthreads();
  if (threadIdx.x == 0) {
    float sc = L == 0 ? 0.f : -INFINITY;
    int s = 0;
    if (Tb > 0) {
      const float* al = row + ((Tb - 1) & 1) * Smax;
      const bool last = S < 2 || al[S - 1] > al[S - 2];
      s = last ? S - 1 : S - 2;
      sc = al[s];
    }
    score[b] = sc;
    fin[0] = sc > -INFINITY;
    if (sc > -INFINITY && Tb > 0) {
      for (int t = Tb - 1; t >= 1; --t) {
        path[t] = s;
        s -= bp[(size_t)t * Smax + s];
      }
      path[0] = s;
    }
  }
  __syncthreads();
  fill_outputs(b, Tb, Tmax, C, Lmax, ext, path, tst, ten, fin, lp, states, tok_start, tok_end, tok_logp);
}

using AlignKernel = void (*)(const float*, const int*, const int*, const int*, int, int, int, int, int*, int*, int*,
                             float*, float*, char*);

template <int KM>
AlignKernel pick_align(bool lp_lds, bool bp_lds) {
  return lp_lds ? ctc_align_kernel<KM, true, true> : bp_lds ? ctc_align_kernel<KM, false, true>
                                                            : ctc_align_kernel<KM, false, false>;
}

}  // namespace

extern "C" {

size_t srf_ctc_align_workspace(int B, int Tmax, int C, int Lmax) {
  if (B <= 0 || Tmax <= 0 || C <= 0 || Lmax < 0) return 0;
  return (size_t)B * (align_lp_bytes(Tmax, C) + align_bp_bytes(Tmax, Lmax));
}

int srf_ctc_align(const float* logits, const int* labels, const int* label_len, const int* logit_len, int B, int Tmax,
                  int C, int Lmax, int blank, int* states, int* tok_start, int* tok_end, float* tok_logp, float* score,
                  void* workspace, size_t workspace_bytes, void* stream) {
  SRF_REQUIRE(logits && label_len && logit_len && states && score && workspace, "ctc_align: null pointer argument");
  SRF_REQUIRE(B > 0 && Tmax > 0 && C > 1 && Lmax >= 0 && blank >= 0 && blank < C,
              "ctc_align: bad shape (B=%d Tmax=%d C=%d Lmax=%d blank=%d)", B, Tmax, C, Lmax, blank);
  SRF_REQUIRE(Lmax == 0 || (labels && tok_start && tok_end && tok_logp),
              "ctc_align: null labels / token outputs with Lmax = %d", Lmax);
  SRF_REQUIRE((uintptr_t)workspace % 16 == 0, "ctc_align: the workspace must be 16-byte aligned");
  if (workspace_bytes < srf_ctc_align_workspace(B, Tmax, C, Lmax)) {
    srf::set_error("CTC alignment workspace too small");
    return SRF_EWORKSPACE;
  }
  const size_t Smax = 2 * (size_t)Lmax + 1;
  const size_t head = align_head_bytes(Tmax, Lmax);
  SRF_REQUIRE(head + 2 * Smax * sizeof(float) <= kAlignLds,
              "ctc_align: Tmax = %d frames with Lmax = %d labels exceed the kernel's LDS tables", Tmax, Lmax);
  hipStream_t st = static_cast<hipStream_t>(stream);
  AlignKernel kern;
  size_t shmem;
  if (Smax > 512) {
    kern = ctc_align_loop_kernel;
    shmem = head + 2 * Smax * sizeof(float);
  } else {
    // wave-resident recursion for up to 512 extended-label states; the back-pointers go to
    // LDS first (the backtrace's dependent reads), then the log-probabilities
    const int KM = Smax <= 128 ? 2 : Smax <= 256 ? 4 : 8;
    const size_t bp_bytes = align_bp_word_bytes(Tmax, KM), lp_bytes = (size_t)Tmax * C * sizeof(float);
    const bool bp_lds = head + bp_bytes <= kAlignLds;
    const bool lp_lds = bp_lds && head + bp_bytes + lp_bytes <= kAlignLds;
    shmem = head + (bp_lds ? bp_bytes : 0) + (lp_lds ? lp_bytes : 0);
    kern = KM == 2 ? pick_align<2>(lp_lds, bp_lds) : KM == 4 ? pick_align<4>(lp_lds, bp_lds)
                                                             : pick_align<8>(lp_lds, bp_lds);
  }
  if (shmem > 64 * 1024)
    SRF_HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
  hipLaunchKernelGGL(kern, dim3(B), dim3(256), shmem, st, logits, labels, label_len, logit_len, Tmax, C, Lmax, blank,
                     states, tok_start, tok_end, tok_logp, score, static_cast<char*>(workspace));
  SRF_LAUNCH_CHECK("ctc_align");
  return SRF_OK;
}

}  // extern "C"
