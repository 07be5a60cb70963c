// Minimum word error rate (MWER) loss over an N-best list: the exact
// CTC log-probability of N hypotheses that share one utterance's logits, the expected
// error over the list and its logit gradient.  Per utterance b with hypotheses
// y_0 .. y_{n-1} (n = n_hyp[b]) and integer errors e_i:
//   ll_i   = log P_CTC(y_i | x)                       (srf_ctc_loss's -nll)
//   p_i    = exp(ll_i - LSE_k ll_k),  d_i = e_i - mean_k e_k
//   loss_b = sum_i p_i d_i,           w_i = p_i (d_i - loss_b) = d loss_b / d ll_i
//   grad   = grad_scale * sum_i w_i occ_i,  occ_i[t, c] = exp(LSE_{s: ext_i[s] = c}(alpha_i + beta_i) - lp - ll_i)
// (sum_i w_i = 0, so the softmax terms of the CTC gradients cancel).  Four launches:
//   1. log-softmax of every frame, once per utterance, into the workspace;
//   2. alpha and beta of all B * N hypotheses, grid (B * N, 2), the recursions of
//      ctc.hip (ctc_dev.h) reading the utterance's log-softmax (from LDS if it fits),
//      each block choosing its recursion by its own hypothesis's length;
//   3. p, loss and w per utterance (one wave);
//   4. the gradient, grid (B, frame blocks): per hypothesis with w_i != 0 the
//      next-occurrence lists of ctc_grad_kernel, alpha + beta staged in LDS, the sum
//      over hypotheses kept in LDS by the thread that owns the (frame, class).
// Workspace, in floats: lp [B][Tmax][C] | alpha, beta [B * N][2][Tmax][Smax] | w [B][N],
// Smax = 2 Lmax + 1.
#include <cmath>
#include <type_traits>

#include "srf_common.h"
#include "ctc_dev.h"
#include "../../include/srf.h"

namespace {

using namespace srf_ctc;

constexpr int kMaxN = SRF_MWER_MAX_HYP;
constexpr size_t kLds = 64 * 1024;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// grid (B, ceil(Tmax / 4)), one wave per frame
__global__ __launch_bounds__(256) void mwer_lsm_kernel(const float* __restrict__ logits,
                                                       const int* __restrict__ logit_len, int Tmax, int C,
                                                       float* __restrict__ lp) {
  const int b = blockIdx.x, t = blockIdx.y * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
  if (t >= clampi(logit_len[b], 0, Tmax)) return;
  const float* x = logits + ((size_t)b * Tmax + t) * C;
  float* y = lp + ((size_t)b * Tmax + t) * C;
  float m = -INFINITY;
  for (int c = l; c < C; c += 64) m = fmaxf(m, x[c]);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  float z = 0.f;
  for (int c = l; c < C; c += 64) z += __expf(x[c] - m);
  z = wave_sum(z);
  const float lz = m + __logf(z);
  for (int c = l; c < C; c += 64) y[c] = x[c] - lz;
}

// grid (B * N, 2): block (r, 0) runs alpha of hypothesis r = b N + i and writes ll[r],
// block (r, 1) runs beta: srf_ctc_loss's recursions, wave-resident for up to 512
// extended-label states (S = 2 L + 1 in <= 128, <= 256, <= 512), else the block loop.
// Dynamic LDS: ext[Smax] (int) | row[2][Smax] | lp[Tmax * C] (LPLDS).
template <bool LPLDS>
__global__ __launch_bounds__(256) void mwer_recursion_kernel(const float* __restrict__ lpg,
                                                             const int* __restrict__ hyp,
                                                             const int* __restrict__ hyp_len,
                                                             const int* __restrict__ n_hyp,
                                                             const int* __restrict__ logit_len, int N, int Tmax,
                                                             int C, int Lmax, int blank, int want_beta,
                                                             float* __restrict__ ll, float* __restrict__ ab) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int Smax = 2 * Lmax + 1;
  int* ext = reinterpret_cast<int*>(smem);
  float* row = smem + Smax;
  const int r = blockIdx.x, b = r / N, i = r - b * N;
  const bool is_beta = blockIdx.y == 1;
  if (is_beta && !want_beta) return;
  if (i >= clampi(n_hyp[b], 0, N)) {
    if (!is_beta && threadIdx.x == 0) ll[r] = -INFINITY;
    return;
  }
  const int L = clampi(hyp_len[r], 0, Lmax);
  const int Tb = clampi(logit_len[b], 0, Tmax);
  const int S = 2 * L + 1;
  const float* lpb = lpg + (size_t)b * Tmax * C;
  float* lp = row + 2 * Smax;
  float* out = ab + ((size_t)r * 2 + (is_beta ? 1 : 0)) * Tmax * Smax;
  // a label outside [0, C) has no emission: such a hypothesis counts as infeasible
  int bad = 0;
  for (int s = threadIdx.x; s < S; s += blockDim.x) {
    int e = blank;
    if (s & 1) {
      e = hyp[(size_t)r * Lmax + (s >> 1)];
      bad |= e < 0 || e >= C;
    }
    ext[s] = e;
  }
  if constexpr (LPLDS) {
    for (int k = threadIdx.x; k < Tb * C; k += blockDim.x) lp[k] = lpb[k];
  }
  if (__syncthreads_or(bad) || Tb == 0) {
    // the gradient skips the hypothesis (p = 0, so w = 0) and never reads its rows
    if (!is_beta && threadIdx.x == 0) ll[r] = -INFINITY;
    return;
  }
  const float* em = LPLDS ? lp : lpb;
  // The row width Smax comes from the widest row the caller allows (a list taken at
  // max_len = max_frames has Lmax = T), the hypothesis itself is usually much shorter:
  // the wave-resident recursion is chosen by its own S (the same in every thread).
  if (S <= 512) {
    if (threadIdx.x >= 64) return;
    auto wave = [&](auto km) {
      constexpr int K = decltype(km)::value;
      if (!is_beta) {
        const float v = alpha_wave<K>(ext, em, C, S, Tb, Smax, blank, out);
        if (threadIdx.x == 0) ll[r] = v;
      } else {
        beta_wave<K>(ext, em, C, S, Tb, Smax, blank, out);
      }
    };
    if (S <= 128)
      wave(std::integral_constant<int, 2>{});
    else if (S <= 256)
      wave(std::integral_constant<int, 4>{});
    else
      wave(std::integral_constant<int, 8>{});
    return;
  }
  if (!is_beta) {
    for (int t = 0; t < Tb; ++t) {
      const float* ap = row + ((t + 1) & 1) * Smax;
      float* an = row + (t & 1) * Smax;
      for (int s = threadIdx.x; s < S; s += blockDim.x) {
        float a;
        if (t == 0) {
          a = (s < 2) ? 0.f : -INFINITY;
        } else {
          a = ap[s];
          if (s >= 1) a = lse2(a, ap[s - 1]);
          if (s >= 2 && ext[s] != blank && ext[s] != ext[s - 2]) a = lse2(a, ap[s - 2]);
        }
        a = (a == -INFINITY) ? -INFINITY : a + em[(size_t)t * C + ext[s]];
        an[s] = a;
        out[(size_t)t * Smax + s] = a;
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      const float* al = row + ((Tb - 1) & 1) * Smax;
      float v = al[S - 1];
      if (S >= 2) v = lse2(v, al[S - 2]);
      ll[r] = v;
    }
  } else {
    for (int t = Tb - 1; t >= 0; --t) {
      const float* bp = row + ((t + 1) & 1) * Smax;
      float* bn = row + (t & 1) * Smax;
      for (int s = threadIdx.x; s < S; s += blockDim.x) {
        float a;
        if (t == Tb - 1) {
          a = (s >= S - 2) ? 0.f : -INFINITY;
        } else {
          a = bp[s];
          if (s + 1 < S) a = lse2(a, bp[s + 1]);
          if (s + 2 < S && ext[s] != blank && ext[s] != ext[s + 2]) a = lse2(a, bp[s + 2]);
        }
        a = (a == -INFINITY) ? -INFINITY : a + em[(size_t)t * C + ext[s]];
        bn[s] = a;
        out[(size_t)t * Smax + s] = a;
      }
      __syncthreads();
    }
  }
}

// grid B, one wave: lane i holds hypothesis i (N <= 32).  d_i = (n e_i - sum e) / n has an
// integer numerator, so equal errors give d = 0, loss = 0 and w = 0 exactly.
__global__ __launch_bounds__(64) void mwer_weights_kernel(const float* __restrict__ ll,
                                                          const int* __restrict__ n_hyp,
                                                          const int* __restrict__ err, int N,
                                                          float* __restrict__ p_hat, float* __restrict__ loss,
                                                          float* __restrict__ w) {
  const int b = blockIdx.x, i = threadIdx.x;
  const int n = clampi(n_hyp[b], 0, N);
  const bool on = i < n;
  const float l = on ? ll[(size_t)b * N + i] : -INFINITY;
  float m = l;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  long long se = on ? (long long)err[(size_t)b * N + i] : 0;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) se += __shfl_xor(se, o, 64);
  float p = 0.f, d = 0.f;
  if (m > -INFINITY) {   // some hypothesis is feasible (then n >= 1)
    const float z = l == -INFINITY ? 0.f : expf(l - m);
    p = z / wave_sum(z);
    if (on) d = (float)((long long)n * err[(size_t)b * N + i] - se) / (float)n;
  }
  const float lo = wave_sum(p * d);
  if (i < N) {
    p_hat[(size_t)b * N + i] = p;
    w[(size_t)b * N + i] = p * (d - lo);
  }
  if (i == 0) loss[b] = lo;
}

// grid (B, ceil(Tmax / FR)), 256 threads = FR frames x 256 / FR class lanes.
// Dynamic LDS: head[C] | next[Lmax] (int) | acc[FR][C] | ab[FR][Smax].
__global__ __launch_bounds__(256) void mwer_grad_kernel(const int* __restrict__ hyp, const int* __restrict__ hyp_len,
                                                        const int* __restrict__ n_hyp,
                                                        const int* __restrict__ logit_len,
                                                        const float* __restrict__ ll, const float* __restrict__ w,
                                                        int N, int Tmax, int C, int Lmax, int blank, float scale,
                                                        int FR, const float* __restrict__ lpg,
                                                        const float* __restrict__ abg, float* __restrict__ grad) {
  extern __shared__ __attribute__((aligned(16))) int lists[];
  int* head = lists;
  int* next = lists + C;
  float* acc = reinterpret_cast<float*>(lists + C + Lmax);
  const int Smax = 2 * Lmax + 1;
  float* ab = acc + (size_t)FR * C;
  const int b = blockIdx.x;
  const int Tb = clampi(logit_len[b], 0, Tmax);
  const int n = clampi(n_hyp[b], 0, N);
  const int t0 = blockIdx.y * FR;
  const int lanes = blockDim.x / FR;
  const int tt = threadIdx.x / lanes, cl = threadIdx.x % lanes;
  const int t = t0 + tt;
  const int nt = min(FR, Tb - t0);   // frames of this block inside the utterance
  for (int c = cl; c < C; c += lanes) acc[tt * C + c] = 0.f;
  if (nt > 0) {
    const float* lp = lpg + (size_t)b * Tmax * C;
    for (int i = 0; i < n; ++i) {
      const size_t r = (size_t)b * N + i;
      const float wi = w[r];
      if (wi == 0.f) continue;   // the same in every thread; an infeasible hypothesis has p = 0
      const float li = ll[r];
      const int L = clampi(hyp_len[r], 0, Lmax), S = 2 * L + 1;
      const int* lab = hyp + r * Lmax;
      const float* alpha = abg + r * 2 * Tmax * Smax;
      const float* beta = alpha + (size_t)Tmax * Smax;
      // first occurrence of each class and next occurrence of each label position
      for (int c = threadIdx.x; c < C; c += blockDim.x) {
        int h = -1;
        for (int k = L - 1; k >= 0; --k) h = lab[k] == c ? k : h;
        head[c] = h;
      }
      for (int k = threadIdx.x; k < L; k += blockDim.x) {
        const int c = lab[k];
        int nx = -1;
        for (int k2 = L - 1; k2 > k; --k2) nx = lab[k2] == c ? k2 : nx;
        next[k] = nx;
      }
      for (int j = threadIdx.x; j < nt * S; j += blockDim.x) {
        const int ft = j / S, s = j - ft * S;
        const size_t o = (size_t)(t0 + ft) * Smax + s;
        ab[ft * Smax + s] = alpha[o] + beta[o];
      }
      __syncthreads();
      if (tt < nt) {
        const float* abt = ab + tt * Smax;
        for (int c = cl; c < C; c += lanes) {
          float a = -INFINITY;
          if (c == blank) {
            for (int s2 = 0; s2 <= 2 * L; s2 += 2) a = lse2f(a, abt[s2]);
          } else {
            for (int k = head[c]; k >= 0; k = next[k]) a = lse2f(a, abt[2 * k + 1]);
          }
          if (a != -INFINITY) acc[tt * C + c] += wi * __expf(a - lp[(size_t)t * C + c] - li);
        }
      }
      __syncthreads();   // the lists and ab are rewritten for the next hypothesis
    }
  }
  if (t >= Tmax) return;
  float* gb = grad + ((size_t)b * Tmax + t) * C;
  for (int c = cl; c < C; c += lanes) gb[c] = t < Tb ? acc[tt * C + c] * scale : 0.f;
}

size_t rec_lds(int Lmax) { return 3 * (2 * (size_t)Lmax + 1) * sizeof(float); }
size_t grad_lds(int C, int Lmax, int fr) {
  return ((size_t)C + Lmax) * sizeof(int) + (size_t)fr * ((size_t)C + 2 * (size_t)Lmax + 1) * sizeof(float);
}

bool shape_ok(int B, int Tmax, int C, int N, int Lmax) {
  if (!(B >= 1 && Tmax >= 1 && Tmax <= 65535 && C >= 2 && N >= 1 && N <= kMaxN && Lmax >= 0)) return false;
  if ((long long)B * N > 0x7fffffffll) return false;
  if (rec_lds(Lmax) > kLds || grad_lds(C, Lmax, 1) > kLds) return false;
  return (size_t)Tmax * (2 * (size_t)Lmax + 1) <= ((size_t)1 << 29);   // a row block below 2^31 bytes
}

#define SRF_MWER_SHAPE_MSG(what)                                                                                     \
  what ": need B >= 1, 1 <= Tmax <= 65535, C >= 2, 1 <= N <= %d, Lmax >= 0, B N < 2^31, Tmax (2 Lmax + 1) <= 2^29 "  \
       "and LDS lists of at most 64 KiB (12 (2 Lmax + 1) and 4 (2 C + 3 Lmax + 1) bytes) "                           \
       "(B=%d Tmax=%d C=%d N=%d Lmax=%d)",                                                                           \
      kMaxN, B, Tmax, C, N, Lmax

}  // namespace

extern "C" size_t srf_mwer_workspace(int B, int Tmax, int C, int N, int Lmax) {
  if (!shape_ok(B, Tmax, C, N, Lmax)) {
    srf::set_error(SRF_MWER_SHAPE_MSG("mwer_workspace"));
    return 0;
  }
  const size_t Smax = 2 * (size_t)Lmax + 1;
  return ((size_t)B * Tmax * C + (size_t)B * N * Tmax * 2 * Smax + (size_t)B * N) * sizeof(float);
}

extern "C" int srf_mwer_loss(const float* logits, const int* logit_len, const int* hyp, const int* hyp_len,
                             const int* n_hyp, const int* err, int B, int Tmax, int C, int N, int Lmax, int blank,
                             float grad_scale, float* hyp_logp, float* p_hat, float* loss, float* grad,
                             void* workspace, size_t workspace_bytes, void* stream) {
  SRF_REQUIRE(shape_ok(B, Tmax, C, N, Lmax), SRF_MWER_SHAPE_MSG("mwer_loss"));
  SRF_REQUIRE(blank >= 0 && blank < C, "mwer_loss: blank = %d outside [0, %d)", blank, C);
  SRF_REQUIRE(logits && logit_len && hyp_len && n_hyp && err && hyp_logp && p_hat && loss && workspace &&
                  (hyp || Lmax == 0),
              "mwer_loss: null pointer argument");
  const size_t need = srf_mwer_workspace(B, Tmax, C, N, Lmax);
  if (workspace_bytes < need) {
    srf::set_error("mwer_loss: the workspace holds %zu bytes, %zu are needed", workspace_bytes, need);
    return SRF_EWORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t Smax = 2 * (size_t)Lmax + 1;
  float* lp = static_cast<float*>(workspace);
  float* ab = lp + (size_t)B * Tmax * C;
  float* w = ab + (size_t)B * N * Tmax * 2 * Smax;
  hipLaunchKernelGGL(mwer_lsm_kernel, dim3((unsigned)B, (unsigned)((Tmax + 3) / 4)), dim3(256), 0, st, logits,
                     logit_len, Tmax, C, lp);
  SRF_LAUNCH_CHECK("mwer_lsm");
  size_t shmem = rec_lds(Lmax);
  const size_t lp_bytes = (size_t)Tmax * C * sizeof(float);
  const bool lp_in_lds = shmem + lp_bytes <= kLds;
  if (lp_in_lds) shmem += lp_bytes;
  auto kern = lp_in_lds ? mwer_recursion_kernel<true> : mwer_recursion_kernel<false>;
  hipLaunchKernelGGL(kern, dim3((unsigned)(B * N), 2), dim3(256), shmem, st, lp, hyp, hyp_len, n_hyp, logit_len, N,
                     Tmax, C, Lmax, blank, grad ? 1 : 0, hyp_logp, ab);
  SRF_LAUNCH_CHECK("mwer_recursion");
  hipLaunchKernelGGL(mwer_weights_kernel, dim3((unsigned)B), dim3(64), 0, st, hyp_logp, n_hyp, err, N, p_hat, loss,
                     w);
  SRF_LAUNCH_CHECK("mwer_weights");
  if (grad) {
    int fr = 16;
    while (fr > 1 && grad_lds(C, Lmax, fr) > kLds) fr >>= 1;
    hipLaunchKernelGGL(mwer_grad_kernel, dim3((unsigned)B, (unsigned)((Tmax + fr - 1) / fr)), dim3(256),
                       grad_lds(C, Lmax, fr), st, hyp, hyp_len, n_hyp, logit_len, hyp_logp, w, N, Tmax, C, Lmax,
                       blank, grad_scale, fr, lp, ab, grad);
    SRF_LAUNCH_CHECK("mwer_grad");
  }
  return SRF_OK;
}
