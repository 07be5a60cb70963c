// Endpointing on the device (srf_amd/endpoint.py): where a stream's
// utterance ends, decided from the CTC logits alone.  Per frame two flags,
//   is_sil = log_softmax(x)[blank] > log(blank_threshold),   is_sp = argmax(x) != blank,
// drive an integer machine per stream -- n (frames in the open segment), sil (trailing
// silence run), speech (a label was seen), t (frames consumed):
//   n += 1;  sil = is_sil ? sil + 1 : 0;  speech |= is_sp
//   reason = 2 if speech and sil >= silence_after_speech, else 1 if sil >= silence_only,
//            else 3 if n >= max_segment, else 0
//   if reason: emit (t - n + 1, t, reason);  n = sil = 0;  speech = false
// The flags are fp32, everything after them is integer: the cuts are a function of the
// stream's frames, whatever the chunking, the batch and the other streams.
//
// One workgroup per stream.  The frames are independent, so its waves take them round
// robin (the wave-wide max / arg-max / sum butterfly of the greedy decoder, stream.hip)
// and leave a byte of flags per frame in LDS, a tile of frames at a time so that any
// chunk length fits; then one lane runs the machine over the tile's bytes, the only
// serial part.
#include "srf_common.h"
#include "../../include/srf.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTile = 512;         // frames whose flags lie in LDS at once
constexpr int kStateWords = 4;     // per stream: n, sil, speech, t

__global__ __launch_bounds__(kThreads) void ctc_endpoint_kernel(const float* __restrict__ logits,
                                                                const int* __restrict__ n_valid, int n, int C,
                                                                int blank, float log_thr, int silence_only,
                                                                int silence_after_speech, int max_segment,
                                                                int* __restrict__ state, int max_cuts,
                                                                int* __restrict__ cut_start, int* __restrict__ cut_end,
                                                                int* __restrict__ cut_reason,
                                                                int* __restrict__ n_cuts) {
  __shared__ unsigned char flags[kTile];
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int nv = max(0, min(n_valid[b], n));
  const float* x = logits + (size_t)b * n * C;
  int* cs = cut_start + (size_t)b * max_cuts;
  int* ce = cut_end + (size_t)b * max_cuts;
  int* cr = cut_reason + (size_t)b * max_cuts;
  for (int i = t; i < max_cuts; i += kThreads) cs[i] = ce[i] = cr[i] = -1;
  int* st = state + (size_t)b * kStateWords;
  // (lane 0 of wave 0 alone reads and writes these)
  int seg = 0, sil = 0, speech = 0, now = 0, cuts = 0;
  if (t == 0) {
    seg = st[0];
    sil = st[1];
    speech = st[2];
    now = st[3];
  }
  for (int f0 = 0; f0 < nv; f0 += kTile) {
    const int nf = min(kTile, nv - f0);
    for (int f = wave; f < nf; f += kWaves) {
      const float* row = x + (size_t)(f0 + f) * C;
      // the first maximum of the lane's classes, then of the wave: the larger value and,
      // on equal values, the lower class (torch.argmax, srf_ctc_greedy_n)
      float best = -__builtin_inff();
      int arg = 0x7fffffff;
      for (int c = lane; c < C; c += 64) {
        const float v = row[c];
        if (arg == 0x7fffffff || v > best) {
          best = v;
          arg = c;
        }
      }
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oa = __shfl_xor(arg, o, 64);
        if (oa != 0x7fffffff && (arg == 0x7fffffff || ob > best || (ob == best && oa < arg))) {
          best = ob;
          arg = oa;
        }
      }
      float se = 0.f;
      for (int c = lane; c < C; c += 64) se += expf(row[c] - best);
      se = wave_sum(se);
      if (lane == 0) {
        const float lp_blank = row[blank] - (best + logf(se));
        flags[f] = (unsigned char)((lp_blank > log_thr ? 1 : 0) | (arg != blank ? 2 : 0));
      }
    }
    __syncthreads();   // the tile's flags are written; the -1 fill of the outputs too
    if (t == 0) {
      for (int f = 0; f < nf; ++f) {
        const int fl = flags[f];
        ++seg;
        sil = (fl & 1) ? sil + 1 : 0;
        speech |= fl >> 1;
        const int reason = speech && sil >= silence_after_speech ? 2
                           : sil >= silence_only                 ? 1
                           : seg >= max_segment                  ? 3
                                                                 : 0;
        if (reason) {
          if (cuts < max_cuts) {
            cs[cuts] = now - seg + 1;
            ce[cuts] = now;
            cr[cuts] = reason;
          }
          ++cuts;
          seg = sil = speech = 0;
        }
        ++now;
      }
    }
    __syncthreads();   // the flags are read before the next tile overwrites them
  }
  if (t == 0) {
    st[0] = seg;
    st[1] = sil;
    st[2] = speech;
    st[3] = now;
    n_cuts[b] = cuts;
  }
}

}  // namespace

extern "C" size_t srf_ctc_endpoint_state_bytes(int B) {
  if (B < 1) {
    srf::set_error("ctc_endpoint_state_bytes: need B >= 1 (B=%d)", B);
    return 0;
  }
  return (size_t)B * kStateWords * sizeof(int);
}

extern "C" int srf_ctc_endpoint_reset(void* state, int B, void* stream) {
  SRF_REQUIRE(state && B >= 1, "ctc_endpoint_reset: need a state block and B >= 1 (B=%d)", B);
  SRF_HIP_TRY(hipMemsetAsync(state, 0, (size_t)B * kStateWords * sizeof(int), static_cast<hipStream_t>(stream)));
  return SRF_OK;
}

extern "C" int srf_ctc_endpoint_n(const float* logits, const int* n_valid, int B, int n, int C, int blank,
                                  float log_thr, int silence_only, int silence_after_speech, int max_segment,
                                  void* state, int max_cuts, int* cut_start, int* cut_end, int* cut_reason,
                                  int* n_cuts, void* stream) {
  SRF_REQUIRE(B >= 1 && n >= 0 && C >= 2, "ctc_endpoint: need B >= 1, n >= 0, C >= 2 (B=%d n=%d C=%d)", B, n, C);
  SRF_REQUIRE(blank >= 0 && blank < C, "ctc_endpoint: blank = %d outside [0, %d)", blank, C);
  SRF_REQUIRE(silence_only >= 1 && silence_after_speech >= 1 && max_segment >= 1,
              "ctc_endpoint: the three counts are at least 1 (silence_only=%d silence_after_speech=%d max_segment=%d)",
              silence_only, silence_after_speech, max_segment);
  SRF_REQUIRE(log_thr < 0.f && log_thr > -__builtin_inff(), "ctc_endpoint: log_thr = %g is no log of a threshold in (0, 1)",
              (double)log_thr);
  SRF_REQUIRE(max_cuts >= 1, "ctc_endpoint: need max_cuts >= 1, got %d", max_cuts);
  SRF_REQUIRE(n_valid && state && cut_start && cut_end && cut_reason && n_cuts, "ctc_endpoint: null pointer argument");
  SRF_REQUIRE(n == 0 || logits, "ctc_endpoint: null logits with n = %d", n);
  if (n == 0) return SRF_OK;
  hipLaunchKernelGGL(ctc_endpoint_kernel, dim3((unsigned)B), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                     logits, n_valid, n, C, blank, log_thr, silence_only, silence_after_speech, max_segment,
                     static_cast<int*>(state), max_cuts, cut_start, cut_end, cut_reason, n_cuts);
  SRF_LAUNCH_CHECK("ctc_endpoint");
  return SRF_OK;
}
