// Waveform front end (srf_amd/fbank.py): 16 kHz samples to the
// 123-d features the model reads -- Kaldi's compute-fbank-feats (40 mel bins, log energy,
// snip-edges), add-deltas (order 2, window 2) and the reference's CMVN -- offline and
// chunked.  All arithmetic is fp32; the window, the twiddles and the mel weights come
// from srf_fbank_tables, which computes them on the host in double and rounds once.
//
// srf_fbank_static: one wave per frame, four frames per workgroup.  The 512-point real
// FFT of the zero-padded frame runs as a 256-point complex radix-2 FFT in the wave's 2 KB
// of LDS plus the split step; one lane per mel filter then sums its bin range of the
// power spectrum in ascending order.  A frame's 41 values are a pure function of its 400
// samples (and, with dither, of their global indices): no atomics, no dependence on the
// grid, so any chunking of a signal gives the same bits.
// srf_fbank_deltas: delta and delta-delta of the statics with the frame index clamped per
// utterance, fused with the CMVN and the zeroing of the rows past an utterance's end.
// srf_fbank_stats: per-dimension sum and sum of squares in fp64 plus the frame count,
// one workgroup per dimension, added to device-resident sums.
#include <cfloat>
#include <cmath>
#include <vector>

#include "srf_common.h"
#include "srf_rng.h"
#include "../../include/srf.h"

namespace {

constexpr int kFrameLen = SRF_FBANK_FRAME_LEN, kShift = SRF_FBANK_FRAME_SHIFT;
constexpr int kFft = 512, kBins = 256, kMel = SRF_FBANK_MEL, kStatic = SRF_FBANK_STATIC, kFeat = SRF_FBANK_FEAT;
constexpr int kMelW = 40;   // slots per filter in the weight table (the widest filter has 31 bins)
// table layout, in floats
constexpr int kOffWindow = 0, kOffTw = 400, kOffMelLo = kOffTw + 2 * kBins, kOffMelN = kOffMelLo + kMel;
constexpr int kOffMelW = kOffMelN + kMel, kTableFloats = kOffMelW + kMel * kMelW;
constexpr int kMaxFrames = 0x7fffffff / kShift - 8;   // 160 t + 399 stays an int
constexpr int kFramesPerBlock = 4;

__host__ __device__ inline int frames_of(int n) { return n < kFrameLen ? 0 : 1 + (n - kFrameLen) / kShift; }

double mel_of(double f) { return 1127.0 * std::log(1.0 + f / 700.0); }

bool build_tables(float* out) {
  const double pi = 3.14159265358979323846;
  for (int i = 0; i < kFrameLen; ++i)
    out[kOffWindow + i] = (float)std::pow(0.5 - 0.5 * std::cos(2.0 * pi * i / (kFrameLen - 1)), 0.85);
  for (int k = 0; k < kBins; ++k) {   // exp(-2 pi i k / 512)
    out[kOffTw + 2 * k] = (float)std::cos(2.0 * pi * k / kFft);
    out[kOffTw + 2 * k + 1] = (float)-std::sin(2.0 * pi * k / kFft);
  }
  const double lo = mel_of(20.0), hi = mel_of(8000.0), step = (hi - lo) / (kMel + 1);
  for (int f = 0; f < kMel; ++f) {
    const double left = lo + f * step, center = lo + (f + 1) * step, right = lo + (f + 2) * step;
    int first = -1, n = 0;
    for (int k = 0; k < kBins; ++k) {
      const double m = mel_of(16000.0 / kFft * k);
      if (!(m > left && m < right)) continue;
      if (first < 0) first = k;
      if (k != first + n || n >= kMelW) return false;   // a filter's bins are one run of at most kMelW
      out[kOffMelW + f * kMelW + n++] = (float)(m <= center ? (m - left) / (center - left) : (right - m) / (right - center));
    }
    if (first < 0) return false;
    for (int j = n; j < kMelW; ++j) out[kOffMelW + f * kMelW + j] = 0.f;
    out[kOffMelLo + f] = (float)first;
    out[kOffMelN + f] = (float)n;
  }
  return true;
}

__device__ __forceinline__ unsigned bitrev8(unsigned n) { return __brev(n) >> 24; }

// standard Gaussian of sample idx of stream row b: Box-Muller on two uniforms of the
// dither stream, keyed by (seed, b, idx) alone
__device__ __forceinline__ float dither_gauss(uint64_t seed, int b, int idx) {
  const uint64_t s = seed + (uint64_t)(unsigned)b * 0x9E3779B97F4A7C15ull;
  const float u1 = 1.0f - srf_uniform(s, kStreamDither, 2ull * (unsigned)idx);   // (0, 1]
  const float u2 = srf_uniform(s, kStreamDither, 2ull * (unsigned)idx + 1ull);
  return sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * u2);
}

// Frame t of stream b (blockIdx.y) by wave w of the workgroup; every wave runs every
// barrier, a wave without a frame computes on zeros and stores nothing.
__global__ __launch_bounds__(64 * kFramesPerBlock) void fbank_static_kernel(
    const void* __restrict__ samples, int is_int16, const int* __restrict__ n_samples,
    const float* __restrict__ tab, int stride, int s0, int n_limit, int t0, int t1, int f0, int Ts, float dither,
    unsigned long long seed, float* __restrict__ out) {
  __shared__ float lds[kFramesPerBlock][2 * kBins];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, b = blockIdx.y;
  const int t = t0 + (int)blockIdx.x * kFramesPerBlock + wave;
  const int Tb = frames_of(min(max(n_samples[b], 0), n_limit));
  const bool in_range = t < t1, valid = in_range && t < Tb;
  float* re = lds[wave];
  float* im = re + kBins;
  float* row = out + ((size_t)b * Ts + (size_t)(t - f0)) * kStatic;

  // samples lane + 64 j of the frame, dithered
  constexpr int kPer = (kFrameLen + 63) / 64;
  float x[kPer];
  const size_t base = (size_t)b * stride + (size_t)(valid ? t * kShift - s0 : 0);
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int i = lane + 64 * j;
    float v = 0.f;
    if (valid && i < kFrameLen) {
      v = is_int16 ? (float)static_cast<const short*>(samples)[base + i] : static_cast<const float*>(samples)[base + i];
      if (dither != 0.f) v += dither * dither_gauss(seed, b, t * kShift + i);
    }
    x[j] = v;
  }
  // mean removal and the raw log energy
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < kPer; ++j) s += x[j];
  const float mean = wave_sum(s) * (1.0f / kFrameLen);
  float e = 0.f;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int i = lane + 64 * j;
    x[j] = i < kFrameLen ? x[j] - mean : 0.f;
    e += x[j] * x[j];
  }
  const float log_energy = logf(fmaxf(wave_sum(e), FLT_EPSILON));
  // pre-emphasis reads the neighbour through LDS
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int i = lane + 64 * j;
    if (i < kFrameLen) re[i] = x[j];
  }
  __syncthreads();
  float y[kPer];
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int i = lane + 64 * j;
    y[j] = i < kFrameLen ? (x[j] - 0.97f * re[max(i - 1, 0)]) * tab[kOffWindow + i] : 0.f;
  }
  __syncthreads();
  // z[n] = y[2n] + i y[2n + 1], bit-reversed for the in-place decimation-in-time FFT
#pragma unroll
  for (int j = 0; j < 2 * kBins / 64; ++j) {
    const int i = lane + 64 * j;
    const float v = j < kPer ? y[j < kPer ? j : 0] : 0.f;
    const unsigned p = bitrev8((unsigned)i >> 1);
    if (i & 1)
      im[p] = v;
    else
      re[p] = v;
  }
  __syncthreads();
#pragma unroll
  for (int st = 1; st <= 8; ++st) {
    const int half = 1 << (st - 1);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int k = lane + 64 * r, j = k & (half - 1), i0 = ((k >> (st - 1)) << st) + j, i1 = i0 + half;
      const int tw = (j << (8 - st)) * 2;   // exp(-2 pi i j / 2^st) in the 512-point table
      const float wr = tab[kOffTw + 2 * tw], wi = tab[kOffTw + 2 * tw + 1];
      const float ar = re[i0], ai = im[i0], br = re[i1], bi = im[i1];
      const float tr = wr * br - wi * bi, ti = wr * bi + wi * br;
      re[i0] = ar + tr;
      im[i0] = ai + ti;
      re[i1] = ar - tr;
      im[i1] = ai - ti;
    }
    __syncthreads();
  }
  // split step: X[k] = (Z[k] + conj Z[256 - k]) / 2 - i w^k (Z[k] - conj Z[256 - k]) / 2
  float pw[kBins / 64];
#pragma unroll
  for (int j = 0; j < kBins / 64; ++j) {
    const int k = lane + 64 * j, k2 = (kBins - k) & (kBins - 1);
    const float ar = re[k], ai = im[k], br = re[k2], bi = -im[k2];
    const float er = 0.5f * (ar + br), ei = 0.5f * (ai + bi);   // even samples' spectrum
    const float dr = 0.5f * (ar - br), di = 0.5f * (ai - bi);
    const float or_ = di, oi = -dr;                            // odd samples': -i d
    const float wr = tab[kOffTw + 2 * k], wi = tab[kOffTw + 2 * k + 1];
    const float xr = er + (wr * or_ - wi * oi), xi = ei + (wr * oi + wi * or_);
    pw[j] = xr * xr + xi * xi;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kBins / 64; ++j) re[lane + 64 * j] = pw[j];
  __syncthreads();
  if (lane < kMel) {
    const int lo = (int)tab[kOffMelLo + lane], n = (int)tab[kOffMelN + lane];
    const float* w = tab + kOffMelW + lane * kMelW;
    float acc = 0.f;
    for (int j = 0; j < n; ++j) acc += w[j] * re[lo + j];
    if (in_range) row[1 + lane] = valid ? logf(fmaxf(acc, FLT_EPSILON)) : 0.f;
  } else if (lane == kMel) {
    if (in_range) row[0] = valid ? log_energy : 0.f;
  }
}

constexpr int kDeltaFrames = 4;

// Thread (frame, d < 41) of stream blockIdx.y: the static, its delta and its delta-delta.
__global__ __launch_bounds__(64 * kDeltaFrames) void fbank_deltas_kernel(
    const float* __restrict__ st, const int* __restrict__ n_frames, int Ts, int f0, int t_limit, int t0, int t1,
    const float* __restrict__ mean, const float* __restrict__ stdv, int cmvn_rows, float* __restrict__ out, int To,
    int o0) {
  const int d = threadIdx.x & 63, b = blockIdx.y;
  const int t = t0 + (int)blockIdx.x * kDeltaFrames + (int)(threadIdx.x >> 6);
  if (t >= t1 || d >= kStatic) return;
  const int Tb = min(max(n_frames[b], 0), t_limit);
  float* o = out + ((size_t)b * To + (size_t)(t - o0)) * kFeat;
  if (t >= Tb) {
    o[d] = 0.f;
    o[d + kStatic] = 0.f;
    o[d + 2 * kStatic] = 0.f;
    return;
  }
  const float* sb = st + (size_t)b * Ts * kStatic + d;
  float v[9];
#pragma unroll
  for (int j = 0; j < 9; ++j) {
    const int r = min(max(min(max(t + j - 4, 0), Tb - 1) - f0, 0), Ts - 1);
    v[j] = sb[(size_t)r * kStatic];
  }
  float f[3];
  f[0] = v[4];
  f[1] = -0.2f * v[2] + -0.1f * v[3] + 0.1f * v[5] + 0.2f * v[6];
  f[2] = 0.04f * v[0] + 0.04f * v[1] + 0.01f * v[2] + -0.04f * v[3] + -0.1f * v[4] + -0.04f * v[5] + 0.01f * v[6] +
         0.04f * v[7] + 0.04f * v[8];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int c = d + k * kStatic;
    if (cmvn_rows) {
      const size_t m = (cmvn_rows > 1 ? (size_t)b * kFeat : 0) + c;
      f[k] = (f[k] - mean[m] + 1e-14f) / (stdv[m] + 1e-14f);
    }
    o[c] = f[k];
  }
}

constexpr int kStatThreads = 256;

// Workgroup d owns dimension d: its threads stride over the B * T rows with fp64
// accumulators, reduce them in a fixed order and add to sums; workgroup 0 also counts.
__global__ __launch_bounds__(kStatThreads) void fbank_stats_kernel(const float* __restrict__ feats,
                                                                   const int* __restrict__ n_frames, int B, int T,
                                                                   int D, double* __restrict__ sums) {
  __shared__ double red[2][kStatThreads];
  const int d = blockIdx.x, tid = threadIdx.x;
  double s1 = 0.0, s2 = 0.0;
  for (int b = 0; b < B; ++b) {
    const int Tb = min(max(n_frames[b], 0), T);
    const float* x = feats + (size_t)b * T * D + d;
    for (int t = tid; t < Tb; t += kStatThreads) {
      const double v = (double)x[(size_t)t * D];
      s1 += v;
      s2 += v * v;
    }
  }
  red[0][tid] = s1;
  red[1][tid] = s2;
  __syncthreads();
  for (int o = kStatThreads / 2; o >= 1; o >>= 1) {
    if (tid < o) {
      red[0][tid] += red[0][tid + o];
      red[1][tid] += red[1][tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    sums[d] += red[0][0];
    sums[D + d] += red[1][0];
    if (d == 0) {
      double n = 0.0;
      for (int b = 0; b < B; ++b) n += (double)min(max(n_frames[b], 0), T);
      sums[2 * D] += n;
    }
  }
}

}  // namespace

extern "C" int srf_fbank_num_frames(int n_samples) { return frames_of(n_samples); }

extern "C" size_t srf_fbank_table_floats(void) { return (size_t)kTableFloats; }

extern "C" int srf_fbank_tables(float* tables, size_t n_floats) {
  SRF_REQUIRE(tables && n_floats >= (size_t)kTableFloats, "fbank_tables: need a host buffer of %d floats, got %zu",
              kTableFloats, n_floats);
  std::vector<float> t(kTableFloats);
  SRF_REQUIRE(build_tables(t.data()), "fbank_tables: a mel filter does not fit its %d table slots", kMelW);
  for (int i = 0; i < kTableFloats; ++i) tables[i] = t[i];
  return SRF_OK;
}

extern "C" int srf_fbank_static(const void* samples, int is_int16, const int* n_samples, const float* tables, int B,
                                int stride, int width, int s0, int n_limit, int t0, int t1, int f0, int Ts,
                                float dither, unsigned long long seed, float* statics, void* stream) {
  SRF_REQUIRE(B >= 1 && B <= 65535, "fbank_static: need 1 <= B <= 65535 (B=%d)", B);
  SRF_REQUIRE(width >= 0 && stride >= width, "fbank_static: need 0 <= width <= stride (width=%d stride=%d)", width,
              stride);
  SRF_REQUIRE(0 <= t0 && t0 <= t1 && t1 <= kMaxFrames, "fbank_static: bad frame range [%d, %d)", t0, t1);
  if (t1 == t0) return SRF_OK;
  SRF_REQUIRE(samples && n_samples && tables && statics, "fbank_static: null pointer argument");
  SRF_REQUIRE(s0 >= 0 && (long long)kShift * t0 >= s0, "fbank_static: frame %d starts before the buffer's first sample %d",
              t0, s0);
  SRF_REQUIRE(n_limit >= 0 && (long long)n_limit <= (long long)s0 + width,
              "fbank_static: n_limit %d lies beyond the buffer (samples %d .. %lld)", n_limit, s0,
              (long long)s0 + width);
  SRF_REQUIRE(Ts >= 1 && t0 >= f0 && (long long)t1 - f0 <= Ts,
              "fbank_static: frames [%d, %d) outside the statics buffer (frames %d .. %lld)", t0, t1, f0,
              (long long)f0 + Ts);
  SRF_REQUIRE(dither >= 0.f && dither < HUGE_VALF, "fbank_static: dither must be finite and >= 0");
  const unsigned gx = (unsigned)((t1 - t0 + kFramesPerBlock - 1) / kFramesPerBlock);
  hipLaunchKernelGGL(fbank_static_kernel, dim3(gx, (unsigned)B), dim3(64 * kFramesPerBlock), 0,
                     static_cast<hipStream_t>(stream), samples, is_int16, n_samples, tables, stride, s0, n_limit, t0,
                     t1, f0, Ts, dither, seed, statics);
  SRF_LAUNCH_CHECK("fbank_static");
  return SRF_OK;
}

extern "C" int srf_fbank_deltas(const float* statics, const int* n_frames, int B, int Ts, int f0, int t_limit, int t0,
                                int t1, const float* mean, const float* stdev, int cmvn_rows, float* feats, int To,
                                int o0, void* stream) {
  SRF_REQUIRE(B >= 1 && B <= 65535, "fbank_deltas: need 1 <= B <= 65535 (B=%d)", B);
  SRF_REQUIRE(0 <= t0 && t0 <= t1 && t1 <= kMaxFrames && t_limit >= 0, "fbank_deltas: bad frame range [%d, %d), limit %d",
              t0, t1, t_limit);
  SRF_REQUIRE(cmvn_rows == 0 || cmvn_rows == 1 || cmvn_rows == B,
              "fbank_deltas: cmvn_rows is 0 (none), 1 (shared) or B (per stream), got %d", cmvn_rows);
  if (t1 == t0) return SRF_OK;
  SRF_REQUIRE(statics && n_frames && feats && (cmvn_rows == 0 || (mean && stdev)), "fbank_deltas: null pointer argument");
  SRF_REQUIRE(To >= 1 && t0 >= o0 && (long long)t1 - o0 <= To,
              "fbank_deltas: frames [%d, %d) outside the output buffer (frames %d .. %lld)", t0, t1, o0,
              (long long)o0 + To);
  // statics read: frames t0 - 4 .. t1 + 3 clamped to [0, min(T_b, t_limit) - 1]
  const int lo = t0 - 4 > 0 ? t0 - 4 : 0, hi = t1 + 3 < t_limit - 1 ? t1 + 3 : t_limit - 1;
  SRF_REQUIRE(Ts >= 1 && (hi < lo || (lo >= f0 && (long long)hi - f0 < Ts)),
              "fbank_deltas: statics frames [%d, %d] outside the statics buffer (frames %d .. %lld)", lo, hi, f0,
              (long long)f0 + Ts);
  const unsigned gx = (unsigned)((t1 - t0 + kDeltaFrames - 1) / kDeltaFrames);
  hipLaunchKernelGGL(fbank_deltas_kernel, dim3(gx, (unsigned)B), dim3(64 * kDeltaFrames), 0,
                     static_cast<hipStream_t>(stream), statics, n_frames, Ts, f0, t_limit, t0, t1, mean, stdev,
                     cmvn_rows, feats, To, o0);
  SRF_LAUNCH_CHECK("fbank_deltas");
  return SRF_OK;
}

extern "C" int srf_fbank_stats(const float* feats, const int* n_frames, int B, int T, int D, double* sums,
                               void* stream) {
  SRF_REQUIRE(B >= 1 && T >= 0 && D >= 1 && D <= 65535, "fbank_stats: need B >= 1, T >= 0, 1 <= D <= 65535 (B=%d T=%d D=%d)",
              B, T, D);
  SRF_REQUIRE(n_frames && sums && (T == 0 || feats), "fbank_stats: null pointer argument");
  if (T == 0) return SRF_OK;
  hipLaunchKernelGGL(fbank_stats_kernel, dim3((unsigned)D), dim3(kStatThreads), 0, static_cast<hipStream_t>(stream),
                     feats, n_frames, B, T, D, sums);
  SRF_LAUNCH_CHECK("fbank_stats");
  return SRF_OK;
}
