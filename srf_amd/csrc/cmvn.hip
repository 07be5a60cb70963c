// Online CMVN (srf_amd/fbank.py SlidingCmvn): every frame is
// normalised with the mean and the deviation of the W frames that end with it, topped up
// by a prior while the window fills.  All arithmetic is fp64 with one rounding to fp32.
//
// srf_cmvn_sliding: one workgroup per (tile of kTile absolute frames, stream), one thread
// per dimension, so a row's loads and stores are coalesced.  A thread sums its column over
// the window of the tile's first frame in ascending frame order, then slides the two sums
// frame by frame, "- x[t - W]" before "+ x[t]".  The order of every addition is a function
// of absolute frame indices alone: a launch that starts inside a tile recomputes from the
// tile's first frame and stores only its own range, so the bits of a frame do not depend
// on the launch, the batch or the chunking, and the rounding error of a sum is that of at
// most W + 2 kTile additions however long the stream is.  No LDS, no atomics, nothing is
// read back.
#include "srf_common.h"
#include "../../include/srf.h"

namespace {

constexpr int kTile = SRF_CMVN_TILE, kThreads = SRF_CMVN_MAX_DIM;
constexpr int kMaxFrames = 0x7fffffff - 2 * kTile;
constexpr int kBatch = 16;   // rows in flight per thread

__global__ __launch_bounds__(kThreads) void cmvn_sliding_kernel(
    const float* __restrict__ x, const int* __restrict__ n_frames, int rows, int D, int f0, int t0, int t1,
    const double* __restrict__ pmean, const double* __restrict__ pstd, const double* __restrict__ pcount,
    int prior_rows, int W, int norm_vars, float* __restrict__ out, int To, int o0, double* __restrict__ last) {
  const int d = threadIdx.x, b = blockIdx.y;
  if (d >= D) return;
  const int ts = (t0 / kTile + (int)blockIdx.x) * kTile;        // the tile's first frame
  const int w0 = max(ts, t0), w1 = min(ts + kTile, t1);         // the frames this workgroup stores
  const int Tb = max(n_frames[b], 0);
  const int e = min(Tb, w1);                                    // frames [w0, e) are normalised, [e, w1) zero
  const float* xb = x + (size_t)b * rows * D + d;
  float* ob = out + (size_t)b * To * D + d;
  if (w0 < e) {
    double pm = 0.0, pq = 0.0, pc = 0.0;
    if (prior_rows) {
      const size_t p = prior_rows > 1 ? (size_t)b : 0;
      const double sd = pstd[p * D + d];
      pm = pmean[p * D + d];
      pq = sd * sd + pm * pm;
      pc = pcount[p];
    }
    const int last_t = min(Tb, t1) - 1;                         // the launch's last frame of this stream
    double s1 = 0.0, s2 = 0.0, v = 0.0;
    // frame t from the sums of its window and v = x[t]
    auto emit = [&](int t) {
      const double n = (double)min(t + 1, W);
      const double c = fmin((double)W - n, pc);
      const double m = (s1 + c * pm) / (n + c), q = (s2 + c * pq) / (n + c);
      double y = v - m;
      if (norm_vars) y /= sqrt(fmax(q - m * m, 1e-10));
      ob[(size_t)(t - o0) * D] = (float)y;
      if (last && t == last_t) {
        double* l = last + (size_t)b * (2 * D + 1);
        l[d] = m;
        l[D + d] = q;
        if (d == 0) l[2 * D] = n + c;
      }
    };
    // Both loops load kBatch rows into registers before they add them, in frame order: the
    // additions wait for one round trip to memory per batch, not per frame.
    float nw[kBatch], od[kBatch];
    int u = max(ts - W + 1, 0);
    for (; u + kBatch <= ts + 1; u += kBatch) {
#pragma unroll
      for (int j = 0; j < kBatch; ++j) nw[j] = xb[(size_t)(u + j - f0) * D];
#pragma unroll
      for (int j = 0; j < kBatch; ++j) {
        v = (double)nw[j];
        s1 += v;
        s2 += v * v;
      }
    }
    for (; u <= ts; ++u) {
      v = (double)xb[(size_t)(u - f0) * D];
      s1 += v;
      s2 += v * v;
    }
    if (ts >= w0) emit(ts);
    for (int t = ts + 1; t < e; t += kBatch) {
#pragma unroll
      for (int j = 0; j < kBatch; ++j) {
        const int tt = min(t + j, e - 1);                       // past e: a frame the buffer holds, not used
        nw[j] = xb[(size_t)(tt - f0) * D];
        od[j] = xb[(size_t)((tt >= W ? tt - W : tt) - f0) * D];  // below W nothing leaves the window
      }
#pragma unroll
      for (int j = 0; j < kBatch; ++j) {
        const int tt = t + j;
        if (tt < e) {
          if (tt >= W) {
            const double old = (double)od[j];
            s1 -= old;
            s2 -= old * old;
          }
          v = (double)nw[j];
          s1 += v;
          s2 += v * v;
          if (tt >= w0) emit(tt);
        }
      }
    }
  }
  for (int t = max(w0, e); t < w1; ++t) ob[(size_t)(t - o0) * D] = 0.f;
}

}  // namespace

extern "C" int srf_cmvn_sliding(const float* feats, const int* n_frames, int B, int rows, int D, int f0, int t0, int t1,
                                const double* prior_mean, const double* prior_std, const double* prior_count,
                                int prior_rows, int window, int norm_vars, float* out, int To, int o0, double* last,
                                void* stream) {
  SRF_REQUIRE(B >= 1 && B <= 65535, "cmvn_sliding: need 1 <= B <= 65535 (B=%d)", B);
  SRF_REQUIRE(D >= 1 && D <= SRF_CMVN_MAX_DIM, "cmvn_sliding: need 1 <= D <= %d (D=%d)", SRF_CMVN_MAX_DIM, D);
  SRF_REQUIRE(window >= 1 && window <= SRF_CMVN_MAX_WINDOW, "cmvn_sliding: need 1 <= window <= %d (window=%d)",
              SRF_CMVN_MAX_WINDOW, window);
  SRF_REQUIRE(0 <= t0 && t0 <= t1 && t1 <= kMaxFrames, "cmvn_sliding: bad frame range [%d, %d)", t0, t1);
  SRF_REQUIRE(prior_rows == 0 || prior_rows == 1 || prior_rows == B,
              "cmvn_sliding: prior_rows is 0 (none), 1 (shared) or B (per stream), got %d", prior_rows);
  if (t1 == t0) return SRF_OK;
  SRF_REQUIRE(feats && n_frames && out && (prior_rows == 0 || (prior_mean && prior_std && prior_count)),
              "cmvn_sliding: null pointer argument");
  SRF_REQUIRE(To >= 1 && t0 >= o0 && (long long)t1 - o0 <= To,
              "cmvn_sliding: frames [%d, %d) outside the output buffer (frames %d .. %lld)", t0, t1, o0,
              (long long)o0 + To);
  // frames read: from the window of the first tile's first frame to t1 - 1
  const int ts = t0 / kTile * kTile, lo = ts - window + 1 > 0 ? ts - window + 1 : 0;
  SRF_REQUIRE(rows >= 1 && f0 >= 0 && lo >= f0 && (long long)t1 - f0 <= rows,
              "cmvn_sliding: input frames [%d, %d) outside the input buffer (frames %d .. %lld)", lo, t1, f0,
              (long long)f0 + rows);
  const unsigned gx = (unsigned)((t1 - 1) / kTile - t0 / kTile + 1);
  hipLaunchKernelGGL(cmvn_sliding_kernel, dim3(gx, (unsigned)B), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                     feats, n_frames, rows, D, f0, t0, t1, prior_mean, prior_std, prior_count, prior_rows, window,
                     norm_vars, out, To, o0, last);
  SRF_LAUNCH_CHECK("cmvn_sliding");
  return SRF_OK;
}
