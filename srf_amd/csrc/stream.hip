// Chunked streaming inference (srf_amd/streaming.py): the two device steps a chunk
// needs besides the model's own kernels.
//
// srf_ctc_greedy_n: incremental best-path decoding (arg-max per frame, merge repeats,
// drop blanks; ctc.greedy_decode on the host) of the frames a chunk added, carrying the
// last frame's arg-max across chunk edges, so that a chunk's hypothesis needs no copy of
// its logits to the host.  srf_ctc_greedy_frames_n is the same launch with one more
// output: the frame at which each label was emitted.
//
// srf_stream_advance_n: the sliding state buffers of every stage move their kept tail
// to the front, all buffers of all streams in one launch.
#include "srf_common.h"
#include "../../include/srf.h"

namespace {

// One wave per stream.  Lane l scans classes l, l + 64, ... in ascending order and keeps
// the first maximum; the butterfly keeps the larger value and, on equal values, the lower
// class index -- torch.argmax's choice.  After it every lane holds the frame's arg-max;
// lane 0 runs the collapse.
__global__ __launch_bounds__(64) void ctc_greedy_kernel(const float* __restrict__ logits,
                                                        const int* __restrict__ n_valid, int n, int C, int blank,
                                                        int frame0, int* __restrict__ prev,
                                                        int* __restrict__ labels, int* __restrict__ frames,
                                                        int* __restrict__ count) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int nv = max(0, min(n_valid[b], n));
  const float* x = logits + (size_t)b * n * C;
  int* out = labels + (size_t)b * n;
  int* fout = frames ? frames + (size_t)b * n : nullptr;   // srf_ctc_greedy_frames_n only
  int last = prev[b], cnt = 0;
  for (int f = 0; f < nv; ++f) {
    const float* row = x + (size_t)f * C;
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
    if (lane == 0 && arg != last && arg != blank) {
      if (fout) fout[cnt] = frame0 + f;   // the first frame of the label's arg-max run
      out[cnt++] = arg;
    }
    last = arg;
  }
  if (lane == 0) {
    prev[b] = last;
    count[b] = cnt;
  }
}

struct AdvanceBuf {
  char* ptr;
  unsigned long long row_bytes;
  int rows_per_stream, shift, keep;
};
struct AdvanceArgs {
  AdvanceBuf buf[SRF_STREAM_ADVANCE_MAX];
};

constexpr int kAdvThreads = 256;
constexpr int kAdvUnroll = 4;

// dst[0, n) = src[0, n) in elements of type V with dst < src, possibly overlapping, by one
// workgroup.  Tiles are walked in ascending order.  A tile is read whole into registers,
// the loads are waited for (a plain load may still be in flight across a barrier) and the
// workgroup passes a barrier before any lane stores: a store of tile k lands below
// src + (k + 1) * tile, where no later tile reads, and inside tile k only once every
// lane holds its elements.
template <typename V>
__device__ __forceinline__ void move_down(V* __restrict__ dst, const V* __restrict__ src, size_t n) {
  constexpr size_t kTile = (size_t)kAdvThreads * kAdvUnroll;
  for (size_t base = 0; base < n; base += kTile) {
    V r[kAdvUnroll];
    if (base + kTile <= n) {   // whole tile: the loads issue back to back
#pragma unroll
      for (int u = 0; u < kAdvUnroll; ++u) r[u] = src[base + (size_t)u * kAdvThreads + threadIdx.x];
    } else {
#pragma unroll
      for (int u = 0; u < kAdvUnroll; ++u) {
        const size_t i = base + (size_t)u * kAdvThreads + threadIdx.x;
        if (i < n) r[u] = src[i];
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kAdvUnroll; ++u) {
      const size_t i = base + (size_t)u * kAdvThreads + threadIdx.x;
      if (i < n) dst[i] = r[u];
    }
  }
}

// One workgroup per (buffer, stream): rows [shift, shift + keep) of the stream's
// [rows_per_stream][row_bytes] block move to rows [0, keep).  16-byte elements where the
// block's address, the distance and the length allow, else 4-byte, else bytes.
__global__ __launch_bounds__(kAdvThreads) void stream_advance_kernel(const AdvanceArgs args) {
  const AdvanceBuf d = args.buf[blockIdx.x];
  if (d.shift <= 0 || d.keep <= 0) return;
  char* dst = d.ptr + (size_t)blockIdx.y * d.rows_per_stream * d.row_bytes;
  const size_t delta = (size_t)d.shift * d.row_bytes, bytes = (size_t)d.keep * d.row_bytes;
  const size_t bits = (size_t)(uintptr_t)dst | delta | bytes;
  if (bits % 16 == 0)
    move_down(reinterpret_cast<uint4*>(dst), reinterpret_cast<const uint4*>(dst + delta), bytes / 16);
  else if (bits % 4 == 0)
    move_down(reinterpret_cast<unsigned*>(dst), reinterpret_cast<const unsigned*>(dst + delta), bytes / 4);
  else
    move_down(reinterpret_cast<unsigned char*>(dst), reinterpret_cast<const unsigned char*>(dst + delta), bytes);
}

}  // namespace

extern "C" int srf_ctc_greedy_n(const float* logits, const int* n_valid, int B, int n, int C, int blank, int* prev,
                                int* labels, int* count, void* stream) {
  SRF_REQUIRE(B >= 1 && n >= 0 && C >= 2, "ctc_greedy: need B >= 1, n >= 0, C >= 2 (B=%d n=%d C=%d)", B, n, C);
  SRF_REQUIRE(n_valid && prev && count, "ctc_greedy: null pointer argument");
  SRF_REQUIRE(n == 0 || (logits && labels), "ctc_greedy: null logits / labels with n = %d", n);
  hipLaunchKernelGGL(ctc_greedy_kernel, dim3((unsigned)B), dim3(64), 0, static_cast<hipStream_t>(stream), logits,
                     n_valid, n, C, blank, 0, prev, labels, static_cast<int*>(nullptr), count);
  SRF_LAUNCH_CHECK("ctc_greedy");
  return SRF_OK;
}

extern "C" int srf_ctc_greedy_frames_n(const float* logits, const int* n_valid, int B, int n, int C, int blank,
                                       int frame0, int* prev, int* labels, int* frames, int* count, void* stream) {
  SRF_REQUIRE(B >= 1 && n >= 0 && C >= 2, "ctc_greedy_frames: need B >= 1, n >= 0, C >= 2 (B=%d n=%d C=%d)", B, n, C);
  SRF_REQUIRE(n_valid && prev && count, "ctc_greedy_frames: null pointer argument");
  SRF_REQUIRE(n == 0 || (logits && labels && frames), "ctc_greedy_frames: null logits / labels / frames with n = %d",
              n);
  hipLaunchKernelGGL(ctc_greedy_kernel, dim3((unsigned)B), dim3(64), 0, static_cast<hipStream_t>(stream), logits,
                     n_valid, n, C, blank, frame0, prev, labels, frames, count);
  SRF_LAUNCH_CHECK("ctc_greedy_frames");
  return SRF_OK;
}

extern "C" int srf_stream_advance_n(const srf_stream_buf* bufs, int n_bufs, int B, void* stream) {
  SRF_REQUIRE(bufs && n_bufs >= 1 && n_bufs <= SRF_STREAM_ADVANCE_MAX && B >= 1,
              "stream_advance: 1 .. %d buffers and B >= 1 (n_bufs=%d B=%d)", SRF_STREAM_ADVANCE_MAX, n_bufs, B);
  AdvanceArgs args;
  bool any = false;
  for (int i = 0; i < n_bufs; ++i) {
    const srf_stream_buf& s = bufs[i];
    SRF_REQUIRE(s.ptr && s.row_bytes >= 1 && s.rows_per_stream >= 1, "stream_advance: buffer %d is empty", i);
    SRF_REQUIRE(s.shift >= 0 && s.keep >= 0 && (long long)s.shift + s.keep <= s.rows_per_stream,
                "stream_advance: buffer %d moves rows [%d, %d + %d) of %d", i, s.shift, s.shift, s.keep,
                s.rows_per_stream);
    args.buf[i] = AdvanceBuf{static_cast<char*>(s.ptr), (unsigned long long)s.row_bytes, s.rows_per_stream, s.shift,
                             s.keep};
    any = any || (s.shift > 0 && s.keep > 0);
  }
  for (int i = n_bufs; i < SRF_STREAM_ADVANCE_MAX; ++i) args.buf[i] = AdvanceBuf{nullptr, 0, 0, 0, 0};
  if (!any) return SRF_OK;
  hipLaunchKernelGGL(stream_advance_kernel, dim3((unsigned)n_bufs, (unsigned)B), dim3(kAdvThreads), 0,
                     static_cast<hipStream_t>(stream), args);
  SRF_LAUNCH_CHECK("stream_advance");
  return SRF_OK;
}
