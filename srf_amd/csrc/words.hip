// Words of a CTC character output on the device: segmentation of a label row at a
// separator (srf_word_split), exact word identity and the word-level edit alignment
// (srf_word_align), the step from the character error rate to the word error rate.
// One workgroup of 256 lanes per utterance.
//   classify  tiles of 256 positions: separator (the raw label, before the fold), dropped
//             by the fold, or kept with class fold[x]
//   segment   a kept label starts a word when no kept label lies between it and the last
//             separator.  Per wave two ballots (kept, separator) give every lane its
//             predecessors by mask arithmetic; what crosses a wave's edge is three values
//             (a word is open, kept labels so far, the last kept position) handed over
//             through LDS and carried from tile to tile in registers.  A word's end is the
//             last kept position before the next word's start, so nothing looks ahead.
//   table     (srf_word_align) kept classes compacted, per word its first compacted index,
//             length and a 32-bit hash: the sum over its labels of mix(class, index in the
//             word), added with atomicAdd, so it does not depend on the order
//   ids       reference words then hypothesis words form one list; lane t looks for the
//             first word u < t with the same hash and length and compares the labels: the
//             hash only filters, the labels decide.  Quadratic in the word count at worst.
// srf_word_align then runs srf_edit_align (score.hip) on the two id rows from the same C
// entry: the sweep, its back-pointers, spill paths and tie rule exist once.
// The table lies in LDS when it fits the 96 KiB budget, in the caller's workspace otherwise.
#include "srf_common.h"
#include "../../include/srf.h"

namespace {

constexpr size_t kWordsLds = 96 * 1024;
constexpr int kWordsMax = 8192;
constexpr int kWMisc = 16;   // ints of LDS in front of everything else

// misc[]: per wave of the tile, 0 .. 3 flags (1: holds a separator, 2: kept labels after
// its last separator, or any without one), 4 .. 7 kept labels, 8 .. 11 last kept position
// (-1 none), 12 .. 15 word starts.
enum { W_FLAG = 0, W_KEPT = 4, W_LAST = 8, W_START = 12 };

__host__ __device__ inline int word_cap(int n) { return (n + 1) / 2; }

// Per utterance: cls[Rmax + Hmax] | k0[WT] | len[WT] | hash[WT], WT the two word capacities.
__host__ __device__ inline size_t word_table_bytes(int Hmax, int Rmax) {
  const size_t wt = (size_t)word_cap(Hmax) + word_cap(Rmax);
  return (((size_t)Hmax + Rmax + 3 * wt) * 4 + 15) & ~(size_t)15;
}

struct Table {
  int *cls, *k0, *len;
  unsigned* hash;
};

__device__ __forceinline__ unsigned word_mix(int c, int idx) {
  unsigned h = (unsigned)c * 0x9E3779B1u ^ (unsigned)idx * 0x85EBCA6Bu;
  h ^= h >> 15;
  h *= 0x2C1B3C6Du;
  h ^= h >> 12;
  return h;
}

// TABLE_LDS = false: the table lies in the workspace and a hand-over between lanes needs a
// device fence before the barrier.
template <bool TABLE_LDS>
__device__ __forceinline__ void table_hand_over() {
  if constexpr (!TABLE_LDS) __threadfence();
  __syncthreads();
}

// Segments src[0 .. n) (n uniform; entries past n are not read) by the whole workgroup.
// Words are numbered from w0 and their kept labels from k0: out_start / out_end (either
// may be NULL) are indexed by the word's number minus w0.  TABLE: also the compacted
// classes, each word's first compacted index and its hash (zeroed by the caller).
// Returns the number of words; k_end is the compacted index after the last kept label.
template <bool TABLE, bool TABLE_LDS>
__device__ __forceinline__ int segment_words(const int* __restrict__ src, int n, const int* __restrict__ fold,
                                             int n_fold, int sep, int* __restrict__ misc, int* __restrict__ out_start,
                                             int* __restrict__ out_end, const Table& tb, int k0, int w0, int& k_end) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long below = (1ull << lane) - 1;
  int open = 0, kbase = k0, wbase = w0, lastk = -1;   // uniform carries from tile to tile
  for (int p0 = 0; p0 < n; p0 += 256) {
    const int p = p0 + threadIdx.x;
    const bool in = p < n;
    const int x = in ? src[p] : 0;
    const bool is_sep = in && x == sep;
    bool kept = in && !is_sep;
    int c = x;
    if (fold && kept) {
      kept = x >= 0 && x < n_fold;
      if (kept) {
        c = fold[x];
        kept = c >= 0;
      }
    }
    const unsigned long long K = __ballot(kept), S = __ballot(is_sep);
    if (lane == 0) {
      const int top = S ? 63 - __clzll(S) : -1;
      const unsigned long long after = top >= 63 ? 0ull : K >> (top + 1);
      misc[W_FLAG + wave] = (S ? 1 : 0) | (after ? 2 : 0);
      misc[W_KEPT + wave] = __popcll(K);
      misc[W_LAST + wave] = K ? p0 + wave * 64 + 63 - __clzll(K) : -1;
    }
    __syncthreads();
    int open_in = 0, k_in = 0, last_in = -1;   // the state at this wave's first lane
    int o = open, kk = kbase, ll = lastk;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      if (w == wave) open_in = o, k_in = kk, last_in = ll;
      const int f = misc[W_FLAG + w], l = misc[W_LAST + w];
      o = (f & 1) ? (f >> 1) : (o | (f >> 1));
      kk += misc[W_KEPT + w];
      ll = l >= 0 ? l : ll;
    }
    const unsigned long long lowK = K & below, lowS = S & below;
    bool open_before;
    if (lowS) {
      const int hs = 63 - __clzll(lowS);   // <= 62: a lane below this one
      open_before = (lowK >> (hs + 1)) != 0;
    } else {
      open_before = open_in || lowK != 0;
    }
    const bool start = kept && !open_before;
    const unsigned long long SM = __ballot(start);
    if (lane == 0) misc[W_START + wave] = __popcll(SM);
    __syncthreads();
    int wofs = wbase;
    for (int w = 0; w < wave; ++w) wofs += misc[W_START + w];
    const int wtile = misc[W_START] + misc[W_START + 1] + misc[W_START + 2] + misc[W_START + 3];
    const int k = k_in + __popcll(lowK);
    const int w = wofs + __popcll(SM & below) + (start ? 1 : 0) - 1;   // the word a kept label lies in
    if (kept) {
      if constexpr (TABLE) tb.cls[k] = c;
      if (start) {
        if (out_start) out_start[w - w0] = p;
        if constexpr (TABLE) tb.k0[w] = k;
        if (w > w0 && out_end) out_end[w - 1 - w0] = (lowK ? p0 + wave * 64 + 63 - __clzll(lowK) : last_in) + 1;
      }
    }
    if constexpr (TABLE) {
      table_hand_over<TABLE_LDS>();   // k0 of a word that another lane of this tile started
      if (kept) atomicAdd(&tb.hash[w], word_mix(c, k - tb.k0[w]));
    }
    open = o, kbase = kk, lastk = ll, wbase += wtile;
    __syncthreads();   // misc is written again by the next tile
  }
  k_end = kbase;
  const int W = wbase - w0;
  if (threadIdx.x == 0 && W > 0 && out_end) out_end[W - 1] = lastk + 1;
  return W;
}

template <bool TABLE_LDS>
__device__ __forceinline__ void word_lengths(const Table& tb, int w0, int W, int k_end) {
  table_hand_over<TABLE_LDS>();
  for (int w = w0 + threadIdx.x; w < w0 + W; w += 256) tb.len[w] = (w + 1 < w0 + W ? tb.k0[w + 1] : k_end) - tb.k0[w];
}

struct SplitArgs {
  const int *labels, *label_len, *fold;
  int Lmax, n_fold, sep;
  int *word_start, *word_end, *word_count;
  const int *tok_start, *tok_end;
  const float* tok_logp;
  int *frame_start, *frame_end;
  float* word_logp;
};

__global__ __launch_bounds__(256) void word_split_kernel(const SplitArgs a) {
  __shared__ int misc[kWMisc];
  const int b = blockIdx.x, cap = word_cap(a.Lmax);
  const int n = max(0, min(a.label_len[b], a.Lmax));
  int* ws = a.word_start + (size_t)b * cap;
  int* we = a.word_end + (size_t)b * cap;
  const Table none = {nullptr, nullptr, nullptr, nullptr};
  int k_end;
  const int W = segment_words<false, true>(a.labels + (size_t)b * a.Lmax, n, a.fold, a.n_fold, a.sep, misc, ws, we,
                                           none, 0, 0, k_end);
  for (int w = W + threadIdx.x; w < cap; w += 256) ws[w] = we[w] = -1;
  if (threadIdx.x == 0) a.word_count[b] = W;
  if (!a.tok_start) return;
  __threadfence();   // a word's lane reads the start and end that other lanes stored
  __syncthreads();
  const size_t row = (size_t)b * a.Lmax;
  for (int w = threadIdx.x; w < cap; w += 256) {
    int fs = -1, fe = -1;
    float lp = 0.f;
    if (w < W) {
      const int s = ws[w], e = we[w];
      const int ts = a.tok_start[row + s];
      if (ts >= 0) {   // -1: an infeasible utterance
        fs = ts;
        fe = a.tok_end[row + e - 1];
        for (int p = s; p < e; ++p) lp += a.tok_logp[row + p];
      }
    }
    a.frame_start[(size_t)b * cap + w] = fs;
    a.frame_end[(size_t)b * cap + w] = fe;
    a.word_logp[(size_t)b * cap + w] = lp;
  }
}

struct WordAlignArgs {
  const int *hyp, *hyp_len, *ref, *ref_len, *fold;
  int Hmax, Rmax, n_fold, sep;
  int *hyp_word_start, *hyp_word_end, *hyp_word_id, *ref_word_start, *ref_word_end, *ref_word_id;
  int *ids_h, *ids_r, *cnt_h, *cnt_r;   // workspace: the operands of the edit alignment
  char* tables;
  size_t table_bytes;
};

// Dynamic LDS: misc[16] | the table (TABLE_LDS).
template <bool TABLE_LDS>
__global__ __launch_bounds__(256) void word_ids_kernel(const WordAlignArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  int* misc = reinterpret_cast<int*>(smem_raw);
  const int b = blockIdx.x, tid = threadIdx.x;
  const int WH = word_cap(a.Hmax), WR = word_cap(a.Rmax), WT = WH + WR;
  char* base = TABLE_LDS ? smem_raw + kWMisc * sizeof(int) : a.tables + (size_t)b * a.table_bytes;
  Table tb;
  tb.cls = reinterpret_cast<int*>(base);
  tb.k0 = tb.cls + a.Hmax + a.Rmax;
  tb.len = tb.k0 + WT;
  tb.hash = reinterpret_cast<unsigned*>(tb.len + WT);
  for (int w = tid; w < WT; w += 256) tb.hash[w] = 0u;
  table_hand_over<TABLE_LDS>();
  const int Hb = max(0, min(a.hyp_len[b], a.Hmax)), Rb = max(0, min(a.ref_len[b], a.Rmax));
  int* rs = a.ref_word_start ? a.ref_word_start + (size_t)b * WR : nullptr;
  int* re = a.ref_word_end ? a.ref_word_end + (size_t)b * WR : nullptr;
  int* hs = a.hyp_word_start ? a.hyp_word_start + (size_t)b * WH : nullptr;
  int* he = a.hyp_word_end ? a.hyp_word_end + (size_t)b * WH : nullptr;
  int kr, kh;
  const int R = segment_words<true, TABLE_LDS>(a.ref + (size_t)b * a.Rmax, Rb, a.fold, a.n_fold, a.sep, misc, rs, re, tb,
                                               0, 0, kr);
  word_lengths<TABLE_LDS>(tb, 0, R, kr);
  const int H = segment_words<true, TABLE_LDS>(a.hyp + (size_t)b * a.Hmax, Hb, a.fold, a.n_fold, a.sep, misc, hs, he, tb,
                                               kr, R, kh);
  word_lengths<TABLE_LDS>(tb, R, H, kh);
  table_hand_over<TABLE_LDS>();
  int* idr = a.ids_r + (size_t)b * WR;
  int* idh = a.ids_h + (size_t)b * WH;
  int* out_r = a.ref_word_id ? a.ref_word_id + (size_t)b * WR : nullptr;
  int* out_h = a.hyp_word_id ? a.hyp_word_id + (size_t)b * WH : nullptr;
  for (int t = tid; t < R + H; t += 256) {
    const unsigned ht = tb.hash[t];
    const int lt = tb.len[t], kt = tb.k0[t];
    int id = t;
    for (int u = 0; u < t; ++u) {
      if (tb.hash[u] != ht || tb.len[u] != lt) continue;
      const int ku = tb.k0[u];
      int q = 0;
      while (q < lt && tb.cls[ku + q] == tb.cls[kt + q]) ++q;
      if (q == lt) {
        id = u;
        break;
      }
    }
    if (t < R) {
      idr[t] = id;
      if (out_r) out_r[t] = id;
    } else {
      idh[t - R] = id;
      if (out_h) out_h[t - R] = id;
    }
  }
  for (int w = R + tid; w < WR; w += 256) {
    if (rs) rs[w] = -1;
    if (re) re[w] = -1;
    if (out_r) out_r[w] = -1;
  }
  for (int w = H + tid; w < WH; w += 256) {
    if (hs) hs[w] = -1;
    if (he) he[w] = -1;
    if (out_h) out_h[w] = -1;
  }
  if (tid == 0) {
    a.cnt_r[b] = R;
    a.cnt_h[b] = H;
  }
}

bool words_shape_ok(const char* what, int B, int Hmax, int Rmax) {
  if (B >= 1 && Hmax >= 0 && Hmax <= kWordsMax && Rmax >= 0 && Rmax <= kWordsMax) return true;
  srf::set_error("%s: bad shape (B=%d capacities %d, %d): B >= 1, 0 <= capacity <= %d", what, B, Hmax, Rmax,
                 kWordsMax);
  return false;
}

struct WordGeom {
  bool table_lds;
  size_t table, shmem, ids, tables, edit;   // bytes: per-utterance table, LDS, workspace parts
};

// The launch geometry and the workspace layout (ids | tables | edit alignment) of a call.
inline WordGeom word_geometry(int B, int Hmax, int Rmax) {
  WordGeom g;
  const size_t fixed = kWMisc * sizeof(int);
  g.table = word_table_bytes(Hmax, Rmax);
  g.table_lds = fixed + g.table <= kWordsLds;
  g.shmem = fixed + (g.table_lds ? g.table : 0);
  g.ids = (((size_t)B * (word_cap(Hmax) + word_cap(Rmax) + 2)) * 4 + 15) & ~(size_t)15;
  g.tables = g.table_lds ? 0 : (size_t)B * g.table;
  g.edit = srf_edit_align_workspace(B, word_cap(Hmax), word_cap(Rmax));
  return g;
}

}  // namespace

extern "C" {

size_t srf_word_split_workspace(int B, int Lmax) {
  if (!words_shape_ok("word_split", B, Lmax, 0)) return 0;
  return 16;   // everything fits the kernel's registers and LDS
}

int srf_word_split(const int* labels, const int* label_len, int Lmax, int B, const int* fold, int n_fold, int sep,
                   int* word_start, int* word_end, int* word_count, const int* tok_start, const int* tok_end,
                   const float* tok_logp, int* word_frame_start, int* word_frame_end, float* word_logp,
                   void* workspace, size_t workspace_bytes, void* stream) {
  if (!words_shape_ok("word_split", B, Lmax, 0)) return SRF_EINVAL;
  SRF_REQUIRE(label_len && word_count && workspace, "word_split: null pointer argument");
  SRF_REQUIRE((labels && word_start && word_end) || Lmax == 0, "word_split: null labels or word table with Lmax = %d",
              Lmax);
  SRF_REQUIRE(fold ? n_fold >= 0 : n_fold == 0, "word_split: n_fold = %d %s a fold table", n_fold,
              fold ? "with" : "without");
  const int n_tok = (tok_start != nullptr) + (tok_end != nullptr) + (tok_logp != nullptr);
  const int n_out = (word_frame_start != nullptr) + (word_frame_end != nullptr) + (word_logp != nullptr);
  SRF_REQUIRE(n_tok == 0 || n_tok == 3, "word_split: tok_start, tok_end and tok_logp come together or not at all");
  SRF_REQUIRE(Lmax == 0 || n_out == n_tok,
              "word_split: the frame outputs (start, end, logp) are all given with the tok inputs and all null without");
  SRF_REQUIRE((uintptr_t)workspace % 16 == 0, "word_split: the workspace must be 16-byte aligned");
  if (workspace_bytes < srf_word_split_workspace(B, Lmax)) {
    srf::set_error("word split workspace too small");
    return SRF_EWORKSPACE;
  }
  SplitArgs a;
  a.labels = labels, a.label_len = label_len, a.fold = fold;
  a.Lmax = Lmax, a.n_fold = n_fold, a.sep = sep;
  a.word_start = word_start, a.word_end = word_end, a.word_count = word_count;
  const bool frames = n_tok == 3 && n_out == 3;
  a.tok_start = frames ? tok_start : nullptr, a.tok_end = tok_end, a.tok_logp = tok_logp;
  a.frame_start = word_frame_start, a.frame_end = word_frame_end, a.word_logp = word_logp;
  hipLaunchKernelGGL(word_split_kernel, dim3(B), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  SRF_LAUNCH_CHECK("word_split");
  return SRF_OK;
}

size_t srf_word_align_workspace(int B, int Hmax, int Rmax) {
  if (!words_shape_ok("word_align", B, Hmax, Rmax)) return 0;
  const WordGeom g = word_geometry(B, Hmax, Rmax);
  return g.ids + g.tables + g.edit;
}

int srf_word_align(const int* hyp, const int* hyp_len, int Hmax, const int* ref, const int* ref_len, int Rmax, int B,
                   const int* fold, int n_fold, int sep, int* counts, int* hyp_word_start, int* hyp_word_end,
                   int* hyp_word_id, int* ref_word_start, int* ref_word_end, int* ref_word_id, int* hyp_to_ref,
                   int* ref_to_hyp, long long* totals, void* workspace, size_t workspace_bytes, void* stream) {
  if (!words_shape_ok("word_align", B, Hmax, Rmax)) return SRF_EINVAL;
  SRF_REQUIRE(hyp_len && ref_len && counts && workspace, "word_align: null pointer argument");
  SRF_REQUIRE((hyp || Hmax == 0) && (ref || Rmax == 0), "word_align: null labels with Hmax = %d, Rmax = %d", Hmax,
              Rmax);
  SRF_REQUIRE(fold ? n_fold >= 0 : n_fold == 0, "word_align: n_fold = %d %s a fold table", n_fold,
              fold ? "with" : "without");
  SRF_REQUIRE((uintptr_t)workspace % 16 == 0, "word_align: the workspace must be 16-byte aligned");
  const WordGeom g = word_geometry(B, Hmax, Rmax);
  if (workspace_bytes < g.ids + g.tables + g.edit) {
    srf::set_error("word alignment workspace too small");
    return SRF_EWORKSPACE;
  }
  const int WH = word_cap(Hmax), WR = word_cap(Rmax);
  char* ws = static_cast<char*>(workspace);
  WordAlignArgs a;
  a.hyp = hyp, a.hyp_len = hyp_len, a.ref = ref, a.ref_len = ref_len, a.fold = fold;
  a.Hmax = Hmax, a.Rmax = Rmax, a.n_fold = n_fold, a.sep = sep;
  a.hyp_word_start = hyp_word_start, a.hyp_word_end = hyp_word_end, a.hyp_word_id = hyp_word_id;
  a.ref_word_start = ref_word_start, a.ref_word_end = ref_word_end, a.ref_word_id = ref_word_id;
  a.ids_h = reinterpret_cast<int*>(ws);
  a.ids_r = a.ids_h + (size_t)B * WH;
  a.cnt_h = a.ids_r + (size_t)B * WR;
  a.cnt_r = a.cnt_h + B;
  a.tables = ws + g.ids;
  a.table_bytes = g.table;
  const auto kern = g.table_lds ? word_ids_kernel<true> : word_ids_kernel<false>;
  if (g.shmem > 64 * 1024)
    SRF_HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.shmem));
  hipLaunchKernelGGL(kern, dim3(B), dim3(256), g.shmem, static_cast<hipStream_t>(stream), a);
  SRF_LAUNCH_CHECK("word_align");
  // the word ids are labels of their own: the character alignment's sweep, backtrace and
  // tie rule, over word indices
  return srf_edit_align(a.ids_h, a.cnt_h, WH, a.ids_r, a.cnt_r, WR, B, nullptr, 0, counts, hyp_to_ref, ref_to_hyp,
                        totals, nullptr, 0, ws + g.ids + g.tables, g.edit, stream);
}

}  // extern "C"
