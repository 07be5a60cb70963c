// Scoring of hypotheses against references: batched Levenshtein alignment with a
// backtrace (srf_edit_align), the integer min-plus sibling of ctc_align.hip's Viterbi.
// One workgroup per utterance:
//   fold     x -> fold[x]; dropped when fold[x] < 0 or x outside [0, n_fold); both
//            sequences compacted, the original position of every kept label kept
//   D[i][j]  = min(D[i-1][j-1] + (h[i-1] != r[j-1]), D[i][j-1] + 1, D[i-1][j] + 1),
//            D[i][0] = i, D[0][j] = j
//   ties     the diagonal before the deletion (i, j-1) before the insertion (i-1, j)
// The backtrace from (H, R) takes the recorded choice of every cell, so it is the first
// step of that order that is consistent with D.
//
// Wave 0 sweeps the anti-diagonals with one lane per reference position (KM groups of 64
// in registers): at step d lane j-1 holds D[d-j][j]; its own previous value is the
// insertion predecessor, lane j-2's previous value (one DPP wave_shr:1, the lane at a
// 64-lane boundary fed by a readlane) the deletion predecessor, and the value shifted in
// at the step before is the diagonal.  Every lane packs its cells' two-bit choices, 16
// steps to a word, and stores the words to LDS (workspace when they do not fit).  Lane 0
// walks them back, then the workgroup writes the maps and counts and adds to the
// accumulators.  Rmax > 512: a workgroup loop over the anti-diagonals with two value
// rows in LDS and two bits per cell in the workspace.
#include "srf_common.h"
#include "../../include/srf.h"

namespace {

constexpr size_t kScoreLds = 96 * 1024;
constexpr int kScoreMax = 8192;
constexpr int kMisc = 16;   // ints of LDS in front of everything else

// misc[]: 0 distance, 1 substitutions, 2 matched pairs, 4 / 5 where the backtrace left
// the table (rows / columns still to go), 8 .. 11 the compaction's wave counts.
enum { M_DIST = 0, M_SUB = 1, M_PAIR = 2, M_IEND = 4, M_JEND = 5, M_SCAN = 8 };

struct EditArgs {
  const int *hyp, *hyp_len, *ref, *ref_len, *fold;
  int Hmax, Rmax, n_fold, K;
  int *counts, *hyp_to_ref, *ref_to_hyp;
  unsigned long long *totals, *confusion;
  char* ws;
  size_t ws_per_utt, head_bytes;
};

// Head, in LDS or in the utterance's workspace: hlab[Hmax] | hpos[Hmax] | hmap[Hmax] |
// rlab[Rmax] | rpos[Rmax] | rmap[Rmax] (int), padded to 16 bytes.
__host__ __device__ inline size_t edit_head_bytes(int Hmax, int Rmax) {
  return (3 * ((size_t)Hmax + Rmax) * 4 + 15) & ~(size_t)15;
}
// the wave sweep's back-pointer words: 16 steps per word, 64 KM lanes, Hmax + Rmax - 1 steps
__host__ __device__ inline size_t edit_bp_word_bytes(int Hmax, int Rmax, int KM) {
  const int steps = Hmax + Rmax - 1 > 0 ? Hmax + Rmax - 1 : 0;
  return (size_t)((steps + 15) / 16) * 64 * KM * 4;
}
// the workgroup loop's back-pointers: two bits per cell, four rows of the table to a byte
__host__ __device__ inline size_t edit_bp_loop_bytes(int Hmax, int Rmax) {
  return ((size_t)((Hmax + 3) / 4) * Rmax + 15) & ~(size_t)15;
}
__host__ __device__ inline size_t edit_rows_bytes(int Rmax) { return (2 * ((size_t)Rmax + 1) * 4 + 15) & ~(size_t)15; }

struct EditGeom {
  int KM;   // 0: the workgroup loop
  bool head_lds, bp_lds;
  size_t head, bp, shmem, ws_per_utt;
};

// The launch geometry of a call, from its capacities alone.
inline EditGeom edit_geometry(int Hmax, int Rmax) {
  EditGeom g;
  g.head = edit_head_bytes(Hmax, Rmax);
  const size_t fixed = kMisc * sizeof(int);
  if (Rmax > 512) {
    g.KM = 0;
    g.bp = edit_bp_loop_bytes(Hmax, Rmax);
    const size_t rows = edit_rows_bytes(Rmax);
    g.head_lds = fixed + rows + g.head <= kScoreLds;
    g.bp_lds = false;
    g.shmem = fixed + rows + (g.head_lds ? g.head : 0);
  } else {
    g.KM = Rmax <= 128 ? 2 : Rmax <= 256 ? 4 : 8;
    g.bp = edit_bp_word_bytes(Hmax, Rmax, g.KM);
    g.head_lds = fixed + g.head <= kScoreLds;
    g.bp_lds = g.head_lds && fixed + g.head + g.bp <= kScoreLds;
    g.shmem = fixed + (g.head_lds ? g.head : 0) + (g.bp_lds ? g.bp : 0);
  }
  g.ws_per_utt = (g.head_lds ? 0 : g.head) + (g.bp_lds ? 0 : g.bp);
  return g;
}

__device__ __forceinline__ int dpp_wave_shr1(int old, int src) {   // lane l <- src[l-1], lane 0 <- old
  return __builtin_amdgcn_update_dpp(old, src, 0x138, 0xF, 0xF, false);
}

struct Head {
  int *hlab, *hpos, *hmap, *rlab, *rpos, *rmap;
};
__device__ __forceinline__ Head make_head(char* base, int Hmax, int Rmax) {
  Head h;
  h.hlab = reinterpret_cast<int*>(base);
  h.hpos = h.hlab + Hmax;
  h.hmap = h.hpos + Hmax;
  h.rlab = h.hmap + Hmax;
  h.rpos = h.rlab + Rmax;
  h.rmap = h.rpos + Rmax;
  return h;
}

// Fold and compact src[0 .. n) into lab / pos in order, by the whole workgroup (256
// lanes; n is uniform); entries past n are not read.  Returns the number kept.
__device__ __forceinline__ int fold_compact(const int* __restrict__ src, int n, const int* __restrict__ fold,
                                            int n_fold, int* __restrict__ lab, int* __restrict__ pos,
                                            int* __restrict__ scan) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int base = 0;
  for (int p0 = 0; p0 < n; p0 += 256) {
    const int p = p0 + threadIdx.x;
    bool keep = p < n;
    int x = keep ? src[p] : 0;
    if (fold && keep) {
      keep = x >= 0 && x < n_fold;
      if (keep) {
        x = fold[x];
        keep = x >= 0;
      }
    }
    const unsigned long long mask = __ballot(keep);
    const int before = __popcll(mask & ((1ull << lane) - 1));
    if (lane == 0) scan[wave] = __popcll(mask);
    __syncthreads();
    int off = base;
    for (int w = 0; w < wave; ++w) off += scan[w];
    if (keep) {
      lab[off + before] = x;
      pos[off + before] = p;
    }
    base += scan[0] + scan[1] + scan[2] + scan[3];
    __syncthreads();
  }
  return base;
}

// The choice of one cell: the diagonal on ties, then the deletion, then the insertion.
__device__ __forceinline__ int min3_choice(int sub, int del, int ins, unsigned& code) {
  const bool c1 = del < sub;
  const int m1 = c1 ? del : sub;
  const bool c2 = ins < m1;
  code = c2 ? 2u : c1 ? 1u : 0u;
  return c2 ? ins : m1;
}

// Wave-resident sweep (R <= 64 * KM, H >= 1, R >= 1), called by wave 0.  Step t = 0 ..
// H + R - 2 computes the cells with i + j = t + 2; lane l holds column j = l + 1, whose
// cell at that step is row i = t + 1 - l.  Codes: 0 diagonal, 1 deletion, 2 insertion,
// the step's code at bits 2 * (15 - t % 16) of word bp[(t / 16) * 64 KM + l], stored after
// every 16th step and after the last.  A lane above its column's first row keeps
// D[0][j] = j; rows past H and columns past R carry values that no live cell reads (a
// cell only looks up and to the left).  Column R's lane writes D[H][R] to *dist.
template <int KM>
__device__ __forceinline__ void edit_wave(const int* __restrict__ hl, const int* __restrict__ rl, int H, int R,
                                          unsigned* __restrict__ bp, int* __restrict__ dist) {
  const int lane = threadIdx.x & 63;
  int v[KM], dg[KM], r[KM], hc[KM];
  unsigned hist[KM];
#pragma unroll
  for (int k = 0; k < KM; ++k) {
    const int l = lane + 64 * k;
    r[k] = rl[min(l, R - 1)];
    v[k] = l + 1;   // D[0][j]
    dg[k] = l;      // D[0][j-1]
    hc[k] = hl[min(max(-l, 0), H - 1)];
    hist[k] = 0;
  }
  const int n = H + R - 1;
  for (int t = 0; t < n; ++t) {
    int hn[KM], nv[KM];
#pragma unroll
    for (int k = 0; k < KM; ++k) hn[k] = hl[min(max(t + 1 - lane - 64 * k, 0), H - 1)];
#pragma unroll
    for (int k = 0; k < KM; ++k) {
      const int j = lane + 64 * k + 1;
      // column j - 1 at the step before: D[i][0] = i = t + 1 for the first lane
      const int feed = k > 0 ? __builtin_amdgcn_readlane(v[k - 1], 63) : t + 1;
      const int left = dpp_wave_shr1(feed, v[k]);
      unsigned code;
      const int m = min3_choice(dg[k] + (hc[k] != r[k] ? 1 : 0), left + 1, v[k] + 1, code);
      nv[k] = t + 2 > j ? m : j;   // above row 1 the lane keeps D[0][j]
      hist[k] = (hist[k] << 2) | code;
      dg[k] = left;
    }
    if ((t & 15) == 15 || t == n - 1) {
      const int sh = 2 * (15 - (t & 15));
#pragma unroll
      for (int k = 0; k < KM; ++k) bp[(size_t)(t >> 4) * (64 * KM) + lane + 64 * k] = hist[k] << sh;
    }
#pragma unroll
    for (int k = 0; k < KM; ++k) {
      v[k] = nv[k];
      hc[k] = hn[k];
    }
  }
#pragma unroll
  for (int k = 0; k < KM; ++k)
    if (lane + 64 * k == R - 1) *dist = v[k];
}

// The walk back from (H, R) by one lane, code(i, j) the recorded choice of cell (i, j),
// 1 <= i <= H, 1 <= j <= R.  Writes the partner (folded index, or -1) of every label it
// passes and leaves in misc where it reached the table's edge: the rows and columns
// still to go are insertions and deletions, filled in by the workgroup.
template <class Code>
__device__ __forceinline__ void walk_back(int H, int R, const Head& hd, int* __restrict__ misc, Code code) {
  int i = H, j = R;
  while (i > 0 && j > 0) {
    const unsigned c = code(i, j);
    if (c == 0) {
      hd.hmap[i - 1] = j - 1;
      hd.rmap[j - 1] = i - 1;
      --i;
      --j;
    } else if (c == 1) {
      hd.rmap[--j] = -1;
    } else {
      hd.hmap[--i] = -1;
    }
  }
  misc[M_IEND] = i;
  misc[M_JEND] = j;
}

// After the walk back and a barrier: the maps, the counts and the accumulators, by the
// whole workgroup.  HEADLDS = false: the head lies in the workspace and every hand-over
// between lanes needs a device fence before the barrier.
template <bool HEADLDS>
__device__ __forceinline__ void hand_over() {
  if constexpr (!HEADLDS) __threadfence();
  __syncthreads();
}

template <bool HEADLDS>
__device__ __forceinline__ void write_outputs(const EditArgs& a, int b, int H, int R, const Head& hd,
                                              int* __restrict__ misc) {
  const int tid = threadIdx.x, nt = blockDim.x;
  int* h2r = a.hyp_to_ref ? a.hyp_to_ref + (size_t)b * a.Hmax : nullptr;
  int* r2h = a.ref_to_hyp ? a.ref_to_hyp + (size_t)b * a.Rmax : nullptr;
  const int i_end = misc[M_IEND], j_end = misc[M_JEND];
  for (int i = tid; i < i_end; i += nt) hd.hmap[i] = -1;
  for (int j = tid; j < j_end; j += nt) hd.rmap[j] = -1;
  if (h2r)
    for (int p = tid; p < a.Hmax; p += nt) h2r[p] = -2;
  if (r2h)
    for (int p = tid; p < a.Rmax; p += nt) r2h[p] = -2;
  __threadfence();   // the -2 fill precedes the partners written below by other lanes
  __syncthreads();
  const int K = a.K;
  unsigned long long* conf = a.confusion;
  int n_sub = 0, n_pair = 0;
  for (int i = tid; i < H; i += nt) {
    const int m = hd.hmap[i], hc = hd.hlab[i];
    const bool h_in = hc >= 0 && hc < K;
    if (m < 0) {
      if (h2r) h2r[hd.hpos[i]] = -1;
      if (conf && h_in) atomicAdd(conf + (size_t)K * (K + 1) + hc, 1ull);
    } else {
      const int rc = hd.rlab[m];
      ++n_pair;
      n_sub += hc != rc;
      if (h2r) h2r[hd.hpos[i]] = hd.rpos[m];
      if (conf && h_in && rc >= 0 && rc < K) atomicAdd(conf + (size_t)rc * (K + 1) + hc, 1ull);
    }
  }
  for (int j = tid; j < R; j += nt) {
    const int m = hd.rmap[j];
    if (m < 0) {
      const int rc = hd.rlab[j];
      if (r2h) r2h[hd.rpos[j]] = -1;
      if (conf && rc >= 0 && rc < K) atomicAdd(conf + (size_t)rc * (K + 1) + K, 1ull);
    } else if (r2h) {
      r2h[hd.rpos[j]] = hd.hpos[m];
    }
  }
  if (n_sub) atomicAdd(&misc[M_SUB], n_sub);
  if (n_pair) atomicAdd(&misc[M_PAIR], n_pair);
  __syncthreads();
  if (tid == 0) {
    const int sub = misc[M_SUB], pair = misc[M_PAIR];
    const int c[6] = {misc[M_DIST], sub, R - pair, H - pair, R, H};
#pragma unroll
    for (int q = 0; q < 6; ++q) a.counts[(size_t)b * 6 + q] = c[q];
    if (a.totals) {
#pragma unroll
      for (int q = 0; q < 6; ++q)
        if (c[q]) atomicAdd(a.totals + q, (unsigned long long)c[q]);
      atomicAdd(a.totals + 6, 1ull);
      if (c[0] > 0) atomicAdd(a.totals + 7, 1ull);
    }
  }
}

// Lengths, head pointers and the two folded sequences; returns H and R after the fold.
template <bool HEADLDS>
__device__ __forceinline__ Head load_phase(const EditArgs& a, int b, char* lds_head, char* wsb, int* misc, int& H,
                                           int& R) {
  const Head hd = make_head(HEADLDS ? lds_head : wsb, a.Hmax, a.Rmax);
  if (threadIdx.x < kMisc) misc[threadIdx.x] = 0;
  __syncthreads();
  const int Hb = max(0, min(a.hyp_len[b], a.Hmax)), Rb = max(0, min(a.ref_len[b], a.Rmax));
  H = fold_compact(a.hyp + (size_t)b * a.Hmax, Hb, a.fold, a.n_fold, hd.hlab, hd.hpos, misc + M_SCAN);
  R = fold_compact(a.ref + (size_t)b * a.Rmax, Rb, a.fold, a.n_fold, hd.rlab, hd.rpos, misc + M_SCAN);
  hand_over<HEADLDS>();
  return hd;
}

// Dynamic LDS: misc[16] | head (HEADLDS) | back-pointer words (BPLDS).
template <int KM, bool HEADLDS, bool BPLDS>
__global__ __launch_bounds__(256) void edit_align_kernel(const EditArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  int* misc = reinterpret_cast<int*>(smem_raw);
  char* lds_head = smem_raw + kMisc * sizeof(int);
  const int b = blockIdx.x;
  char* wsb = a.ws + (size_t)b * a.ws_per_utt;
  int H, R;
  const Head hd = load_phase<HEADLDS>(a, b, lds_head, wsb, misc, H, R);
  unsigned* bp = reinterpret_cast<unsigned*>(BPLDS ? lds_head + a.head_bytes : wsb + (HEADLDS ? 0 : a.head_bytes));
  if (threadIdx.x < 64) {
    if (H > 0 && R > 0) {
      edit_wave<KM>(hd.hlab, hd.rlab, H, R, bp, &misc[M_DIST]);
      if constexpr (!BPLDS) __threadfence();   // lane 0 reads what every lane stored
    }
    if (threadIdx.x == 0) {
      if (H == 0 || R == 0) misc[M_DIST] = max(H, R);
      walk_back(H, R, hd, misc, [&](int i, int j) {
        const int t = i + j - 2;
        return bp[(size_t)(t >> 4) * (64 * KM) + (j - 1)] >> (2 * (15 - (t & 15))) & 3u;
      });
    }
  }
  hand_over<HEADLDS>();
  write_outputs<HEADLDS>(a, b, H, R, hd, misc);
}

// Rmax > 512: the workgroup walks the anti-diagonals.  v1[j] / v2[j] hold column j's cell
// of the last step and of the step before; a step reads its three predecessors, then
// (after a barrier) every lane moves its own column on.  Back-pointers: two bits per cell
// in the workspace, byte [(i-1) / 4][j-1], bits 2 ((i-1) % 4); a column's cells are always
// computed by the same lane, which therefore owns the byte.
// Dynamic LDS: misc[16] | v1[Rmax + 1] v2[Rmax + 1] | head (HEADLDS).
template <bool HEADLDS>
__global__ __launch_bounds__(256) void edit_align_loop_kernel(const EditArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  int* misc = reinterpret_cast<int*>(smem_raw);
  int* v1 = misc + kMisc;
  int* v2 = v1 + a.Rmax + 1;
  char* lds_head = smem_raw + kMisc * sizeof(int) + edit_rows_bytes(a.Rmax);
  const int b = blockIdx.x;
  char* wsb = a.ws + (size_t)b * a.ws_per_utt;
  int H, R;
  const Head hd = load_phase<HEADLDS>(a, b, lds_head, wsb, misc, H, R);
  unsigned char* bp = reinterpret_cast<unsigned char*>(wsb + (HEADLDS ? 0 : a.head_bytes));
  const int Rmax = a.Rmax;
  const int n = H > 0 && R > 0 ? H + R - 1 : 0;
  for (int t = 0; t < n; ++t) {
    const int d = t + 2, jlo = max(1, d - H), jhi = min(R, d - 1);
    // at most (Rmax + 255) / 256 <= 32 columns per lane: the new values wait in registers
    // for the barrier, in the order they are computed
    int keep_up[32], keep_new[32];
    int q = 0;
    for (int j = jlo + (int)threadIdx.x; j <= jhi; j += 256, ++q) {
      const int i = d - j;
      const int up = i == 1 ? j : v1[j];
      const int left = j == 1 ? i : v1[j - 1];
      const int dg = i == 1 ? j - 1 : j == 1 ? i - 1 : v2[j - 1];
      unsigned code;
      const int m = min3_choice(dg + (hd.hlab[i - 1] != hd.rlab[j - 1] ? 1 : 0), left + 1, up + 1, code);
      const size_t at = (size_t)((i - 1) >> 2) * Rmax + (j - 1);
      const int sh = 2 * ((i - 1) & 3);
      bp[at] = (unsigned char)((sh ? bp[at] : 0u) | (code << sh));
      keep_up[q & 31] = up;
      keep_new[q & 31] = m;
    }
    __syncthreads();
    q = 0;
    for (int j = jlo + (int)threadIdx.x; j <= jhi; j += 256, ++q) {
      v2[j] = keep_up[q & 31];
      v1[j] = keep_new[q & 31];
    }
    __syncthreads();
  }
  __threadfence();   // lane 0 reads every lane's back-pointers
  __syncthreads();
  if (threadIdx.x == 0) {
    misc[M_DIST] = n > 0 ? v1[R] : max(H, R);
    walk_back(H, R, hd, misc, [&](int i, int j) {
      return (unsigned)(bp[(size_t)((i - 1) >> 2) * Rmax + (j - 1)] >> (2 * ((i - 1) & 3))) & 3u;
    });
  }
  hand_over<HEADLDS>();
  write_outputs<HEADLDS>(a, b, H, R, hd, misc);
}

using EditKernel = void (*)(const EditArgs);

template <int KM>
EditKernel pick_edit(bool head_lds, bool bp_lds) {
  return bp_lds ? edit_align_kernel<KM, true, true> : head_lds ? edit_align_kernel<KM, true, false>
                                                               : edit_align_kernel<KM, false, false>;
}

bool edit_shape_ok(int B, int Hmax, int Rmax) {
  if (B >= 1 && Hmax >= 0 && Hmax <= kScoreMax && Rmax >= 0 && Rmax <= kScoreMax) return true;
  srf::set_error("edit_align: bad shape (B=%d Hmax=%d Rmax=%d): B >= 1, 0 <= Hmax, Rmax <= %d", B, Hmax, Rmax,
                 kScoreMax);
  return false;
}

}  // namespace

extern "C" {

size_t srf_edit_align_workspace(int B, int Hmax, int Rmax) {
  if (!edit_shape_ok(B, Hmax, Rmax)) return 0;
  const size_t need = (size_t)B * edit_geometry(Hmax, Rmax).ws_per_utt;
  return need > 16 ? need : 16;
}

int srf_edit_align(const int* hyp, const int* hyp_len, int Hmax, const int* ref, const int* ref_len, int Rmax, int B,
                   const int* fold, int n_fold, int* counts, int* hyp_to_ref, int* ref_to_hyp, long long* totals,
                   long long* confusion, int K, void* workspace, size_t workspace_bytes, void* stream) {
  if (!edit_shape_ok(B, Hmax, Rmax)) return SRF_EINVAL;
  SRF_REQUIRE(hyp_len && ref_len && counts && workspace, "edit_align: null pointer argument");
  SRF_REQUIRE((hyp || Hmax == 0) && (ref || Rmax == 0), "edit_align: null labels with Hmax = %d, Rmax = %d", Hmax,
              Rmax);
  SRF_REQUIRE(fold ? n_fold >= 0 : n_fold == 0, "edit_align: n_fold = %d %s a fold table", n_fold,
              fold ? "with" : "without");
  SRF_REQUIRE(confusion ? (K >= 1 && K <= 32767) : K >= 0, "edit_align: K = %d classes %s a confusion matrix", K,
              confusion ? "with" : "without");
  SRF_REQUIRE((uintptr_t)workspace % 16 == 0, "edit_align: the workspace must be 16-byte aligned");
  if (workspace_bytes < srf_edit_align_workspace(B, Hmax, Rmax)) {
    srf::set_error("edit alignment workspace too small");
    return SRF_EWORKSPACE;
  }
  const EditGeom g = edit_geometry(Hmax, Rmax);
  EditArgs a;
  a.hyp = hyp, a.hyp_len = hyp_len, a.ref = ref, a.ref_len = ref_len, a.fold = fold;
  a.Hmax = Hmax, a.Rmax = Rmax, a.n_fold = n_fold, a.K = K;
  a.counts = counts, a.hyp_to_ref = hyp_to_ref, a.ref_to_hyp = ref_to_hyp;
  a.totals = reinterpret_cast<unsigned long long*>(totals);
  a.confusion = reinterpret_cast<unsigned long long*>(confusion);
  a.ws = static_cast<char*>(workspace);
  a.ws_per_utt = g.ws_per_utt, a.head_bytes = g.head;
  const EditKernel kern = g.KM == 0   ? (g.head_lds ? edit_align_loop_kernel<true> : edit_align_loop_kernel<false>)
                          : g.KM == 2 ? pick_edit<2>(g.head_lds, g.bp_lds)
                          : g.KM == 4 ? pick_edit<4>(g.head_lds, g.bp_lds)
                                      : pick_edit<8>(g.head_lds, g.bp_lds);
  if (g.shmem > 64 * 1024)
    SRF_HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.shmem));
  hipLaunchKernelGGL(kern, dim3(B), dim3(256), g.shmem, static_cast<hipStream_t>(stream), a);
  SRF_LAUNCH_CHECK("edit_align");
  return SRF_OK;
}

}  // extern "C"
