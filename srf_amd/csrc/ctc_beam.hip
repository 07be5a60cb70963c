// CTC prefix beam search on the device: the algorithm of
// csrc/data/ctc_beam.cpp, one workgroup per utterance, a whole chunk of frames per
// launch, the beam kept in a device state block between launches.
//
// Per frame the host decoder walks the beam in slot order and creates, per slot k, the
// prefix itself and then its extensions by ascending class; a prefix reached twice (a beam
// entry that is the child (p, c) of another beam entry p) is one candidate whose two
// contributions are added.  Here every candidate has the index of its first creation,
//   key(k, itself) = k C,   key(k, extension c) = k C + 1 + (c < blank ? c : c - 1),
// the merged candidate lives at the smaller of its two keys, and the beam_width
// candidates that are largest by (total descending, key ascending) survive.  That is a
// total order, so the result does not depend on which lane looks at which candidate.
//
// No table of all prefixes ever made: the beam holds distinct prefixes, so extension
// (p, c) meets another candidate only if a beam entry n is the prefix p + c.  The host
// knows that from its persistent (parent node, label) -> node map, in which a prefix that
// left the beam and is made again (from its own parent, a frame or more later) gets its
// old node back and so finds its children that stayed.  Trie nodes here are appended per
// survivor and a prefix made again gets a new one, so node ids do not identify prefixes.
// A 64-bit hash of the label sequence does (hash(p + c) = mix(hash(p), c), a pure
// function of the prefix): every entry carries its own and its parent's, each frame
// starts by finding every entry's parent slot (parent hash = hash and length = length - 1
// over at most 128 x 128 pairs), and an entry marks its parent's extension in a
// [slot][class] byte table.  Two different prefixes of one beam collide with probability
// 2^-64 per pair.
//
// Candidate scores never go to memory: a lane computes prev + lp[c] for its (at most 32)
// candidates once and keeps the ordered bits in registers.  A radix select (four 8-bit
// passes over the ordered bits of the total, two more over the key if equal totals
// straddle the edge of the beam) finds the threshold; the survivors (at most 128)
// are ranked by counting and placed in rank order, new prefixes taking trie nodes in that
// order, so the state after a frame is a pure function of the state before it and the
// frame, whatever the chunking.
//
// With a language model fused in (srf_ctc_beam_lm_*) every extension
// also gets bonus[state of the prefix][class].  The push kernel is one template: without
// tables it is the kernel above, instruction for instruction; with them every entry carries
// its automaton state and accumulated bonus (two more beam arrays in the state block), and
// a frame's candidate bonuses are copied global -> LDS while the per-slot step runs.
#include <type_traits>

#include "srf_common.h"
#include "../../include/srf.h"

namespace {

constexpr int kThreads = 512;
constexpr int kMaxW = SRF_CTC_BEAM_MAX_WIDTH;
constexpr int kMaxC = SRF_CTC_BEAM_MAX_CLASSES;
constexpr int kHeader = 4;   // state words per utterance before the beam: entries, trie nodes, frames, unused
constexpr int kFields = 9;   // beam arrays: node, pb, pnb, last, len, hash (2 words), parent's hash (2 words)
constexpr int kLmFields = kFields + 2;   // with a fused language model: its state, the accumulated bonus
template <bool kLM>
constexpr int kFieldsOf = kLM ? kLmFields : kFields;
constexpr unsigned long long kRootHash = 0x243f6a8885a308d3ull;
static_assert(kMaxW * kMaxC <= (1 << 14), "a candidate key takes 14 bits");
constexpr int kPerLane = kMaxW * kMaxC / kThreads;   // candidates a lane looks at, at most
static_assert(kPerLane % 8 == 0, "the fused kernel copies the bonuses in groups of eight keys per lane");
static_assert(kThreads == 4 * kMaxW, "the ranking pass splits the survivors over four quarters of the workgroup");

constexpr unsigned kKeyMax = (1u << 14) - 1;
constexpr unsigned char kNoFold = 0xff;

__host__ __device__ inline size_t trie_capacity(int W, int max_frames) { return 1 + (size_t)max_frames * W; }
__host__ __device__ inline size_t state_words(int W, int max_frames, int fields) {
  return kHeader + (size_t)fields * W + 2 * trie_capacity(W, max_frames);
}

// hash of prefix + (c,) from the prefix's (the splitmix64 finaliser over hash ^ f(c))
__device__ __forceinline__ unsigned long long extend_hash(unsigned long long h, int c) {
  unsigned long long z = h ^ ((unsigned long long)(c + 1) * 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

__device__ __forceinline__ float neg_inf() { return -__builtin_inff(); }

__device__ __forceinline__ float log_sum_exp(float a, float b) {
  if (a == neg_inf()) return b;
  if (b == neg_inf()) return a;
  const float m = fmaxf(a, b);
  return m + log1pf(expf(-fabsf(a - b)));
}

// Order-preserving map of a float onto unsigned (larger float, larger word), -0 as +0;
// 0 is kept for "no candidate".
__device__ __forceinline__ unsigned ordered(float f) {
  unsigned b = __float_as_uint(f);
  if ((b << 1) == 0) b = 0;
  const unsigned u = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return u == 0 ? 1u : u;
}
__device__ __forceinline__ float unordered(unsigned u) {
  return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

// A fused language model: a deterministic automaton over the classes
// as two device tables, bonus [S][C] (what extending a prefix in state s by class c adds to
// its score) and next [S][C] (the state after it).  Both are functions of the prefix alone,
// as its hash is, so merging and re-made parents stay consistent.
struct LmTables {
  const float* bonus;
  const int* next;
  int S;
};
struct NoLmBeam {};
struct LmBeam {
  // [key]: the candidate's bonus, this frame.  First in the workgroup's LDS (Smem's base
  // class, the kernel's only shared variable): the global -> LDS copies that fill it take
  // their LDS address from M0, and all of it lies below 64 KiB.
  float cb[kMaxW * kMaxC];
  int lmst[2][kMaxW];    // the entry's state, in [0, S)
  float acc[2][kMaxW];   // the bonuses of its labels, added in label order
};
static_assert(sizeof(LmBeam::cb) <= (1 << 16), "the candidates' bonuses lie in the first 64 KiB of LDS");

template <bool kLM>
struct alignas(16) Smem : std::conditional_t<kLM, LmBeam, NoLmBeam> {
  float lp[kMaxC];
  // the beam, double-buffered over frames
  int node[2][kMaxW];
  float pb[2][kMaxW], pnb[2][kMaxW];
  int last[2][kMaxW], len[2][kMaxW];
  unsigned long long hash[2][kMaxW], phash[2][kMaxW];
  int ps[kMaxW];        // slot of the entry's parent in the current beam, -1 if it is not there
  // per slot, this frame
  float tot[kMaxW], npb[kMaxW], npnb[kMaxW];
  unsigned su[kMaxW];   // ordered total of the slot's own candidate
  int alias[kMaxW];     // the key its own candidate lives at
  int fidx[kMaxW];      // the extension it folded in (to clear the table), -1 if none
  // survivors
  unsigned long long sel[kMaxW];
  int rank[kMaxW], extb[kMaxW];
  unsigned hist[2][256];
  unsigned char fold[kMaxW * kMaxC];   // [slot * C + j]: the beam entry that extension is, or kNoFold
  int digit, above, eq, need, nsel, nadd;
};

struct Cand {
  unsigned u;   // 0: no candidate at this key
  int ext;      // 1: a new prefix (slot k extended by a class), 0: beam entry `slot` itself
  int slot;
};

__device__ __forceinline__ int class_of(int j, int blank) { return j - 1 < blank ? j - 1 : j; }

// Fused: where candidate i's bonus lies, bonus[state of its slot][its class].  Keys of
// consecutive lanes are consecutive classes of one slot, so a wave reads runs of a row.  A
// slot's own candidate (j = 0) has no class and reads its first extension's word, unused.
// A key past the last candidate reads the last slot's row (no branch; its word is unused too).
__device__ __forceinline__ int bonus_index(const Smem<true>& s, int cur, int i, const FastDiv& divC, int C,
                                           int blank, int nb) {
  const int k = (int)fdiv((unsigned)i, divC), j = max(i - k * C, 1);
  return s.lmst[cur][min(k, nb - 1)] * C + class_of(j, blank);
}

__device__ __forceinline__ void glds4(const float* src, float* lds_dst) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                   (__attribute__((address_space(3))) void*)lds_dst, 4, 0, 0);
}

template <bool kLM>
__device__ __forceinline__ Cand candidate(const Smem<kLM>& s, int cur, int i, const FastDiv& divC, int C, int blank) {
  const int k = (int)fdiv((unsigned)i, divC), j = i - k * C;
  Cand r{0u, 0, k};
  if (j == 0) {
    if (s.alias[k] == i) r.u = s.su[k];
    return r;
  }
  const unsigned char f = s.fold[i];
  if (f != kNoFold) {
    r.slot = f;
    if (s.alias[f] == i) r.u = s.su[f];
    return r;
  }
  const int c = class_of(j, blank);
  const float prev = c == s.last[cur][k] ? s.pb[cur][k] : s.tot[k];
  if (prev == neg_inf()) return r;
  if constexpr (kLM)
    r.u = ordered((prev + s.lp[c]) + s.cb[i]);
  else
    r.u = ordered(prev + s.lp[c]);
  r.ext = 1;
  return r;
}

// Wave 0 after a histogram pass: the bin in which the need-th largest matching candidate
// lies, how many lie in higher bins, and how many in that bin.  first: need is the beam
// width capped by the number of candidates.
template <bool kLM>
__device__ __forceinline__ void pick_bin(Smem<kLM>& s, const unsigned* h, int need, bool first, int W) {
  const int lane = threadIdx.x;
  const uint4 v = reinterpret_cast<const uint4*>(h)[lane];
  const int b[4] = {(int)v.x, (int)v.y, (int)v.z, (int)v.w};
  const int own = b[0] + b[1] + b[2] + b[3];
  int suf = own;   // candidates in this lane's bins and higher ones
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_down(suf, o, 64);
    if (lane + o < 64) suf += t;
  }
  const int total = __shfl(suf, 0, 64);
  if (first) need = min(W, total);
  int acc = suf - own;
  if (acc < need && need <= suf) {
#pragma unroll
    for (int q = 3; q >= 0; --q) {
      if (acc + b[q] >= need) {
        s.digit = 4 * lane + q;
        s.above = acc;
        s.eq = b[q];
        s.need = need;
        break;
      }
      acc += b[q];
    }
  }
}

__device__ __forceinline__ const LmTables& tables_of(const LmTables& lm) { return lm; }

// Lm: nothing, and this is the search of section 12 with the arguments it always had, or
// LmTables, and bonus[state][c] is added to every extension (section 17).
template <class... Lm>
__global__ __launch_bounds__(kThreads) void ctc_beam_push_kernel(unsigned* __restrict__ state,
                                                                 const float* __restrict__ logits,
                                                                 const int* __restrict__ n_valid, int n, int C,
                                                                 int blank, int W, int max_frames, FastDiv divC,
                                                                 Lm... tables) {
  constexpr bool kLM = sizeof...(Lm) == 1;
  static_assert(sizeof...(Lm) <= 1, "at most one language model");
  __shared__ Smem<kLM> s;
  const int b = blockIdx.x, t = threadIdx.x;
  const int nv = max(0, min(n_valid[b], n));
  if (nv == 0) return;
  const size_t cap = trie_capacity(W, max_frames);
  unsigned* st = state + (size_t)b * state_words(W, max_frames, kFieldsOf<kLM>);
  int* hdr = reinterpret_cast<int*>(st);
  unsigned* beam = st + kHeader;
  int* trie_parent = reinterpret_cast<int*>(beam + (size_t)kFieldsOf<kLM> * W);
  int* trie_label = trie_parent + cap;
  const float* x = logits + (size_t)b * n * C;

  int nb = min(max(hdr[0], 1), W), n_nodes = hdr[1];
  int cur = 0;
  if (t < nb) {
    s.node[0][t] = (int)beam[t];
    s.pb[0][t] = __uint_as_float(beam[W + t]);
    s.pnb[0][t] = __uint_as_float(beam[2 * W + t]);
    // (the clamp keeps a block that was never reset from indexing outside the tables)
    const int last = (int)beam[3 * W + t];
    s.last[0][t] = last >= C || last == blank ? -1 : max(last, -1);
    s.len[0][t] = (int)beam[4 * W + t];
    s.hash[0][t] = (unsigned long long)beam[6 * W + t] << 32 | beam[5 * W + t];
    s.phash[0][t] = (unsigned long long)beam[8 * W + t] << 32 | beam[7 * W + t];
    if constexpr (kLM) {
      // (clamped as last is: a block that was never reset does not index outside the tables)
      s.lmst[0][t] = min(max((int)beam[9 * W + t], 0), tables_of(tables...).S - 1);
      s.acc[0][t] = __uint_as_float(beam[10 * W + t]);
    }
  }
  if (t < kMaxW) s.ps[t] = -1;
  for (int i = t; i < kMaxW * kMaxC / 4; i += kThreads) reinterpret_cast<unsigned*>(s.fold)[i] = 0xffffffffu;
  if (t < 256) s.hist[0][t] = s.hist[1][t] = 0;

  __syncthreads();

  // wave 0 loads a frame's logits (classes lane and lane + 64) at the start of the frame before
  float xa = neg_inf(), xb = neg_inf();
  if (t < 64) {
    if (t < C) xa = x[t];
    if (t + 64 < C) xb = x[t + 64];
  }

  // Fused: a lane's candidates' bonuses.  They depend on the beam alone, not on the frame, so
  // they are asked for at the start of a frame, all at once, and arrive from L2 while the
  // parent match, the log-softmax and the per-slot step run; uc[m] holds the bonus until the
  // candidate's ordered total takes its place.

  for (int f = 0; f < nv; ++f) {
    // ---- every entry's parent slot: the entry one label shorter whose hash is its parent's
    {
      const int me = t & (kMaxW - 1), q = t / kMaxW;
      if (me < nb && s.last[cur][me] >= 0) {
        const unsigned long long want = s.phash[cur][me];
        const int want_len = s.len[cur][me] - 1;
        const int hi = min(nb, (q + 1) * (kMaxW / 4));
        for (int k = q * (kMaxW / 4); k < hi; ++k)
          if (s.hash[cur][k] == want && s.len[cur][k] == want_len) s.ps[me] = k;
      }
    }
    // ---- log-softmax of the frame
    if (t < 64) {
      const float a = xa, c = xb;
      if (f + 1 < nv) {
        const float* row = x + (size_t)(f + 1) * C;
        if (t < C) xa = row[t];
        if (t + 64 < C) xb = row[t + 64];
      }
      float mx = fmaxf(a, c);
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
      const float se = wave_sum((t < C ? expf(a - mx) : 0.f) + (t + 64 < C ? expf(c - mx) : 0.f));
      const float norm = mx + logf(se);
      if (t < C) s.lp[t] = a - norm;
      if (t + 64 < C) s.lp[t + 64] = c - norm;
    }
    __syncthreads();

    // Fused: every candidate's bonus, global -> LDS without passing through registers (the
    // sweeps below leave none).  They depend on the beam alone and land while the per-slot
    // step runs; the barrier after it waits for them.  Whole waves issue: the copy's LDS
    // address is the wave's first lane's plus 4 bytes per lane.
    if constexpr (kLM) {
      const int ncand = nb * C;
      // (the lane index made opaque: computed from t, the 32 slot and class indices would be
      // kept in registers over the whole frame loop, and there are none left for them)
      int lane = t;
      asm volatile("" : "+v"(lane));
      // Groups of eight without a branch inside: a group's eight state reads from LDS come
      // first and its copies go out back to back; a key past the last candidate copies a
      // word nobody uses.
#pragma unroll
      for (int g = 0; g < kPerLane; g += 8) {
        if (g * kThreads >= ncand) break;
        int at[8];   // (read before the group's first copy: a copy writes LDS, and no read moves across it)
#pragma unroll
        for (int m = 0; m < 8; ++m) at[m] = bonus_index(s, cur, (g + m) * kThreads + lane, divC, C, blank, nb);
#pragma unroll
        for (int m = 0; m < 8; ++m)
          glds4(tables_of(tables...).bonus + at[m], &s.cb[(g + m) * kThreads + lane]);
      }
    }

    // ---- per beam slot: its own candidate, with its parent's extension folded in
    if (t < kMaxW) {
      s.rank[t] = 0;
      s.extb[t] = 0;
    }
    if (t == 0) s.nsel = 0;
    if (t < nb) {
      const float pb = s.pb[cur][t], pnb = s.pnb[cur][t];
      const int last = s.last[cur][t], ps = s.ps[t];
      float fold_bonus = 0.f;   // fused: of the parent's extension by last, from the parent's state
      if constexpr (kLM) {
        if (ps >= 0) fold_bonus = tables_of(tables...).bonus[s.lmst[cur][ps] * C + last];
      }
      const float tot = log_sum_exp(pb, pnb);
      float npnb = last >= 0 ? pnb + s.lp[last] : neg_inf();
      int alias = t * C, fidx = -1;
      if (ps >= 0) {
        const float ppb = s.pb[cur][ps];
        const float prev = last == s.last[cur][ps] ? ppb : log_sum_exp(ppb, s.pnb[cur][ps]);
        if (prev != neg_inf()) {
          if constexpr (kLM)
            npnb = log_sum_exp(npnb, (prev + s.lp[last]) + fold_bonus);
          else
            npnb = log_sum_exp(npnb, prev + s.lp[last]);
          fidx = ps * C + 1 + (last < blank ? last : last - 1);
          s.fold[fidx] = (unsigned char)t;
          alias = min(alias, fidx);
        }
      }
      const float npb = tot + s.lp[blank];
      s.tot[t] = tot;
      s.npb[t] = npb;
      s.npnb[t] = npnb;
      s.su[t] = ordered(log_sum_exp(npb, npnb));
      s.alias[t] = alias;
      s.fidx[t] = fidx;
    }
    __syncthreads();

    // ---- radix select: the need-th largest (ordered total, kKeyMax - key)
    // Each lane keeps the ordered totals of its candidates (keys t, t + kThreads, ...) in
    // registers for all passes.  Totals of one frame share their leading bits, so a lane
    // counts runs of equal digits and adds each run to the histogram once.
    const int ncand = nb * C;
    unsigned uc[kPerLane];
#pragma unroll
    for (int m = 0; m < kPerLane; ++m) {
      const int i = m * kThreads + t;
      uc[m] = i < ncand ? candidate(s, cur, i, divC, C, blank).u : 0u;
    }
    unsigned V = 0, Lthr = 0;
    int need = 0, eq = 0;
    for (int p = 0; p < 6; ++p) {
      const bool on_key = p >= 4;
      const int shift = on_key ? 8 * (5 - p) : 8 * (3 - p);
      unsigned* h = s.hist[p & 1];
      if (t < 256) s.hist[(p + 1) & 1][t] = 0;
      unsigned run_digit = 0, run = 0;
#pragma unroll
      for (int m = 0; m < kPerLane; ++m) {
        if (m * kThreads >= ncand) break;
        const unsigned u = uc[m];
        if (u == 0) continue;
        unsigned digit;
        if (!on_key) {
          if (p != 0 && (u >> (shift + 8)) != (V >> (shift + 8))) continue;
          digit = (u >> shift) & 255u;
        } else {
          if (u != V) continue;
          const unsigned lo = kKeyMax - (unsigned)(m * kThreads + t);
          if (p != 4 && (lo >> 8) != (Lthr >> 8)) continue;
          digit = (lo >> shift) & 255u;
        }
        if (digit != run_digit) {
          if (run) atomicAdd(&h[run_digit], run);
          run_digit = digit;
          run = 0;
        }
        ++run;
      }
      if (run) atomicAdd(&h[run_digit], run);
      __syncthreads();
      if (t < 64) pick_bin(s, h, need, p == 0, W);
      __syncthreads();
      need = s.need - s.above;
      eq = s.eq;
      if (on_key)
        Lthr |= (unsigned)s.digit << shift;
      else
        V |= (unsigned)s.digit << shift;
      // after the fourth pass V is the threshold total: eq candidates have it, need of
      // them survive.  All of them: done; else the two passes over the key choose.
      // (hist[0] was cleared during the fourth pass, as it is during the sixth)
      if (p == 3 && eq == need) break;
    }

    // ---- the survivors, in any order
#pragma unroll
    for (int m = 0; m < kPerLane; ++m) {
      if (m * kThreads >= ncand) break;
      const unsigned u = uc[m];
      if (u == 0) continue;
      const int i = m * kThreads + t;
      const unsigned lo = kKeyMax - (unsigned)i;
      if (u > V || (u == V && lo >= Lthr)) {
        const int ext = candidate(s, cur, i, divC, C, blank).ext;
        const int at = atomicAdd(&s.nsel, 1);
        if (at < kMaxW) s.sel[at] = (unsigned long long)u << 32 | (lo << 1) | (unsigned)ext;
      }
    }
    __syncthreads();
    const int nsel = min(s.nsel, W);

    // ---- rank of each survivor, and how many new prefixes precede it
    {
      const int me = t & (kMaxW - 1), q = t / kMaxW;
      if (me < nsel) {
        const unsigned long long mine = s.sel[me];
        int r = 0, e = 0;
        const int hi = min(nsel, (q + 1) * (kMaxW / 4));
        for (int o = q * (kMaxW / 4); o < hi; ++o) {
          const unsigned long long other = s.sel[o];
          if (other > mine) {
            ++r;
            e += (int)(other & 1u);
          }
        }
        if (r) atomicAdd(&s.rank[me], r);
        if (e) atomicAdd(&s.extb[me], e);
      }
    }
    __syncthreads();

    // ---- place them: the next beam, in rank order
    const int nxt = cur ^ 1;
    if (t < kMaxW) s.ps[t] = -1;
    if (t < nsel) {
      const unsigned long long mine = s.sel[t];
      const int r = s.rank[t], ext = (int)(mine & 1u);
      const int i = (int)(kKeyMax - ((unsigned)mine >> 1));
      const int k = (int)fdiv((unsigned)i, divC), j = i - k * C;
      if (!ext) {
        const int from = j == 0 ? k : (int)s.fold[i];
        s.node[nxt][r] = s.node[cur][from];
        s.pb[nxt][r] = s.npb[from];
        s.pnb[nxt][r] = s.npnb[from];
        s.last[nxt][r] = s.last[cur][from];
        s.len[nxt][r] = s.len[cur][from];
        s.hash[nxt][r] = s.hash[cur][from];
        s.phash[nxt][r] = s.phash[cur][from];
        if constexpr (kLM) {
          s.lmst[nxt][r] = s.lmst[cur][from];
          s.acc[nxt][r] = s.acc[cur][from];
        }
      } else {
        const int c = class_of(j, blank);
        if constexpr (kLM) {
          // the only read of next: a survivor that is a new prefix.  (Clamped like a state
          // from the block: a table that breaks its contract cannot lead outside the tables.)
          const int at = s.lmst[cur][k] * C + c;
          s.lmst[nxt][r] = min(max(tables_of(tables...).next[at], 0), tables_of(tables...).S - 1);
          s.acc[nxt][r] = s.acc[cur][k] + tables_of(tables...).bonus[at];
        }
        const size_t id = (size_t)n_nodes + s.extb[t];
        if (id < cap) {   // holds while the frames pushed stay within max_frames (checked on the host)
          trie_parent[id] = s.node[cur][k];
          trie_label[id] = c;
        }
        s.node[nxt][r] = (int)id;
        s.pb[nxt][r] = neg_inf();
        s.pnb[nxt][r] = unordered((unsigned)(mine >> 32));
        s.last[nxt][r] = c;
        s.len[nxt][r] = s.len[cur][k] + 1;
        s.hash[nxt][r] = extend_hash(s.hash[cur][k], c);
        s.phash[nxt][r] = s.hash[cur][k];
      }
      if (r == nsel - 1) s.nadd = s.extb[t] + ext;
    }
    __syncthreads();

    // ---- the fold table back to empty (it is written again after the next frame's first barrier)
    if (t < nb && s.fidx[t] >= 0) s.fold[s.fidx[t]] = kNoFold;
    n_nodes += s.nadd;
    nb = nsel;
    cur = nxt;
  }
  if (t < nb) {
    beam[t] = (unsigned)s.node[cur][t];
    beam[W + t] = __float_as_uint(s.pb[cur][t]);
    beam[2 * W + t] = __float_as_uint(s.pnb[cur][t]);
    beam[3 * W + t] = (unsigned)s.last[cur][t];
    beam[4 * W + t] = (unsigned)s.len[cur][t];
    beam[5 * W + t] = (unsigned)s.hash[cur][t];
    beam[6 * W + t] = (unsigned)(s.hash[cur][t] >> 32);
    beam[7 * W + t] = (unsigned)s.phash[cur][t];
    beam[8 * W + t] = (unsigned)(s.phash[cur][t] >> 32);
    if constexpr (kLM) {
      beam[9 * W + t] = (unsigned)s.lmst[cur][t];
      beam[10 * W + t] = __float_as_uint(s.acc[cur][t]);
    }
  }
  if (t == 0) {
    hdr[0] = nb;
    hdr[1] = n_nodes;
    hdr[2] += nv;
  }
}

// One utterance's block back to the single empty prefix (one lane).
template <bool kLM>
__device__ __forceinline__ void reset_utterance(unsigned* st, int W, int max_frames) {
  int* hdr = reinterpret_cast<int*>(st);
  unsigned* beam = st + kHeader;
  int* trie_parent = reinterpret_cast<int*>(beam + (size_t)kFieldsOf<kLM> * W);
  hdr[0] = 1;
  hdr[1] = 1;
  hdr[2] = 0;
  hdr[3] = 0;
  beam[0] = 0;                                // the root: the empty prefix
  beam[W] = __float_as_uint(0.f);             // pb
  beam[2 * W] = __float_as_uint(neg_inf());   // pnb
  beam[3 * W] = (unsigned)-1;                 // no last label
  beam[4 * W] = 0;                            // length
  beam[5 * W] = (unsigned)kRootHash;
  beam[6 * W] = (unsigned)(kRootHash >> 32);
  beam[7 * W] = beam[8 * W] = 0;              // no parent
  if constexpr (kLM) {
    beam[9 * W] = 0;                          // state 0 belongs to the empty prefix
    beam[10 * W] = __float_as_uint(0.f);      // no bonus yet
  }
  trie_parent[0] = -1;
  trie_parent[trie_capacity(W, max_frames)] = -1;   // label of the root
}

template <bool kLM>
__global__ __launch_bounds__(64) void ctc_beam_reset_kernel(unsigned* __restrict__ state, int W, int max_frames) {
  if (threadIdx.x != 0) return;
  reset_utterance<kLM>(state + (size_t)blockIdx.x * state_words(W, max_frames, kFieldsOf<kLM>), W, max_frames);
}

// The most probable prefix of utterance b, by one lane: the first slot with the largest
// total (after a frame the beam is in rank order, so slot 0), its labels from a walk of the
// trie from its node to the root.  Labels at index max_len and beyond are not stored.
// (fused: log_prob is the ranking score, lm_score the accumulated bonus of that entry)
template <bool kLM>
__device__ __forceinline__ void best_of(const unsigned* st, int b, int W, int max_frames, int max_len,
                                        int* __restrict__ labels, int* __restrict__ count,
                                        float* __restrict__ log_prob, float* __restrict__ lm_score) {
  const size_t cap = trie_capacity(W, max_frames);
  const int* hdr = reinterpret_cast<const int*>(st);
  const unsigned* beam = st + kHeader;
  const int* trie_parent = reinterpret_cast<const int*>(beam + (size_t)kFieldsOf<kLM> * W);
  const int* trie_label = trie_parent + cap;
  const int nb = min(max(hdr[0], 1), W);
  int best = 0;
  float best_tot = log_sum_exp(__uint_as_float(beam[W]), __uint_as_float(beam[2 * W]));
  for (int k = 1; k < nb; ++k) {
    const float tot = log_sum_exp(__uint_as_float(beam[W + k]), __uint_as_float(beam[2 * W + k]));
    if (tot > best_tot) {
      best = k;
      best_tot = tot;
    }
  }
  const int len = min(max((int)beam[4 * W + best], 0), max_frames);
  int* out = labels + (size_t)b * max_len;
  int node = (int)beam[best];
  for (int i = len - 1; i >= 0 && node > 0 && (size_t)node < cap; --i) {
    if (i < max_len) out[i] = trie_label[node];
    node = trie_parent[node];
  }
  count[b] = len;
  log_prob[b] = best_tot;
  if constexpr (kLM) lm_score[b] = __uint_as_float(beam[10 * W + best]);
}

// One wave per utterance; lane 0 does the work.
template <bool kLM>
__global__ __launch_bounds__(64) void ctc_beam_best_kernel(const unsigned* __restrict__ state, int W, int max_frames,
                                                           int* __restrict__ labels, int* __restrict__ count,
                                                           float* __restrict__ log_prob,
                                                           float* __restrict__ lm_score) {
  if (threadIdx.x != 0) return;
  const int b = blockIdx.x;
  best_of<kLM>(state + (size_t)b * state_words(W, max_frames, kFieldsOf<kLM>), b, W, max_frames, max_frames, labels,
               count, log_prob, lm_score);
}

// Closing a segment.  One wave per utterance.  cut[b] >= 0: the
// utterance's segment ends with chunk frame cut[b], which is the last frame pushed to it;
// lane 0 writes what best would return and puts the block back to the reset state, this
// utterance alone.  cut[b] < 0: count[b] = -1 and nothing else is touched.
// With rest: the whole wave then copies the chunk's frames after the cut, frames
// [cut[b] + 1, n_valid[b]), to the front of rest [b][n][C] and sets n_rest[b] to their
// number (0 without a cut), for the push that opens the next segment.
template <bool kLM>
__global__ __launch_bounds__(64) void ctc_beam_cut_kernel(unsigned* __restrict__ state, int W, int max_frames,
                                                          const int* __restrict__ cut, int max_len,
                                                          int* __restrict__ labels, int* __restrict__ count,
                                                          float* __restrict__ log_prob, float* __restrict__ lm_score,
                                                          const float* __restrict__ logits,
                                                          const int* __restrict__ n_valid, int n, int C,
                                                          float* __restrict__ rest, int* __restrict__ n_rest) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int at = cut[b];
  if (lane == 0) {
    if (at < 0) {
      count[b] = -1;
    } else {
      unsigned* st = state + (size_t)b * state_words(W, max_frames, kFieldsOf<kLM>);
      best_of<kLM>(st, b, W, max_frames, max_len, labels, count, log_prob, lm_score);
      reset_utterance<kLM>(st, W, max_frames);
    }
  }
  if (!rest) return;
  const int nv = max(0, min(n_valid[b], n));
  const int first = at < 0 ? 0 : min(at, n - 1) + 1;   // (at < n by contract; clamped, the copy stays inside the chunk)
  const int left = at < 0 ? 0 : max(0, nv - first);
  if (lane == 0) n_rest[b] = left;
  const float* src = logits + ((size_t)b * n + first) * C;
  float* dst = rest + (size_t)b * n * C;
  for (int i = lane; i < left * C; i += 64) dst[i] = src[i];
}

// The N first beam entries of each utterance.  After a frame the beam lies in rank order
// (total descending, creation key ascending), so hypothesis i is slot i; before the first
// frame the root is the only entry.  The walk from a node to the root follows parent
// pointers and is serial, so a lane walks one hypothesis: a wave holds 64 (utterance,
// hypothesis) pairs, every lane on its own trie path.  Grid (B, ceil(N / 64)).
// (Fused: lm_score [B][N] gets each entry's accumulated bonus, 0 past the beam's entries.)
template <bool kLM>
__global__ __launch_bounds__(64) void ctc_beam_nbest_kernel(const unsigned* __restrict__ state, int W, int max_frames,
                                                            int N, int max_len, int* __restrict__ labels,
                                                            int* __restrict__ count, float* __restrict__ log_prob,
                                                            float* __restrict__ lm_score, int* __restrict__ n_hyp) {
  const int b = blockIdx.x, i = blockIdx.y * 64 + threadIdx.x;
  if (i >= N) return;
  const size_t cap = trie_capacity(W, max_frames);
  const unsigned* st = state + (size_t)b * state_words(W, max_frames, kFieldsOf<kLM>);
  const int* hdr = reinterpret_cast<const int*>(st);
  const unsigned* beam = st + kHeader;
  const int* trie_parent = reinterpret_cast<const int*>(beam + (size_t)kFieldsOf<kLM> * W);
  const int* trie_label = trie_parent + cap;
  const int nb = min(max(hdr[0], 1), W);
  if (i == 0) n_hyp[b] = min(N, nb);
  const size_t row = (size_t)b * N + i;
  if (i >= nb) {
    count[row] = 0;
    log_prob[row] = neg_inf();
    if constexpr (kLM) lm_score[row] = 0.f;
    return;
  }
  log_prob[row] = log_sum_exp(__uint_as_float(beam[W + i]), __uint_as_float(beam[2 * W + i]));
  if constexpr (kLM) lm_score[row] = __uint_as_float(beam[10 * W + i]);
  const int len = min(max((int)beam[4 * W + i], 0), max_frames);
  if (len > max_len) {
    count[row] = -1;
    return;
  }
  int* out = labels + row * max_len;
  int node = (int)beam[i];
  for (int k = len - 1; k >= 0 && node > 0 && (size_t)node < cap; --k) {
    out[k] = trie_label[node];
    node = trie_parent[node];
  }
  count[row] = len;
}

bool shape_ok(int B, int C, int W, int max_frames, int fields) {
  return B >= 1 && C >= 2 && C <= kMaxC && W >= 1 && W <= kMaxW && max_frames >= 1 &&
         state_words(W, max_frames, fields) <= (size_t)0x7fffffff;
}

// The entry points' checks; what: the entry point's name in the message, fields: kFields
// or kLmFields.
#define SRF_BEAM_SHAPE(what, fields)                                                                                  \
  SRF_REQUIRE(shape_ok(B, C, beam_width, max_frames, fields),                                                         \
              "%s: need B >= 1, 2 <= C <= %d, 1 <= beam_width <= %d, max_frames >= 1 and a trie below 2^31 "          \
              "words (B=%d C=%d beam_width=%d max_frames=%d)",                                                        \
              what, kMaxC, kMaxW, B, C, beam_width, max_frames)

#define SRF_BEAM_BYTES(what, fields)                                                                                  \
  SRF_REQUIRE(state_bytes >= (size_t)B * state_words(beam_width, max_frames, fields) * 4,                             \
              "%s: the state block holds %zu bytes, %zu are needed", what, state_bytes,                               \
              (size_t)B * state_words(beam_width, max_frames, fields) * 4)

size_t state_bytes_of(const char* what, int B, int C, int beam_width, int max_frames, int fields) {
  if (!shape_ok(B, C, beam_width, max_frames, fields)) {
    srf::set_error("%s: need B >= 1, 2 <= C <= %d, 1 <= beam_width <= %d, max_frames >= 1 and a "
                   "trie below 2^31 words (B=%d C=%d beam_width=%d max_frames=%d)",
                   what, kMaxC, kMaxW, B, C, beam_width, max_frames);
    return 0;
  }
  return (size_t)B * state_words(beam_width, max_frames, fields) * 4;
}

template <bool kLM>
int reset(const char* what, void* state, size_t state_bytes, int B, int C, int beam_width, int max_frames,
          int* frames_pushed, void* stream) {
  SRF_BEAM_SHAPE(what, kFieldsOf<kLM>);
  SRF_REQUIRE(state && frames_pushed, "%s: null state / frames_pushed", what);
  SRF_BEAM_BYTES(what, kFieldsOf<kLM>);
  hipLaunchKernelGGL(ctc_beam_reset_kernel<kLM>, dim3((unsigned)B), dim3(64), 0, static_cast<hipStream_t>(stream),
                     static_cast<unsigned*>(state), beam_width, max_frames);
  SRF_LAUNCH_CHECK(what);
  *frames_pushed = 0;
  return SRF_OK;
}

// lm: null for the unfused search
int push(const char* what, void* state, size_t state_bytes, int B, int C, int beam_width, int max_frames, int blank,
         const float* logits, const int* n_valid, int n, const LmTables* lm, int* frames_pushed, void* stream) {
  const int fields = lm ? kLmFields : kFields;
  SRF_BEAM_SHAPE(what, fields);
  SRF_REQUIRE(state && frames_pushed, "%s: null state / frames_pushed", what);
  SRF_BEAM_BYTES(what, fields);
  SRF_REQUIRE(blank >= 0 && blank < C, "%s: blank = %d outside [0, %d)", what, blank, C);
  SRF_REQUIRE(n >= 0 && n_valid, "%s: need n >= 0 and n_valid (n=%d)", what, n);
  SRF_REQUIRE(n == 0 || logits, "%s: null logits with n = %d", what, n);
  if (lm) {
    SRF_REQUIRE(lm->bonus && lm->next, "%s: null language-model table", what);
    SRF_REQUIRE(lm->S >= 1 && (long long)lm->S * C < (1ll << 31),
                "%s: need n_states >= 1 and n_states * C < 2^31 (n_states=%d C=%d)", what, lm->S, C);
  }
  SRF_REQUIRE(*frames_pushed >= 0 && (long long)*frames_pushed + n <= max_frames,
              "%s: %d frames after %d pushed since the reset exceed max_frames = %d", what, n, *frames_pushed,
              max_frames);
  if (n == 0) return SRF_OK;
  if (lm)
    hipLaunchKernelGGL(ctc_beam_push_kernel<LmTables>, dim3((unsigned)B), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), static_cast<unsigned*>(state), logits, n_valid, n, C, blank,
                       beam_width, max_frames, make_fastdiv((unsigned)C), *lm);
  else
    hipLaunchKernelGGL(ctc_beam_push_kernel<>, dim3((unsigned)B), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                       static_cast<unsigned*>(state), logits, n_valid, n, C, blank, beam_width, max_frames,
                       make_fastdiv((unsigned)C));
  SRF_LAUNCH_CHECK(what);
  *frames_pushed += n;
  return SRF_OK;
}

template <bool kLM>
int best(const char* what, const void* state, size_t state_bytes, int B, int C, int beam_width, int max_frames,
         int* labels, int* count, float* log_prob, float* lm_score, void* stream) {
  SRF_BEAM_SHAPE(what, kFieldsOf<kLM>);
  SRF_REQUIRE(state && labels && count && log_prob && (lm_score || !kLM), "%s: null pointer argument", what);
  SRF_BEAM_BYTES(what, kFieldsOf<kLM>);
  hipLaunchKernelGGL(ctc_beam_best_kernel<kLM>, dim3((unsigned)B), dim3(64), 0, static_cast<hipStream_t>(stream),
                     static_cast<const unsigned*>(state), beam_width, max_frames, labels, count, log_prob, lm_score);
  SRF_LAUNCH_CHECK(what);
  return SRF_OK;
}

template <bool kLM>
int cut(const char* what, void* state, size_t state_bytes, int B, int C, int beam_width, int max_frames,
        const int* cut_at, int max_len, int* labels, int* count, float* log_prob, float* lm_score, const float* logits,
        const int* n_valid, int n, float* rest, int* n_rest, void* stream) {
  SRF_BEAM_SHAPE(what, kFieldsOf<kLM>);
  SRF_REQUIRE(max_len >= 1, "%s: need max_len >= 1, got %d", what, max_len);
  SRF_REQUIRE(state && cut_at && labels && count && log_prob && (lm_score || !kLM), "%s: null pointer argument", what);
  SRF_REQUIRE(!rest || (logits && n_valid && n_rest && n >= 1),
              "%s: the frames after the cut need logits, n_valid, n_rest and n >= 1 (n=%d)", what, n);
  SRF_BEAM_BYTES(what, kFieldsOf<kLM>);
  hipLaunchKernelGGL(ctc_beam_cut_kernel<kLM>, dim3((unsigned)B), dim3(64), 0, static_cast<hipStream_t>(stream),
                     static_cast<unsigned*>(state), beam_width, max_frames, cut_at, max_len, labels, count, log_prob,
                     lm_score, logits, n_valid, n, C, rest, n_rest);
  SRF_LAUNCH_CHECK(what);
  return SRF_OK;
}

template <bool kLM>
int nbest(const char* what, const void* state, size_t state_bytes, int B, int C, int beam_width, int max_frames, int N,
          int max_len, int* labels, int* count, float* log_prob, float* lm_score, int* n_hyp, void* stream) {
  SRF_BEAM_SHAPE(what, kFieldsOf<kLM>);
  SRF_REQUIRE(N >= 1 && N <= beam_width && max_len >= 1,
              "%s: need 1 <= N <= beam_width and max_len >= 1 (N=%d beam_width=%d max_len=%d)", what, N, beam_width,
              max_len);
  SRF_REQUIRE(state && labels && count && log_prob && n_hyp && (lm_score || !kLM), "%s: null pointer argument", what);
  SRF_BEAM_BYTES(what, kFieldsOf<kLM>);
  hipLaunchKernelGGL(ctc_beam_nbest_kernel<kLM>, dim3((unsigned)B, (unsigned)((N + 63) / 64)), dim3(64), 0,
                     static_cast<hipStream_t>(stream), static_cast<const unsigned*>(state), beam_width, max_frames, N,
                     max_len, labels, count, log_prob, lm_score, n_hyp);
  SRF_LAUNCH_CHECK(what);
  return SRF_OK;
}

}  // namespace

extern "C" size_t srf_ctc_beam_state_bytes(int B, int C, int beam_width, int max_frames) {
  return state_bytes_of("ctc_beam_state_bytes", B, C, beam_width, max_frames, kFields);
}

extern "C" int srf_ctc_beam_reset(void* state, size_t state_bytes, int B, int C, int beam_width, int max_frames,
                                  int* frames_pushed, void* stream) {
  return reset<false>("ctc_beam_reset", state, state_bytes, B, C, beam_width, max_frames, frames_pushed, stream);
}

extern "C" int srf_ctc_beam_push_n(void* state, size_t state_bytes, int B, int C, int beam_width, int max_frames,
                                   int blank, const float* logits, const int* n_valid, int n, int* frames_pushed,
                                   void* stream) {
  return push("ctc_beam_push", state, state_bytes, B, C, beam_width, max_frames, blank, logits, n_valid, n, nullptr,
              frames_pushed, stream);
}

extern "C" int srf_ctc_beam_best(const void* state, size_t state_bytes, int B, int C, int beam_width, int max_frames,
                                 int* labels, int* count, float* log_prob, void* stream) {
  return best<false>("ctc_beam_best", state, state_bytes, B, C, beam_width, max_frames, labels, count, log_prob,
                     nullptr, stream);
}

extern "C" int srf_ctc_beam_nbest(const void* state, size_t state_bytes, int B, int C, int beam_width, int max_frames,
                                  int N, int max_len, int* labels, int* count, float* log_prob, int* n_hyp,
                                  void* stream) {
  return nbest<false>("ctc_beam_nbest", state, state_bytes, B, C, beam_width, max_frames, N, max_len, labels, count,
                      log_prob, nullptr, n_hyp, stream);
}

extern "C" int srf_ctc_beam_cut(void* state, size_t state_bytes, int B, int C, int beam_width, int max_frames,
                                const int* cut_at, int max_len, int* labels, int* count, float* log_prob,
                                const float* logits, const int* n_valid, int n, float* rest, int* n_rest,
                                void* stream) {
  return cut<false>("ctc_beam_cut", state, state_bytes, B, C, beam_width, max_frames, cut_at, max_len, labels, count,
                    log_prob, nullptr, logits, n_valid, n, rest, n_rest, stream);
}

extern "C" int srf_ctc_beam_lm_cut(void* state, size_t state_bytes, int B, int C, int beam_width, int max_frames,
                                   const int* cut_at, int max_len, int* labels, int* count, float* score,
                                   float* lm_score, const float* logits, const int* n_valid, int n, float* rest,
                                   int* n_rest, void* stream) {
  return cut<true>("ctc_beam_lm_cut", state, state_bytes, B, C, beam_width, max_frames, cut_at, max_len, labels, count,
                   score, lm_score, logits, n_valid, n, rest, n_rest, stream);
}

extern "C" size_t srf_ctc_beam_lm_state_bytes(int B, int C, int beam_width, int max_frames) {
  return state_bytes_of("ctc_beam_lm_state_bytes", B, C, beam_width, max_frames, kLmFields);
}

extern "C" int srf_ctc_beam_lm_reset(void* state, size_t state_bytes, int B, int C, int beam_width, int max_frames,
                                     int* frames_pushed, void* stream) {
  return reset<true>("ctc_beam_lm_reset", state, state_bytes, B, C, beam_width, max_frames, frames_pushed, stream);
}

extern "C" int srf_ctc_beam_lm_push_n(void* state, size_t state_bytes, int B, int C, int beam_width, int max_frames,
                                      int blank, const float* logits, const int* n_valid, int n, const float* bonus,
                                      const int* next, int n_states, int* frames_pushed, void* stream) {
  const LmTables lm{bonus, next, n_states};
  return push("ctc_beam_lm_push", state, state_bytes, B, C, beam_width, max_frames, blank, logits, n_valid, n, &lm,
              frames_pushed, stream);
}

extern "C" int srf_ctc_beam_lm_best(const void* state, size_t state_bytes, int B, int C, int beam_width,
                                    int max_frames, int* labels, int* count, float* score, float* lm_score,
                                    void* stream) {
  return best<true>("ctc_beam_lm_best", state, state_bytes, B, C, beam_width, max_frames, labels, count, score,
                    lm_score, stream);
}

extern "C" int srf_ctc_beam_lm_nbest(const void* state, size_t state_bytes, int B, int C, int beam_width,
                                     int max_frames, int N, int max_len, int* labels, int* count, float* score,
                                     float* lm_score, int* n_hyp, void* stream) {
  return nbest<true>("ctc_beam_lm_nbest", state, state_bytes, B, C, beam_width, max_frames, N, max_len, labels, count,
                     score, lm_score, n_hyp, stream);
}
