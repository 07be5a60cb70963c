// Host interface of the 32x32-tile split-fp16 DR passes (route_fwd32.hip) and the layer
// geometry they share with route_dr.hip, whose resolve() decides per shape whether these
// passes or its own exact-fp32 ones run (DrPlan, there).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace srf {

// One DR layer call.  Every host function of both files takes this, none a list of ints.
struct DrGeom {
  int B, T, N, din, lpad, rpad, J, dout, iters, mask_first;
  int F() const { return B * T; }                     // frames
  int in_n() const { return N * (lpad + rpad + 1); }   // input capsules of a frame's window
  int JD() const { return J * dout; }                 // output rows
  int NT() const { return (J * dout + 15) / 16; }     // 16-row tiles
};

// Row tiles (of 32 rows) per wave of route_fwd32 / route_bwd32 for din 8, 16.
constexpr int kFwd32TW = 4;
// Frame stride of the stored couplings (frame-minor layout, 32-frame aligned).
__host__ __device__ inline int fwd32_frame_stride(int F) { return (F + 31) / 32 * 32; }

// Balanced split of the r >= 1 passes.  The linear space of units u = ft * in_n + i
// (frame tile ft, input capsule i), U = n_ftiles * in_n of them, is cut into G contiguous
// spans: workgroup w owns [bal_first(w), bal_first(w + 1)).  A segment is the part of a
// span inside one frame tile; it writes its partial sum into the slab slot that is its
// ordinal among the tile's segments, w - bal_owner(ft * in_n).  1 <= G <= U (every span
// holds a unit) and U * (G + 1) < 2^31 (fwd32_plan), so 32-bit arithmetic is exact.
__host__ __device__ inline int bal_first(int w, int U, int G) {
  return (int)((uint32_t)w * (uint32_t)U / (uint32_t)G);
}
// the workgroup whose span holds unit u: the largest w with bal_first(w) <= u
__host__ __device__ inline int bal_owner(int u, int U, int G) {
  return (int)((((uint32_t)u + 1u) * (uint32_t)G - 1u) / (uint32_t)U);
}
// segments (= slab slots in use) of frame tile ft
__host__ __device__ inline int bal_tile_slots(int ft, int in_n, int U, int G) {
  return bal_owner((ft + 1) * in_n - 1, U, G) - bal_owner(ft * in_n, U, G) + 1;
}
// Placement of the balanced spans on the XCDs.  Workgroup w walks capsule (p_w + k) % in_n
// at its step k, p_w = bal_first(w) % in_n, so the distance between two workgroups'
// capsules lasts for the whole pass; p_w / in_n is, up to the floor, (w * n_ft % G) / G
// (U / (G * in_n) = n_ft / G).  The dispatcher deals blocks round-robin over the 8 XCDs:
// XCD x runs blocks x, x + 8, ...  With block b = workgroup b an XCD's workgroups are
// spread over all of W at every step; bal_place instead ranks the blocks XCD-major and
// hands rank r the workgroup of the r-th smallest phase, so an XCD's workgroups read
// neighbouring W slabs and share them in its L2.  With d = gcd(n_ft, G), G' = G / d and
// inv = (n_ft / d)^-1 mod G' (bal_place_params), the phases are the multiples of d / G,
// each held by the d workgroups w0 + j * G'.  d = 0 is the identity (placement off, or
// G <= 8: one block per XCD).  A permutation of who runs which span: no segment, slab
// slot or sum depends on it.  G * G < 2^32 (G <= U, U * (G + 1) < 2^31).
__host__ __device__ inline int bal_place(int b, int G, int d, int inv) {
  if (d == 0) return b;
  const uint32_t x = (uint32_t)b & 7u, k = (uint32_t)b >> 3, q = (uint32_t)G >> 3, rem = (uint32_t)G & 7u;
  const uint32_t r = x * q + (x < rem ? x : rem) + k;
  const uint32_t Gp = (uint32_t)G / (uint32_t)d;
  return (int)((r / (uint32_t)d) * (uint32_t)inv % Gp + (r % (uint32_t)d) * Gp);
}
// d and inv of bal_place for G workgroups over n_ft frame tiles (d = 0: identity)
inline void bal_place_params(int G, int n_ft, bool on, int* d, int* inv) {
  *d = 0, *inv = 0;
  if (!on || G <= 8 || n_ft <= 0) return;
  int a = n_ft, b = G;
  while (b) { const int t = a % b; a = b, b = t; }
  const int Gp = G / a, m = (n_ft / a) % Gp;
  int v = 0;   // Gp is small (<= G): search the inverse; Gp = 1 gives 0
  for (int c = 0; c < Gp; ++c)
    if ((long long)c * m % Gp == 1 % Gp) { v = c; break; }
  *d = a, *inv = v;
}
// Process-global switch of the placement (srf_route_dr_set_bal_placement); the default
// is the compile-time SRF_DR_BAL_XCD.  Read when a pass is launched (or captured).
void fwd32_set_bal_placement(bool on);
bool fwd32_bal_placement();

// The plan argument `n_chunks` of every entry point selects the split: 0 = the cost
// model's choice, 1 .. in_n = that many uniform i-chunks, kBalFlag | G = the balanced
// split over G workgroups (G = 0: as many as are resident).  srf_route_dr_auto_chunks
// returns the cost model's choice in this encoding, so the forward, the backward and both
// workspace queries decode the same plan from the same integer.
constexpr int kBalFlag = 1 << 20;

// The plan of the 32x32 passes has two parts.  The shape part is a function of the geometry
// alone: it lays out the operand planes, and through them the coupling storage that a
// forward writes and a backward (possibly under another plan argument) reads.  The split
// part is what the plan argument selects.  fwd32_cpl_layout, fwd32_planes_bytes and
// fwd32_hdr take a Fwd32Shape, so no layout can depend on a plan argument.
struct Fwd32Shape {
  int NW;              // waves per workgroup
  int TW;              // 32-row tiles per wave (kFwd32TW; 2 for din 32 with J*dout <= 512)
  int JDp;             // J*dout padded to NW*TW*32 rows
  int xpad;            // zero halves after each x plane (the invalid-frame row)
  int n_ftiles;        // 32-frame tiles
  size_t xplane;       // elements per x plane (data + zero row)
  size_t ws_w, ws_b, ws_x, ws_h;   // operand plane regions (bytes)
};
struct Fwd32Split {
  // uniform i-chunks: the iteration-0 pass and its bias sums always, the r >= 1 passes
  // unless the plan is balanced
  int n_chunks, chunk_len;
  int bal_G, bal_U;    // balanced r >= 1 passes: workgroups and units (bal_G = 0: chunked)
  int n_slots;         // slab slots a frame tile of the r >= 1 passes can use
  int plan_arg;        // the plan in the entry points' encoding (what auto_chunks returns)
  size_t ws_bsum, ws_slab;   // per-pass scratch regions (bytes)
};
struct Fwd32Plan : Fwd32Shape, Fwd32Split {};

bool fwd32_supported(int din, int dout, int J);
// n_chunks: the plan argument (above)
Fwd32Plan fwd32_plan(const DrGeom& g, int n_chunks = 0);
// Operand planes (split W, bias, x and their scale header: written by fwd32_prepare,
// read by every pass)
// and per-pass scratch (i-chunk bias sums + partial slabs) may live apart: a
// training forward keeps its planes for the backward (coupling storage).
size_t fwd32_planes_bytes(const Fwd32Shape& p);
size_t fwd32_scratch_bytes(const Fwd32Split& p);
size_t fwd32_workspace(const Fwd32Plan& p);   // planes + scratch
size_t fwd32_lds(const Fwd32Shape& p);
float* fwd32_slab(const Fwd32Split& p, void* scratch);
// the planes' scale header {2^-(aw+bx), aw, bx} (written by fwd32_prepare)
const float* fwd32_hdr(const Fwd32Shape& p, const void* planes);
// split W / emb into scaled fp16 planes, bias into bf16 planes, and the i-chunk bias
// sums (two launches per forward: absmax, prep);
// WT / xT (nullable): also the fp32 W^T [in_n][din][JD] and window^T [in_n][din][Fp]
// operands of the backward gx / gW contractions; wt16 (din 32): WT instead holds the
// split-fp16 A planes of route_gux16_kernel (same bytes); xt16 (din 32): xT instead
// holds route_gw16s_kernel's blocked split-fp16 B planes [in_n][Fp/16][2][din][16]
// (same bytes)
int fwd32_prepare(const Fwd32Plan& p, const DrGeom& g, const float* emb, const float* W, const float* bias,
                  void* planes, void* scratch, float* WT, float* xT, hipStream_t st, bool wt16 = false,
                  bool xt16 = false);
// one routing pass: partial s over i-chunks into fwd32_slab(p, scratch); passes r >= 1
// also store the couplings c^r (cst) when cst != nullptr.
int fwd32_pass(const Fwd32Plan& p, const DrGeom& g, bool first, const void* planes, void* scratch, const float* vc,
               float* cst, hipStream_t st);
// iteration 0 over all input capsules with the finish fused: writes s^0 (s_out),
// Vc^1 = v^0 (vc_out) and, for one-iteration layers, v (v_out); din = dout = 32
bool fwd32_first_full_supported(const Fwd32Shape& p, const DrGeom& g);
int fwd32_first_full(const Fwd32Plan& p, const DrGeom& g, const void* planes, void* scratch, float* s_out,
                     float* vc_out, float* v_out, hipStream_t st);
// Coupling storage of one training forward (float offsets): c^r [iters-1][in_n][JP][Fs],
// lz [iters-1][in_n][Fs], the operand planes, WT, xT; JP = JDp / dout,
// Fs = fwd32_frame_stride(F).  A function of the geometry alone (Fwd32Shape, above).
// lz once held logZ^r of the softmax over j.  No pass writes or reads it any more (the
// backward from stored couplings needs c^r alone); the region keeps its place so that
// every offset behind it, and srf_route_dr_coupling_floats, stay what they were.
struct Fwd32Cpl {
  size_t c, lz, planes, WT, xT, total;
};
Fwd32Cpl fwd32_cpl_layout(const Fwd32Shape& p, const DrGeom& g);
// one backward routing pass r >= 1 from the stored couplings: partial gVc^r over
// i-chunks into fwd32_slab(p, scratch) and the logit gradients gL^r (glst, laid out as
// the couplings) of the gx / gW passes
int bwd32_pass(const Fwd32Plan& p, const DrGeom& g, const void* planes, void* scratch, const float* cst,
               const float* gs, float* glst, hipStream_t st);

}  // namespace srf
