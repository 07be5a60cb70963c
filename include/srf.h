/* srf.h -- C ABI of the MI355X-native Sequential Routing Framework hot path.
 *
 * Every entry point takes caller-owned device pointers (fp32 unless stated),
 * plain int shapes and a hipStream_t passed as void*.  Nothing allocates and
 * nothing synchronises: calls are stream-ordered and may be captured into a
 * hipGraph.  One piece of process-wide state exists, set only by the caller: the
 * dropout step counter of srf_set_seed_source (below); every other call depends
 * on its arguments alone.  Return value: 0 on success, < 0 on error
 * (SRF_EINVAL -1 bad argument, SRF_EHIP -2 HIP error, SRF_EUNSUPPORTED -3,
 * SRF_EWORKSPACE -4); srf_last_error() then holds a thread-local message.
 *
 * Layouts (HBM):
 *   emb   [B*T][N][din]          capsules of one routing layer's input frames
 *   W     [in_n][J][dout][din]   in_n = N*(lpad+1+rpad); the reference variable
 *                                W%d of shape (1,1,in_n,J,dout,din)
 *   bias  [in_n][J][dout]        the reference b%d of shape (1,1,in_n,J,dout,1)
 *   v     [B*T][J][dout]
 */
#ifndef SRF_H_
#define SRF_H_
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Library identity / diagnostics. */
int srf_version(void);
const char* srf_last_error(void);

/* ---- Dynamic routing layer: window + pose transform + DR ------------------
 * Replaces tfsr/model/sequence_router_naive.py:149-185 (ZeroPadding2D+concat
 * window :150-151, tile+matmul pose :154-159, tf.while_loop DR :171-185 with
 * _loop_body :199-206) and, for the backward, its TF autodiff.
 * mask_first = 1 for the last layer (the -1e9 logit mask on capsule 0,
 * naive:173-178).  n_chunks is the plan argument: how the input capsules are
 * split over workgroups, either 1 .. in_n uniform chunks or the opaque value
 * srf_route_dr_auto_chunks returns (the tuned default; it may encode a balanced
 * split, and is > 1 whenever the work is split).
 * saved: 2*iters*B*T*J*dout floats written by the forward and read by the
 * backward (s^r and the accumulated agreement vector after each iteration;
 * the last plane, the vector after the last iteration, has no reader and is
 * not written by layers with more than one iteration). */
int srf_route_dr_auto_chunks(int B, int T, int N, int din, int lpad, int rpad, int J, int dout);
/* Host only (no device needed): the work split that plan argument n_chunks (0: the
 * default) gives the routing passes r >= 1 of a 32x32-pass shape.  info[5] =
 * {balanced, workgroups, units = frame tiles * in_n, slab slots per frame tile, the
 * plan argument in srf_route_dr_auto_chunks' encoding}; table receives up to `capacity`
 * rows {workgroup, frame tile, i0, i1, slab slot}, one per segment, in the order the
 * workgroups walk them.  Returns the number of segments (which may exceed capacity);
 * other shapes are an error. */
int srf_route_dr_split_table(int B, int T, int N, int din, int lpad, int rpad, int J, int dout, int n_chunks,
                             int* info, int* table, int capacity);
/* A balanced plan runs one persistent workgroup per span of srf_route_dr_split_table.
 * on != 0: the spans are placed on the XCDs by their capsule phase, so the workgroups
 * of an XCD read neighbouring W slabs and share them in its L2; 0: block b runs
 * workgroup b.  Process-global, read when a pass is launched (a captured graph keeps
 * what it was captured with); the default is the library's SRF_DR_BAL_XCD.  A
 * permutation of which block runs which span: every result is bit for bit the same
 * but g_emb, whose float atomics reorder.  Chunked plans are not affected. */
int srf_route_dr_set_bal_placement(int on);
/* Host only: the placement under the current setting.  block_to_wg receives, for up to
 * `capacity` blocks, the workgroup (row `workgroup` of the split table) that block b of
 * the pass grid runs.  Returns the number of workgroups G (which may exceed capacity),
 * 0 for a chunked plan, and a negative error where srf_route_dr_split_table does. */
int srf_route_dr_split_placement(int B, int T, int N, int din, int lpad, int rpad, int J, int dout, int n_chunks,
                                 int* block_to_wg, int capacity);
size_t srf_route_dr_saved_floats(int B, int T, int J, int dout, int iters);
size_t srf_route_dr_fwd_workspace(int B, int T, int N, int din, int lpad, int rpad, int J, int dout, int iters,
                                  int n_chunks);
size_t srf_route_dr_bwd_workspace(int B, int T, int N, int din, int lpad, int rpad, int J, int dout, int iters,
                                  int n_chunks);
int srf_route_dr_fwd(const float* emb, const float* W, const float* bias, int B, int T, int N, int din, int lpad,
                     int rpad, int J, int dout, int iters, int mask_first, int n_chunks, float* v_out,
                     float* saved, void* workspace, size_t workspace_bytes, void* stream);
/* Coupling storage (the 32x32 split-fp16 path: din in {8, 16, 32} <= dout in {8, 16, 32},
 * J*dout <= 1024; 0 for other shapes or iters < 2): the couplings c^r of the routing
 * iterations r >= 1 (and, at an unchanged offset and size, the region that once held
 * logZ^r: no longer written or read), written by srf_route_dr_fwd_ex when
 * couplings != NULL and read by srf_route_dr_bwd_ex / _bwd_data_ex, whose
 * backward routing passes then skip the logit and softmax recompute.  NULL
 * couplings: the plain entry points' behaviour (forward stores nothing, backward
 * recomputes).  Inference passes NULL. */
size_t srf_route_dr_coupling_floats(int B, int T, int N, int din, int lpad, int rpad, int J, int dout, int iters);
/* Where a training forward (couplings != NULL) leaves its prepared operands inside the
 * coupling storage; launches nothing.  out[SRF_DR_LAYOUT_N]: float offset and byte length
 * of Ws (0, 1), bs (2, 3), xs (4, 5), hdr (6, 7), WT (8, 9), xT (10, 11); JDp (12),
 * xplane (13), Fp (14); whether WT (15) / xT (16) hold the split-fp16 formats (1) or fp32
 * (0).  SRF_EUNSUPPORTED for a shape without coupling storage. */
#define SRF_DR_LAYOUT_N 17
int srf_route_dr_operand_layout(int B, int T, int N, int din, int lpad, int rpad, int J, int dout, int iters,
                                long long* out);
int srf_route_dr_fwd_ex(const float* emb, const float* W, const float* bias, int B, int T, int N, int din, int lpad,
                        int rpad, int J, int dout, int iters, int mask_first, int n_chunks, float* v_out,
                        float* saved, float* couplings, void* workspace, size_t workspace_bytes, void* stream);
int srf_route_dr_bwd_ex(const float* emb, const float* W, const float* bias, int B, int T, int N, int din, int lpad,
                        int rpad, int J, int dout, int iters, int mask_first, int n_chunks, const float* saved,
                        const float* couplings, const float* g_v, float* g_emb, float* g_W, float* g_bias,
                        void* workspace, size_t workspace_bytes, void* stream);
/* _bwd_weights of a backward whose _bwd_data_ex was given couplings: the same
 * saved and couplings buffers. */
int srf_route_dr_bwd_weights_ex(const float* emb, int B, int T, int N, int din, int lpad, int rpad, int J, int dout,
                                int iters, int mask_first, int n_chunks, const float* saved, const float* couplings,
                                float* g_W, float* g_bias, void* workspace, size_t workspace_bytes, void* stream);
int srf_route_dr_bwd_data_ex(const float* emb, const float* W, const float* bias, int B, int T, int N, int din,
                             int lpad, int rpad, int J, int dout, int iters, int mask_first, int n_chunks,
                             const float* saved, const float* couplings, const float* g_v, float* g_emb,
                             void* workspace, size_t workspace_bytes, void* stream);
/* Dropout step counter -- PROCESS-GLOBAL state: a device uint64 that every dropout
 * kernel launched afterwards, from any thread and for any model, mixes into its
 * seed (NULL restores the per-call seeds alone).  It lets a training step captured
 * into a hipGraph draw fresh masks on every replay: the step advances the counter
 * on the device.  Forward and backward of one step must see the same counter value
 * (the autograd backward runs on torch's device worker thread, hence process-wide,
 * not per thread).  One process drives one GPU, so the host keeps one counter per
 * process and never detaches it (srf_amd.trainer_sr.seed_counter). */
int srf_set_seed_source(const void* step_counter);
/* Fault word -- PROCESS-GLOBAL state like the step counter: a device uint32 that a
 * grouped SDR recurrence (srf_sdr_range.group > 1) sets to nonzero when a member gave
 * up waiting for the others (they were not resident together), i.e. when the launch's
 * results are wrong.  Kernels only set it; the caller reads and clears it at its next
 * synchronisation (srf_amd.ops.check_faults).  NULL: no reporting. */
int srf_set_fault_flag(void* flag);
/* Gradients are written (not accumulated): g_emb [B*T][N][din], g_W like W,
 * g_bias like bias. */
int srf_route_dr_bwd(const float* emb, const float* W, const float* bias, int B, int T, int N, int din, int lpad,
                     int rpad, int J, int dout, int iters, int mask_first, int n_chunks, const float* saved,
                     const float* g_v, float* g_emb, float* g_W, float* g_bias, void* workspace,
                     size_t workspace_bytes, void* stream);
/* The same backward in two stream-ordered parts.  _data writes g_emb and leaves the
 * gu blocks in the workspace; _weights (same workspace, same geometry) then writes
 * g_W and g_bias.  _weights depends on nothing else, so a caller may launch it on a
 * second stream that waits for _data, and join that stream before reading g_W /
 * g_bias or reusing the workspace: the weight contraction then overlaps the
 * backward of the layers below.  srf_route_dr_bwd = _data + _weights on one stream. */
int srf_route_dr_bwd_data(const float* emb, const float* W, const float* bias, int B, int T, int N, int din,
                          int lpad, int rpad, int J, int dout, int iters, int mask_first, int n_chunks,
                          const float* saved, const float* g_v, float* g_emb, void* workspace,
                          size_t workspace_bytes, void* stream);
int srf_route_dr_bwd_weights(const float* emb, int B, int T, int N, int din, int lpad, int rpad, int J, int dout,
                             int iters, int mask_first, int n_chunks, float* g_W, float* g_bias, void* workspace,
                             size_t workspace_bytes, void* stream);

/* ---- Sequential dynamic routing layer: window + pose transform + SDR -------
 * Replaces tfsr/model/sequence_router_naive.py:162-170 (tf.while_loop over the
 * frames) with body_context :231-245 and, for the last layer, pad_body_context
 * :212-229; and their TF autodiff.  Frames of an utterance are routed in order,
 * the previous frame's final v seeding the next frame's logits.  saved: the
 * per-frame v (srf_route_sdr_saved_floats), written by the forward, read by the
 * backward.  Returns SRF_EUNSUPPORTED when one frame's routing state exceeds a
 * CU's LDS. */
size_t srf_route_sdr_saved_floats(int B, int T, int J, int dout);
size_t srf_route_sdr_fwd_workspace(int B, int T, int N, int din, int lpad, int rpad, int J, int dout);
size_t srf_route_sdr_bwd_workspace(int B, int T, int N, int din, int lpad, int rpad, int J, int dout, int iters);
int srf_route_sdr_fwd(const float* emb, const float* W, const float* bias, int B, int T, int N, int din, int lpad,
                      int rpad, int J, int dout, int iters, int mask_first, float* v_out, float* saved,
                      void* workspace, size_t workspace_bytes, void* stream);
int srf_route_sdr_bwd(const float* emb, const float* W, const float* bias, int B, int T, int N, int din, int lpad,
                      int rpad, int J, int dout, int iters, int mask_first, const float* saved, const float* g_v,
                      float* g_emb, float* g_W, float* g_bias, void* workspace, size_t workspace_bytes,
                      void* stream);

/* ---- Batched frame ranges (the layer-pipelined SDR stack, ops.SdrStack): one launch
 * runs up to SRF_SDR_MAX_ITEMS frame ranges [t0, t1) of layers with the same shape
 * (one anti-diagonal of the stack's wavefront), instead of one HIP stream per layer.
 * Each entry point reads only its fields; the single-range functions below are the
 * n = 1 case.  Ranges with t0 == t1 are skipped (gW: one with accumulate == 0 still
 * zeroes its layer's gradient).  Replaces the per-layer loop of
 * sequence_router_naive.py:145-191 over the frames of :162-170. */
#define SRF_SDR_MAX_ITEMS 8
typedef struct {
  int t0, t1;                  /* frame range of every utterance */
  const float* emb;            /* layer input [B][T][N][din] (pose, gW) */
  const float* W;              /* pose: [in_n][J*dout][din] */
  const float* bias;           /* pose: [in_n][J*dout] */
  const float* WT;             /* gx: W^T [in_n][din][J*dout] */
  float* u;                    /* pose output / recurrence input, frames [v0, v0 + vn) */
  int v0, vn;
  float* v;                    /* recur_fwd: v_out; recur_bwd: the forward's v [B][T][J*dout] */
  float* couplings;            /* [B][T][srf_route_sdr_coupling_floats] or NULL */
  void* workspace;             /* srf_route_sdr_recur_workspace bytes, per range */
  size_t workspace_bytes;
  const float* g_v;            /* recur_bwd: dL/dv [B][T][J*dout] */
  float* carry;                /* recur_bwd: [B][J*dout] in / out */
  float* gu;                   /* recur_bwd output, gx / gW input: frames [g0, g0 + gn) */
  int g0, gn;
  float* g_emb;                /* gx: added into [B][T][N][din] */
  float* g_W;                  /* gW: [in_n][J*dout][din] */
  float* g_bias;               /* gW: [in_n][J*dout] */
  int accumulate;              /* gW: add to g_W / g_bias (else overwrite) */
  int u_bf16;                  /* u holds bf16 (written by pose_n mode 2; read by the streaming
                                  recurrence kernels only, i.e. srf_route_sdr_couplings_required) */
  int group;                   /* recur_fwd_n / recur_bwd_n on the streaming kernels: workgroups per
                                  utterance (0 or 1: one; at most 8, equal over a launch's ranges).
                                  A group splits the input capsules and adds its partial sums inside
                                  the launch, spin-waiting on its members: the launch's
                                  B * n * group workgroups must be resident together.  The library
                                  cannot see what else holds CUs: it refuses a launch above the
                                  device's CU count less 4, and the caller keeps other grouped
                                  launches, and kernels that occupy CUs for long (collectives),
                                  off the device meanwhile.  A member that waits too long stops
                                  and sets the fault word (srf_set_fault_flag): the results of
                                  that launch are then wrong.  The group's counters live in the
                                  workspace: it must be zero before the first grouped launch on
                                  it, and each grouped launch leaves its counters zero again
                                  (the timeout word excepted).  Other shapes ignore it. */
  int gu_factored;             /* recur_bwd_n on the register kernels with couplings (C3): gu holds
                                  each frame's gu factors (srf_route_sdr_fact_floats per frame)
                                  instead of gu; srf_route_sdr_gx_gw_fact_n reads them */
} srf_sdr_range;
/* pose_n fp8: 0 fp32 pose, 1 fp8 pose (fp32 u), 2 fp8 pose storing u in bf16 */
int srf_route_sdr_pose_n(const srf_sdr_range* ranges, int n, int B, int T, int N, int din, int lpad, int rpad, int J,
                         int dout, int fp8, void* stream);
int srf_route_sdr_recur_fwd_n(const srf_sdr_range* ranges, int n, int B, int T, int in_n, int J, int dout, int iters,
                              int mask_first, void* stream);
int srf_route_sdr_recur_bwd_n(const srf_sdr_range* ranges, int n, int B, int T, int in_n, int J, int dout, int iters,
                              int mask_first, void* stream);
int srf_route_sdr_gx_n(const srf_sdr_range* ranges, int n, int B, int T, int N, int din, int lpad, int rpad, int J,
                       int dout, void* stream);
int srf_route_sdr_gw_n(const srf_sdr_range* ranges, int n, int B, int T, int N, int din, int lpad, int rpad, int J,
                       int dout, void* stream);
/* gx_n and gw_n of the same ranges in one launch that reads gu once (din 32; other
 * shapes run the two entry points above).  Reads W (not WT) besides their fields. */
int srf_route_sdr_gx_gw_n(const srf_sdr_range* ranges, int n, int B, int T, int N, int din, int lpad, int rpad,
                          int J, int dout, void* stream);
/* The same from the recurrence's gu factors (ranges with gu_factored, whose recur_bwd_n
 * wrote srf_route_sdr_fact_floats per frame into gu): gu_ij = sum_r c^r_ij gs^r_j +
 * gL^r_ij Vc^r_j is formed inside the contraction with the forward's couplings, so gu
 * never crosses HBM.  din = dout = 32, J a multiple of 8, iters <= 3.  Reads couplings,
 * gu (the factors), W, emb; writes as gx_gw_n. */
int srf_route_sdr_gx_gw_fact_n(const srf_sdr_range* ranges, int n, int B, int T, int N, int din, int lpad, int rpad,
                               int J, int dout, int iters, void* stream);

/* ---- The SDR layer in frame ranges (the layer-pipelined SDR stack) ----------
 * srf_route_sdr_fwd/bwd split into calls over frames [t0, t1) of every utterance,
 * so a host can run an SDR stack as a wavefront over (layer, frame range): layer
 * l's range k needs only layer l-1's output up to frame t1 - 1 + rpad (the window,
 * naive:150-151), and, going backward, layer l+1's gx down to frame t0 - rpad.
 * Same arithmetic as the whole-layer calls (naive:162-170, 212-245 and autodiff).
 *   u / gu buffers hold frames [v0, v0 + vn) / [g0, g0 + gn) of each utterance,
 *   laid out [B][vn][in_n][J*dout] (v0 = 0, vn = T: the whole layer);
 *   v_out, v_saved, g_v are whole [B][T][J*dout];
 *   recur_fwd starts from v_out[t0 - 1] (0 at t0 = 0): earlier ranges first;
 *   recur_bwd walks t1-1 .. t0, carry [B][J*dout] holds dL/dv_{t1-1} on entry
 *   (zero it before the last range) and dL/dv_{t0-1} on return: later ranges first;
 *   gx adds W^T gu of the range's frames into g_emb through the window adjoint
 *   (zero g_emb first); gw writes (accumulate = 0) or adds the range's
 *   gW = sum_f gu x^T and g_bias = sum_f gu.
 * recur_workspace: state slices for shapes beyond the register / LDS budget (0 else). */
int srf_route_sdr_pose(const float* emb, const float* W, const float* bias, int B, int T, int N, int din, int lpad,
                       int rpad, int J, int dout, int t0, int t1, float* u, int v0, int vn, void* stream);
/* The same on fp8 (OCP e4m3) MFMA, opt-in (BASELINE C5 "fp8 pose-transform MFMA"): x
 * per frame and W per row scaled by powers of two into e4m3 range, fp32 accumulation,
 * fp32 bias.  Bound per element: |u - u_exact| <= 0.13 * sum_k |W_rk| |x_k| (+ fp32
 * rounding).  in_d 32 or 64. */
int srf_route_sdr_pose_fp8(const float* emb, const float* W, const float* bias, int B, int T, int N, int din, int lpad,
                           int rpad, int J, int dout, int t0, int t1, float* u, int v0, int vn, void* stream);
size_t srf_route_sdr_recur_workspace(int B, int in_n, int J, int dout, int iters);
/* The part of that workspace that must be zero before its first grouped launch (the
 * group counters and the timeout word, srf_sdr_range.group): *offset_bytes from the
 * workspace's start, the return value its length in bytes.  The rest (kernel scratch,
 * exchange area) needs no initialisation.  Shapes on the LDS / global-state kernels
 * return the whole workspace. */
size_t srf_route_sdr_recur_zero_range(int B, int in_n, int J, int dout, int iters, size_t* offset_bytes);
/* Coupling storage per frame (0 when the shape runs on the LDS / global-state
 * kernels): with couplings != NULL ([B][T][this many floats]) recur_fwd stores each
 * frame's couplings c^r and pre-squash s^r, and recur_bwd reads them instead of
 * recomputing the frame's iterations (NULL: recompute).  Shapes on the streaming
 * kernels (frames beyond the register budget, e.g. BASELINE C5) have no recompute
 * path: srf_route_sdr_couplings_required is 1 and recur_bwd needs them. */
size_t srf_route_sdr_coupling_floats(int in_n, int J, int dout, int iters);
int srf_route_sdr_couplings_required(int in_n, int J, int dout, int iters);
/* Floats of one frame's gu factors (srf_sdr_range.gu_factored): gL^r [iters][in_n][JP],
 * gs^r and Vc^r [iters][J*dout] each (JP = J rounded up to a power of two, at least 4);
 * 0 where the layer's backward cannot write them (no register kernel for the shape). */
size_t srf_route_sdr_fact_floats(int in_n, int J, int dout, int iters);
int srf_route_sdr_recur_fwd(const float* u, int v0, int vn, int B, int T, int in_n, int J, int dout, int iters,
                            int mask_first, int t0, int t1, float* v_out, float* couplings, void* workspace,
                            size_t workspace_bytes, void* stream);
int srf_route_sdr_recur_bwd(const float* u, int v0, int vn, const float* v_saved, const float* couplings,
                            const float* g_v, int B, int T, int in_n, int J, int dout, int iters, int mask_first,
                            int t0, int t1, float* carry, float* gu, int g0, int gn, void* workspace,
                            size_t workspace_bytes, void* stream);
/* W [in_n][J*dout][din] -> WT [in_n][din][J*dout] (the gx operand). */
int srf_route_sdr_transpose_w(const float* W, int in_n, int J, int dout, int din, float* WT, void* stream);
int srf_route_sdr_gx(const float* gu, int g0, int gn, const float* WT, int B, int T, int N, int din, int lpad,
                     int rpad, int J, int dout, int t0, int t1, float* g_emb, void* stream);
int srf_route_sdr_gw(const float* gu, int g0, int gn, const float* emb, int B, int T, int N, int din, int lpad,
                     int rpad, int J, int dout, int t0, int t1, int accumulate, float* g_W, float* g_bias,
                     void* stream);

/* ---- CNN front end (CapsulationLayer, tfsr/model/sequence_router.py:44-82) ---
 * feats [B][T][feat_dim] fp32 (already cropped to max(inp_len), trainer_sr.py:59-60),
 * inp_len [B] int32 (device).  Kernels [3][3][Cin][64] (kh, kw, cin, cout), as the
 * reference's Conv2D variables; biases/gamma/beta [64].  The two convolutions of
 * each stage are the reference's conv_layers[0][k] and conv_layers[1][k]
 * (sequence_router.py:76-77).  out = mask2(BN2(.)) [B][T2][F2][64] with
 * T2 = ceil(ceil(T/2)/2), F2 = ceil(ceil(feat_dim/2)/2) (srf_cnnfe_out_dims).
 * training = 1: batch statistics, moving statistics updated in place (momentum
 * 0.99), dropout drop_p on every conv output; training = 0: moving statistics,
 * no dropout.  Dropout masks are a pure function of (seed, element), so
 * srf_cnnfe_bwd regenerates them.  nfilt must be 64. */
int srf_cnnfe_out_dims(int T, int feat_dim, int* T2, int* F2);
size_t srf_cnnfe_saved_bytes(int B, int T, int feat_dim, int nfilt);
size_t srf_cnnfe_fwd_workspace(int B, int T, int feat_dim, int nfilt);
size_t srf_cnnfe_bwd_workspace(int B, int T, int feat_dim, int nfilt);
int srf_cnnfe_fwd(const float* feats, const int* inp_len, int B, int T, int feat_dim, int nfilt,
                  const float* k0a, const float* b0a, const float* k0b, const float* b0b, const float* gamma0,
                  const float* beta0, const float* k1a, const float* b1a, const float* k1b, const float* b1b,
                  const float* gamma1, const float* beta1, float* mmean0, float* mvar0, float* mmean1, float* mvar1,
                  int training, float drop_p, unsigned long long seed, float* out, void* saved, size_t saved_bytes,
                  void* workspace, size_t workspace_bytes, void* stream);
/* Gradients (written) of every CNN-FE parameter from g_out = dL/d out. */
int srf_cnnfe_bwd(const float* feats, const int* inp_len, int B, int T, int feat_dim, int nfilt, const float* gamma0,
                  const float* k1a, const float* k1b, const float* gamma1, float drop_p, unsigned long long seed,
                  const void* saved, const float* g_out, float* g_k0a, float* g_b0a, float* g_k0b, float* g_b0b,
                  float* g_gamma0, float* g_beta0, float* g_k1a, float* g_b1a, float* g_k1b, float* g_b1b,
                  float* g_gamma1, float* g_beta1, void* workspace, size_t workspace_bytes, void* stream);

/* The same backward in parts (bit mask), for a caller that runs the stage-2 weight
 * gradient on a second stream: PREP (BN2 sums, the stage-2 output gradient g_ab and
 * the bias gradients) first; then DATA (stage-2 data gradient, BN1, stage 1) and WGRAD
 * (stage-2 kernel gradients) both read what PREP wrote and nothing of each other, so
 * they may run concurrently after it.  One workspace for all parts.  ALL = the
 * sequential srf_cnnfe_bwd. */
#define SRF_CNNFE_BWD_PREP 1
#define SRF_CNNFE_BWD_DATA 2
#define SRF_CNNFE_BWD_WGRAD 4
#define SRF_CNNFE_BWD_ALL 7
int srf_cnnfe_bwd_parts(int parts, const float* feats, const int* inp_len, int B, int T, int feat_dim, int nfilt,
                        const float* gamma0, const float* k1a, const float* k1b, const float* gamma1, float drop_p,
                        unsigned long long seed, const void* saved, const float* g_out, float* g_k0a, float* g_b0a,
                        float* g_k0b, float* g_b0b, float* g_gamma0, float* g_beta0, float* g_k1a, float* g_b1a,
                        float* g_k1b, float* g_b1b, float* g_gamma1, float* g_beta1, void* workspace,
                        size_t workspace_bytes, void* stream);

/* ---- Primary capsules (sequence_router_naive.py:129-142) -------------------
 * X = CNN-FE output viewed as [B*T][K] (K = F2*64, index f*64 + c as the
 * reference's reshape, :131); Wp [K][PH], bp [PH]; encaps kernels [3][3][1][PD],
 * biases [PD]; LN gamma/beta [PH*PD].  z [B*T][PH][PD] =
 * drop_in(LN(squash_PD(mask(max(drop(encaps1(e)), drop(encaps2(e))))))).
 * p_caps is the hard-coded 0.2 of naive:82, p_in = --train-inp-dropout. */
size_t srf_primary_caps_saved_bytes(int B, int T, int PH, int PD);
size_t srf_primary_caps_bwd_workspace(int B, int T, int K, int PH, int PD);
int srf_primary_caps_fwd(const float* X, const int* inp_len, int B, int T, int K, int PH, int PD, const float* Wp,
                         const float* bp, const float* K1, const float* b1, const float* K2, const float* b2,
                         const float* gamma, const float* beta, int training, float p_caps, float p_in,
                         unsigned long long seed, float* z, void* saved, size_t saved_bytes, void* stream);
int srf_primary_caps_bwd(const float* X, const int* inp_len, int B, int T, int K, int PH, int PD, const float* Wp,
                         const float* K1, const float* K2, const float* gamma, const float* beta, int training,
                         float p_caps, float p_in, unsigned long long seed, const void* saved, const float* g_z,
                         float* g_X, float* g_Wp, float* g_bp, float* g_K1, float* g_b1, float* g_K2, float* g_b2,
                         float* g_gamma, float* g_beta, void* workspace, size_t workspace_bytes, void* stream);
/* The einsum variant (sequence_router_einsum.py:129-131): e = (X Wp + bp) * proj_scale
 * (+ get_pos_enc(T, PH), model_helper.py:30-58, when pos_enc != 0; PH even, >= 4)
 * before the encaps convs.  The plain entry points are proj_scale = 1, pos_enc = 0
 * (naive and lowmemory, naive:131-132 / lowmemory:133-135). */
int srf_primary_caps_fwd_ex(const float* X, const int* inp_len, int B, int T, int K, int PH, int PD, const float* Wp,
                            const float* bp, const float* K1, const float* b1, const float* K2, const float* b2,
                            const float* gamma, const float* beta, int training, float p_caps, float p_in,
                            unsigned long long seed, float proj_scale, int pos_enc, float* z, void* saved,
                            size_t saved_bytes, void* stream);
int srf_primary_caps_bwd_ex(const float* X, const int* inp_len, int B, int T, int K, int PH, int PD, const float* Wp,
                            const float* K1, const float* K2, const float* gamma, const float* beta, int training,
                            float p_caps, float p_in, unsigned long long seed, float proj_scale, const void* saved,
                            const float* g_z, float* g_X, float* g_Wp, float* g_bp, float* g_K1, float* g_b1,
                            float* g_K2, float* g_b2, float* g_gamma, float* g_beta, void* workspace,
                            size_t workspace_bytes, void* stream);

/* ---- Per-layer LayerNorm + dropout and the output head (naive:187-193) -----
 * capsnorm: y = drop(LN(x)) per frame over n = J*D (ln_mid%d + dropout_mid_%d);
 * head: logits[F][J] = LN_out(length_D(drop(LN_mid(v)))), lens[F][J] saved.
 * stat [F][4] is written by the forward and read by the backward. */
size_t srf_capsnorm_bwd_workspace(int F, int n, int J);
int srf_capsnorm_fwd(const float* x, int F, int n, const float* gamma, const float* beta, int training, float p,
                     unsigned long long seed, int layer, float* y, float* stat, void* stream);
int srf_capsnorm_bwd(const float* x, int F, int n, const float* gamma, const float* beta, int training, float p,
                     unsigned long long seed, int layer, const float* stat, const float* g_y, float* g_x,
                     float* g_gamma, float* g_beta, void* workspace, size_t workspace_bytes, void* stream);
/* capsnorm over the rows (b, t), t in [t0, t1), of every utterance of a [B][T] batch
 * (same masks and arithmetic as the whole call).  The backward writes g_x rows and
 * gpart rows [B*T][2n] (per-row gamma / beta gradient terms); once every range is
 * done, srf_capsnorm_bwd_params sums gpart into g_gamma / g_beta. */
int srf_capsnorm_fwd_range(const float* x, int B, int T, int t0, int t1, int n, const float* gamma, const float* beta,
                           int training, float p, unsigned long long seed, int layer, float* y, float* stat,
                           void* stream);
int srf_capsnorm_bwd_range(const float* x, int B, int T, int t0, int t1, int n, const float* gamma, const float* beta,
                           int training, float p, unsigned long long seed, int layer, const float* stat,
                           const float* g_y, float* g_x, float* gpart, void* stream);
/* The ranges of up to SRF_CAPSNORM_MAX_ITEMS same-width layers (n = J*D) in one launch
 * (the layer-pipelined SDR stack's inner layers, one anti-diagonal at a time): the
 * *_range calls above for each entry, non-head (ln_mid%d + dropout_mid_%d of `layer`).
 * The forward reads x / gamma / beta, writes y / stat; the backward reads x / gamma /
 * beta / stat / g_y, writes g_x / gpart.  Empty ranges are skipped. */
#define SRF_CAPSNORM_MAX_ITEMS 8
typedef struct {
  int t0, t1, layer;
  const float* x;
  const float* gamma;
  const float* beta;
  float* y;
  float* stat;
  const float* g_y;
  float* g_x;
  float* gpart;
} srf_capsnorm_range;
int srf_capsnorm_fwd_range_n(const srf_capsnorm_range* ranges, int n_ranges, int B, int T, int n, int training,
                             float p, unsigned long long seed, void* stream);
int srf_capsnorm_bwd_range_n(const srf_capsnorm_range* ranges, int n_ranges, int B, int T, int n, int training,
                             float p, unsigned long long seed, void* stream);
size_t srf_capsnorm_params_workspace(int F, int n);
int srf_capsnorm_bwd_params(const float* gpart, int F, int n, float* g_gamma, float* g_beta, void* workspace,
                            size_t workspace_bytes, void* stream);
int srf_caps_head_fwd(const float* v, int F, int J, int D, const float* gamma_mid, const float* beta_mid,
                      const float* gamma_out, const float* beta_out, int training, float p, unsigned long long seed,
                      int layer, float* logits, float* stat, float* lens, void* stream);
/* length_eps of the output length: 1e-7 for naive / lowmemory (naive:256,
 * sequence_router.py:39), 1e-9 for einsum (sequence_router_einsum.py:238).  The
 * backward reads the saved lens, so it is the same for every variant. */
int srf_caps_head_fwd_ex(const float* v, int F, int J, int D, const float* gamma_mid, const float* beta_mid,
                         const float* gamma_out, const float* beta_out, int training, float p, unsigned long long seed,
                         int layer, float length_eps, float* logits, float* stat, float* lens, void* stream);
int srf_caps_head_bwd(const float* v, int F, int J, int D, const float* gamma_mid, const float* beta_mid,
                      const float* gamma_out, int training, float p, unsigned long long seed, int layer,
                      const float* stat, const float* lens, const float* g_logits, float* g_v, float* g_gamma_mid,
                      float* g_beta_mid, float* g_gamma_out, float* g_beta_out, void* workspace,
                      size_t workspace_bytes, void* stream);

/* ---- CTC (tf.nn.ctc_loss at trainer_sr.py:64-66) ---------------------------
 * logits [B][Tmax][C] batch-major, labels [B][Lmax] int32 (dense, padded),
 * label_len / logit_len [B] int32 (logit_len = ceil(inp_len/4)).  nll [B]; if
 * grad != NULL also d(grad_scale * nll_b)/d logits [B][Tmax][C] (zero past
 * logit_len; zero for an infeasible utterance, whose nll is +inf). */
size_t srf_ctc_workspace(int B, int Tmax, int C, int Lmax);
int srf_ctc_loss(const float* logits, const int* labels, const int* label_len, const int* logit_len, int B, int Tmax,
                 int C, int Lmax, int blank, float grad_scale, float* nll, float* grad, void* workspace,
                 size_t workspace_bytes, void* stream);
/* srf_ctc_align: CTC forced alignment (Viterbi) of the given labels, same calling
 * convention as srf_ctc_loss (T_b = min(logit_len[b], Tmax)).  With lp = log_softmax in
 * fp32 and the extended label of S = 2 L_b + 1 states (even: blank, 2k + 1: label k), the
 * result is the path that starts in state 0 or 1, ends in S - 1 or S - 2, moves by 0 or
 * +1 per frame, by +2 only into a label state whose label differs from the label two
 * states back, and maximises the sum of lp[t, ext[state_t]]; score [B] is that sum.
 * Ties: among equal predecessors the lowest source state wins (+2 before +1 before
 * stay); at the last frame S - 2 unless S - 1 is strictly larger.
 * states [B][Tmax]: the state per frame, -1 for t >= T_b.  tok_start / tok_end [B][Lmax]:
 * first frame of label k's run and one past its last, -1 for k >= L_b.  tok_logp
 * [B][Lmax]: sum of lp over label k's frames, 0 where there is no label.  T_b = 0 with
 * L_b = 0 scores 0; L_b = 0 keeps every frame in state 0; an infeasible utterance (T_b
 * too short for its labels) scores -inf and all its other outputs are -1 / 0.  The token
 * outputs and labels may be NULL when Lmax = 0.  workspace: 16-byte aligned. */
size_t srf_ctc_align_workspace(int B, int Tmax, int C, int Lmax);
int srf_ctc_align(const float* logits, const int* labels, const int* label_len, const int* logit_len, int B, int Tmax,
                  int C, int Lmax, int blank, int* states, int* tok_start, int* tok_end, float* tok_logp, float* score,
                  void* workspace, size_t workspace_bytes, void* stream);

/* ---- Scoring (the label error rate of an evaluation) ------------------------
 * srf_edit_align: Levenshtein alignment, with a backtrace, of B hypotheses hyp [B][Hmax]
 * against B references ref [B][Rmax] (int32 labels, dense, padded), hyp_len / ref_len [B]
 * int32 clamped to [0, Hmax] / [0, Rmax]; entries past a length are never read.  All
 * results are integers, so every output bit is defined.
 * Fold (fold != NULL, fold [n_fold] int32): a label x becomes fold[x]; a label with
 * fold[x] < 0 or x outside [0, n_fold) is dropped.  Both sequences are folded and
 * compacted before the alignment (repeats are not merged); h [0, H) and r [0, R) are what
 * is left.  fold = NULL (then n_fold = 0): labels are compared as they are.
 * Distance: D[i][0] = i, D[0][j] = j, D[i][j] = min(D[i-1][j-1] + (h[i-1] != r[j-1]),
 * D[i][j-1] + 1, D[i-1][j] + 1).  Backtrace: from (H, R), at every cell the first step
 * that is consistent with D among (1) the diagonal, a correct label or a substitution,
 * (2) the deletion (i, j) -> (i, j-1), a reference label without a hypothesis label,
 * (3) the insertion (i, j) -> (i-1, j); i.e. on equal values the diagonal wins, then the
 * deletion, then the insertion.  h = [1, 2], r = [2, 1] is two substitutions;
 * h = [1, 1, 2], r = [1, 2] inserts h[0]; h = [1, 2], r = [1, 1, 2] deletes r[0].
 * counts [B][6]: D[H][R], substitutions, deletions, insertions, R, H.
 * hyp_to_ref [B][Hmax], ref_to_hyp [B][Rmax], indexed by the positions before the fold:
 * the position (before the fold) of the partner for a correct or substituted label, -1
 * for an inserted / deleted label, -2 for a label the fold dropped and for a position
 * past the utterance's length.  Either map may be NULL.
 * Accumulators, both optional and added to with 64-bit integer atomics (the caller zeroes
 * them; the sums do not depend on the order): totals [8] = the sums of the six counts,
 * the number of utterances, the number of utterances with D[H][R] > 0.  confusion
 * [K + 1][K + 1] (1 <= K <= 32767), row the reference class and column the hypothesis
 * class after the fold: the diagonal holds the correct labels, column K the deletions,
 * row K the insertions, [K][K] stays 0; a pair with a class outside [0, K) is left out
 * of confusion and still counts in totals.  Without confusion K is not used (K >= 0).
 * 0 <= Hmax, Rmax <= 8192, B >= 1; anything else is refused before any launch (the
 * workspace query then returns 0 and leaves a message).  workspace: 16-byte aligned,
 * srf_edit_align_workspace bytes (never 0 for a legal shape). */
size_t srf_edit_align_workspace(int B, int Hmax, int Rmax);
int srf_edit_align(const int* hyp, const int* hyp_len, int Hmax, const int* ref, const int* ref_len, int Rmax, int B,
                   const int* fold, int n_fold, int* counts, int* hyp_to_ref, int* ref_to_hyp, long long* totals,
                   long long* confusion, int K, void* workspace, size_t workspace_bytes, void* stream);
/* Words: a character model's labels cut at a separator label, and srf_edit_align's
 * alignment over words instead of labels (the word error rate).  Everything is an integer
 * except word_logp, so every output bit is defined.
 * A dense int32 label row x[0, n), n = clamp(len, 0, Lmax); entries past n are never read.
 * Position p is a separator if x[p] == sep (the raw label is tested before the fold, so a
 * separator stays one whatever the fold says about it).  Otherwise, with a fold (fold
 * [n_fold], srf_edit_align's table), p is dropped if x[p] is outside [0, n_fold) or
 * fold[x[p]] < 0, else kept with class fold[x[p]]; without a fold p is kept with class x[p].
 * A word is a maximal run of kept labels between separators: a dropped label neither
 * splits a word nor adds to it (with n dropped, A n B is the word AB), and a run without a
 * kept label is no word, so leading, trailing and repeated separators make none.  Word k,
 * in order of appearance: start = the position (before the fold) of its first kept label,
 * end = one past the position of its last, len = its kept labels.  At most (Lmax + 1) / 2.
 * Two words are equal iff they have equal len and equal classes at every index (exact: a
 * hash may only filter).  Ids: with the utterance's reference words r_0 .. r_{R-1}
 * followed by its hypothesis words h_0 .. h_{H-1} as one list, a word's id is the index in
 * that list of the first word equal to it: id(r_j) <= j; id(h_i) is a reference index if
 * a reference word equals h_i, else R + i' for the first equal hypothesis word h_i'.
 * The word alignment is srf_edit_align's definition on the two id rows: the same D, the
 * same ties (diagonal, deletion, insertion), counts with R and H counted in words.
 *
 * srf_word_split: word_start / word_end [B][(Lmax + 1) / 2], -1 past word_count [B].
 * tok_start / tok_end / tok_logp [B][Lmax] are srf_ctc_align's outputs for the same
 * labels, all three or none.  With them word_frame_start = tok_start[start],
 * word_frame_end = tok_end[end - 1], word_logp = the fp32 sum of tok_logp[p] over p in
 * [start, end) in increasing p (one lane, sequentially: a float32 loop gives the same
 * bits); -1 / -1 / 0 past the count and for an infeasible utterance (tok_start -1).
 * Without them the three frame outputs are NULL.
 *
 * srf_word_align: counts [B][6] (required) and totals [8] (optional, 64-bit atomics) as
 * srf_edit_align's, in words.  The per-word arrays, [B][(Hmax + 1) / 2] and
 * [B][(Rmax + 1) / 2], hold -1 past the count; hyp_to_ref / ref_to_hyp, of the same
 * widths and over word indices, hold -2 past the count and -1 for an inserted / deleted
 * word.  Each per-word array may be NULL.  Two launches on the stream (the segmentation
 * with the ids, then srf_edit_align's kernel on the ids), no host synchronisation and no
 * allocation.  The id step compares a word with the words before it and is quadratic in
 * the word count at worst.
 * 0 <= Lmax, Hmax, Rmax <= 8192, B >= 1; anything else is refused before any launch (the
 * workspace query then returns 0 and leaves a message).  workspace: 16-byte aligned, the
 * query's bytes (never 0 for a legal shape). */
size_t srf_word_split_workspace(int B, int Lmax);
int srf_word_split(const int* labels, const int* label_len, int Lmax, int B, const int* fold, int n_fold, int sep,
                   int* word_start, int* word_end, int* word_count, const int* tok_start, const int* tok_end,
                   const float* tok_logp, int* word_frame_start, int* word_frame_end, float* word_logp,
                   void* workspace, size_t workspace_bytes, void* stream);
size_t srf_word_align_workspace(int B, int Hmax, int Rmax);
int srf_word_align(const int* hyp, const int* hyp_len, int Hmax, const int* ref, const int* ref_len, int Rmax, int B,
                   const int* fold, int n_fold, int sep, int* counts, int* hyp_word_start, int* hyp_word_end,
                   int* hyp_word_id, int* ref_word_start, int* ref_word_end, int* ref_word_id, int* hyp_to_ref,
                   int* ref_to_hyp, long long* totals, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Chunked streaming inference (srf_amd/streaming.py) --------------------
 * srf_ctc_greedy_n: best-path decoding (per-frame arg-max, repeats merged, blanks
 * dropped; trainer_sr.py's greedy hypothesis) of one chunk of logits [B][n][C], of which
 * the first n_valid[b] frames of stream b count (clamped to [0, n]).  prev [B] is read
 * and written: the arg-max of the stream's last decoded frame, -1 before its first, so a
 * label that repeats across a chunk edge is merged.  labels [B][n] receives each
 * stream's new labels compacted to the front, count [B] how many.  On equal logits the
 * lowest class index wins (torch.argmax).  One wave per stream; any C >= 2, n >= 0. */
int srf_ctc_greedy_n(const float* logits, const int* n_valid, int B, int n, int C, int blank, int* prev, int* labels,
                     int* count, void* stream);
/* srf_ctc_greedy_frames_n: srf_ctc_greedy_n with one more output, frames [B][n]:
 * frames[b][i] = frame0 + f for the chunk frame f at which labels[b][i] was emitted, the
 * first frame of its arg-max run (a run that continues across a chunk edge was emitted in
 * the earlier chunk).  labels, count and prev are those of srf_ctc_greedy_n. */
int srf_ctc_greedy_frames_n(const float* logits, const int* n_valid, int B, int n, int C, int blank, int frame0,
                            int* prev, int* labels, int* frames, int* count, void* stream);
/* srf_ctc_beam_*: CTC prefix beam search on the device (tf.nn.ctc_beam_search_decoder
 * with top_paths = 1 as process_test_step calls it; the algorithm of srf_ctc_beam_search
 * in srf_data.h, which defines the result), batched and resumable: one workgroup per
 * utterance, all frames of a chunk in one launch, the beam kept on the device between
 * chunks.  1 <= beam_width <= SRF_CTC_BEAM_MAX_WIDTH, 2 <= C <= SRF_CTC_BEAM_MAX_CLASSES,
 * 0 <= blank < C; anything else is refused.
 *
 * state: one opaque device block of srf_ctc_beam_state_bytes(B, C, beam_width,
 * max_frames) bytes (4-byte aligned; 0 and a message if the shape is refused).  Per
 * utterance it holds the beam (at most beam_width entries: trie node, log p(ends in
 * blank), log p(ends in a label), last label, length, a 64-bit hash of the label
 * sequence and of its parent's, by which a prefix finds its parent), the prefix trie as
 * (parent, label) arrays of 1 + max_frames * beam_width nodes (a node is appended only
 * for a prefix that survives a frame) and the frame count.  frames_pushed is a host
 * counter the caller keeps with the block: reset zeroes it, push adds n to it.
 *
 * reset: every utterance back to the single empty prefix (pb = 0, pnb = -inf).
 * push_n: logits [B][n][C], n_valid [B] (device); consumes the first clamp(n_valid[b], 0,
 * n) frames of utterance b.  n = 0 is legal and launches nothing.  A push with
 * *frames_pushed + n > max_frames is refused (SRF_EINVAL) and nothing runs.  The state
 * after a frame depends on the state before it and the frame only, so any chunking of
 * the same frames gives the same bits.
 * best: the most probable prefix of each utterance: labels [B][max_frames] (the first
 * count[b] are written), count [B], log_prob [B] = log(p_b + p_nb).  The state is not
 * changed, so it may be called between pushes. */
#define SRF_CTC_BEAM_MAX_WIDTH 128
#define SRF_CTC_BEAM_MAX_CLASSES 128
size_t srf_ctc_beam_state_bytes(int B, int C, int beam_width, int max_frames);
int srf_ctc_beam_reset(void* state, size_t state_bytes, int B, int C, int beam_width, int max_frames,
                       int* frames_pushed, void* stream);
int srf_ctc_beam_push_n(void* state, size_t state_bytes, int B, int C, int beam_width, int max_frames, int blank,
                        const float* logits, const int* n_valid, int n, int* frames_pushed, void* stream);
int srf_ctc_beam_best(const void* state, size_t state_bytes, int B, int C, int beam_width, int max_frames, int* labels,
                      int* count, float* log_prob, void* stream);
/* srf_ctc_beam_nbest: the N most probable prefixes of each utterance in the beam's own
 * rank order (total descending, then creation key ascending); row 0 is srf_ctc_beam_best's
 * result bit for bit.  labels [B][N][max_len] (the first count entries of a row are
 * written), count [B][N], log_prob [B][N] = log(p_b + p_nb), n_hyp [B] = min(N, beam
 * entries).  Rows >= n_hyp[b] get count = 0 and log_prob = -inf.  A prefix longer than
 * max_len gets count = -1 and no labels (its log_prob is set); max_len = max_frames
 * always suffices.  One lane per (utterance, hypothesis) walks the trie; the state is not
 * changed, so it may be called between pushes.  Refused before any launch unless
 * 1 <= N <= beam_width and max_len >= 1. */
int srf_ctc_beam_nbest(const void* state, size_t state_bytes, int B, int C, int beam_width, int max_frames, int N,
                       int max_len, int* labels, int* count, float* log_prob, int* n_hyp, void* stream);
/* srf_ctc_beam_lm_*: the same search with a language model fused into the beam (shallow
 * fusion; srf_ctc_beam_search_lm in srf_data.h defines the result).  The model is a
 * deterministic automaton over the classes in two device tables of n_states rows:
 *   bonus [n_states][C] float32, finite: what extending a prefix in state s by class c adds
 *     to its score (alpha * log p_lm(c | s) + beta; the blank's column is never read),
 *   next [n_states][C] int32 in [0, n_states): the state after that extension;
 * state 0 belongs to the empty prefix.  The one change to the search: the extension of a
 * prefix in state s by class c is
 *   pnb'(l + c) = ((c == last ? pb : tot) + lp[c]) + bonus[s][c]      (fp32, in this order),
 * also where an entry folds in its parent's extension (with the parent's state); the blank
 * and repeat steps add nothing.  The ranking score is log p_ctc(prefix) + the sum of the
 * prefix's bonuses; keys, tie rule, selection and hashing are those of srf_ctc_beam_*.
 *
 * The state block has its own size (srf_ctc_beam_lm_state_bytes: two more beam arrays, the
 * entry's state and its accumulated bonus) and is not interchangeable with the unfused
 * one; reset, push_n, best and nbest take the arguments of their unfused namesakes.
 * push_n also takes the tables and is refused for a null table, n_states < 1 or
 * n_states * C >= 2^31; the same tables belong to every push between two resets.  The
 * kernel clamps states to [0, n_states), so no table content makes it read outside the
 * tables.  best / nbest: score is the ranking score, lm_score ([B], [B][N]) the
 * accumulated bonus of that prefix (0 past n_hyp), their difference its CTC part. */
size_t srf_ctc_beam_lm_state_bytes(int B, int C, int beam_width, int max_frames);
int srf_ctc_beam_lm_reset(void* state, size_t state_bytes, int B, int C, int beam_width, int max_frames,
                          int* frames_pushed, void* stream);
int srf_ctc_beam_lm_push_n(void* state, size_t state_bytes, int B, int C, int beam_width, int max_frames, int blank,
                           const float* logits, const int* n_valid, int n, const float* bonus, const int* next,
                           int n_states, int* frames_pushed, void* stream);
int srf_ctc_beam_lm_best(const void* state, size_t state_bytes, int B, int C, int beam_width, int max_frames,
                         int* labels, int* count, float* score, float* lm_score, void* stream);
int srf_ctc_beam_lm_nbest(const void* state, size_t state_bytes, int B, int C, int beam_width, int max_frames, int N,
                          int max_len, int* labels, int* count, float* score, float* lm_score, int* n_hyp,
                          void* stream);
/* srf_ctc_beam_cut / srf_ctc_beam_lm_cut: close a segment of some utterances (endpointing,
 * below).  cut [B] (device): for every utterance with cut[b] >= 0, what best would return
 * goes to labels [B][max_len] (labels at index max_len and beyond are not stored), count
 * [B], log_prob / score [B] and, fused, lm_score [B]; then that utterance alone is put back
 * to the reset state, header and beam entry 0 as reset leaves them (fused: state 0 and no
 * bonus).  An utterance with cut[b] < 0 gets count[b] = -1 and is not touched otherwise.
 * The host counter frames_pushed is not involved.
 * With rest (else null, and logits, n_valid, n_rest may be null): cut[b] is the chunk frame
 * of logits [B][n][C] that ended the segment, cut[b] < n; the frames after it, [cut[b] + 1,
 * clamp(n_valid[b], 0, n)), are copied to the front of rest [B][n][C] and n_rest [B]
 * receives their number (0 for an utterance without a cut): the push that opens the next
 * segment, srf_ctc_beam_push_n taking no per-utterance first frame. */
int srf_ctc_beam_cut(void* state, size_t state_bytes, int B, int C, int beam_width, int max_frames, const int* cut,
                     int max_len, int* labels, int* count, float* log_prob, const float* logits, const int* n_valid,
                     int n, float* rest, int* n_rest, void* stream);
int srf_ctc_beam_lm_cut(void* state, size_t state_bytes, int B, int C, int beam_width, int max_frames, const int* cut,
                        int max_len, int* labels, int* count, float* score, float* lm_score, const float* logits,
                        const int* n_valid, int n, float* rest, int* n_rest, void* stream);

/* ---- Endpointing (srf_amd/endpoint.py) ---------------
 * Where an utterance ends, from the CTC logits alone.  Per stream the state is n (frames in
 * the open segment), sil (trailing silence run), speech (a flag) and t (frames consumed
 * since the reset, an int); for every consumed frame x [C], in order:
 *   lp_blank = x[blank] - (max(x) + log(sum(exp(x - max(x)))))          (fp32)
 *   is_sil   = lp_blank > log_thr,   is_sp = argmax(x) != blank  (lowest index on a tie)
 *   n += 1;  sil = is_sil ? sil + 1 : 0;  speech |= is_sp
 *   reason = 2 if speech and sil >= silence_after_speech, else 1 if sil >= silence_only,
 *            else 3 if n >= max_segment, else 0
 *   if reason: emit (t - n + 1, t, reason);  n = sil = 0;  speech = false
 * Everything after the two flags is integer: the cuts are a function of the stream's
 * frames, whatever the chunking, B and the other streams.
 *
 * state: srf_ctc_endpoint_state_bytes(B) bytes on the device (0 and a message for B < 1);
 * reset starts every stream over.  srf_ctc_endpoint_n: logits [B][n][C], n_valid [B]
 * (device, clamped to [0, n]), any C >= 2, the three counts >= 1, log_thr = log of a
 * threshold in (0, 1), max_cuts >= 1.  cut_start, cut_end, cut_reason [B][max_cuts]: the
 * segments [start, end] (inclusive, in frames since the reset) that this call closed, -1
 * past their number; n_cuts [B]: that number.  A call that closes more than max_cuts
 * segments of a stream stores the first max_cuts and still reports the true number; the
 * state always runs to the end of the chunk.  n = 0 launches nothing and writes nothing. */
size_t srf_ctc_endpoint_state_bytes(int B);
int srf_ctc_endpoint_reset(void* state, int B, void* stream);
int srf_ctc_endpoint_n(const float* logits, const int* n_valid, int B, int n, int C, int blank, float log_thr,
                       int silence_only, int silence_after_speech, int max_segment, void* state, int max_cuts,
                       int* cut_start, int* cut_end, int* cut_reason, int* n_cuts, void* stream);

/* ---- MWER: expected error over an N-best list (tfsr/helper/train_helper.py
 * loss_ewerr) ----------------------------------------------------------------
 * logits [B][Tmax][C] and logit_len [B] as srf_ctc_loss's (T_b = clamp(logit_len[b], 0,
 * Tmax)); hyp [B][N][Lmax] int32 dense label rows, hyp_len [B][N] clamped to [0, Lmax]
 * (entries past a length are never read), n_hyp [B] clamped to [0, N], err [B][N] int32
 * error counts.  With lp = log_softmax in fp32, per utterance over its n = n_hyp[b] rows:
 *   ll_i = log P_CTC(y_i | x), the full sum over alignments (-nll of srf_ctc_loss; an
 *          empty row is legal; -inf if infeasible, if T_b = 0 or if a label lies outside
 *          [0, C)),
 *   p_i = exp(ll_i - LSE_k ll_k), ebar = (sum_i e_i) / n, loss_b = sum_i p_i (e_i - ebar),
 *   w_i = p_i (e_i - ebar - loss_b) = d loss_b / d ll_i,
 *   grad[b][t][c] = grad_scale * sum_i w_i occ_i[t][c] for t < T_b, 0 past T_b, where
 *   occ_i is hypothesis i's state occupancy exp(LSE_{s: ext_i[s] = c}(alpha_i + beta_i)
 *   - lp - ll_i).  sum_i w_i = 0, so every row of grad sums to 0 over c.
 * e_i - ebar is computed as (n e_i - sum e) / n: equal errors (and n = 1) give loss = 0
 * and grad = 0 exactly.  n = 0 or every ll_i = -inf: loss = 0, grad = 0, p = 0.
 * Outputs: hyp_logp [B][N] = ll_i (-inf past n_hyp), p_hat [B][N], loss [B], grad
 * [B][Tmax][C] (NULL: loss only, the same bits).  Four launches on the stream, no
 * allocation, no host synchronisation: the log-softmax once per utterance, the alpha /
 * beta recursions of all B N hypotheses in one launch, p / loss / w, the gradient.
 * Limits: B >= 1, 1 <= Tmax <= 65535, C >= 2, 0 <= blank < C, 1 <= N <= SRF_MWER_MAX_HYP,
 * Lmax >= 0 with 12 (2 Lmax + 1) <= 65536 and 4 (2 C + 3 Lmax + 1) <= 65536 (LDS bytes),
 * B N < 2^31, Tmax (2 Lmax + 1) <= 2^29; anything else is refused before any launch (the
 * workspace query then returns 0 and leaves a message).  workspace: 16-byte aligned,
 *   srf_mwer_workspace = 4 (B Tmax C + B N Tmax 2 (2 Lmax + 1) + B N) bytes
 * (log-softmax, alpha and beta of every hypothesis, w). */
#define SRF_MWER_MAX_HYP 32
size_t srf_mwer_workspace(int B, int Tmax, int C, int N, int Lmax);
int srf_mwer_loss(const float* logits, const int* logit_len, const int* hyp, const int* hyp_len, const int* n_hyp,
                  const int* err, int B, int Tmax, int C, int N, int Lmax, int blank, float grad_scale,
                  float* hyp_logp, float* p_hat, float* loss, float* grad, void* workspace, size_t workspace_bytes,
                  void* stream);
/* srf_stream_advance_n: up to SRF_STREAM_ADVANCE_MAX sliding state buffers, each
 * [B][rows_per_stream][row_bytes], move rows [shift, shift + keep) of every stream to
 * rows [0, keep) in one launch (the other rows keep or lose their content: undefined).
 * Source and destination may overlap (keep > shift): one workgroup per (buffer, stream)
 * walks the block in ascending tiles, each read whole into registers before a barrier
 * and stored after it.  shift + keep <= rows_per_stream; shift = 0 or keep = 0 moves
 * nothing. */
#define SRF_STREAM_ADVANCE_MAX 32
typedef struct {
  void* ptr;
  size_t row_bytes;
  int rows_per_stream, shift, keep;
} srf_stream_buf;
int srf_stream_advance_n(const srf_stream_buf* bufs, int n_bufs, int B, void* stream);

/* ---- Waveform front end: 16 kHz samples to 123-d fbank features -------------
 * Replaces the Kaldi step of egs/script/fbank123.sh (compute-fbank-feats --num-mel-bins=40
 * --sample-frequency=16000 --use-log-fbank=True --use-energy=True, add-deltas, CMVN as
 * save_speech_data.py:163 applies it; the online CMVN of a live stream is srf_cmvn_sliding
 * below).  fp32 throughout; DESIGN.md section 18 has the definitions.  Samples are in int16
 * scale, int16 (is_int16 = 1) or float32.
 *
 * Framing (snip-edges): T(n) = 0 for n < 400, else 1 + (n - 400) / 160 (srf_fbank_num_frames);
 * frame t is samples 160 t .. 160 t + 399 of its stream.
 *
 * tables: SRF table block of srf_fbank_table_floats() floats, filled on the host by
 * srf_fbank_tables (Povey window, exp(-2 pi i k / 512) for k < 256, and per mel filter its
 * first bin, bin count and weights; computed in double, rounded once) and copied to the
 * device by the caller.
 *
 * srf_fbank_static: frames [t0, t1) of every stream.  samples [B][stride], of which
 * columns [0, width) hold the global samples s0 .. s0 + width - 1; n_samples [B] (device)
 * the streams' lengths; a stream has T_b = T(min(max(n_samples[b], 0), n_limit)) frames,
 * n_limit <= s0 + width the samples that have arrived.  statics [B][Ts][41], row r = frame
 * f0 + r: rows of frames t < T_b get [log energy | 40 log-mel values], rows of frames
 * T_b <= t < t1 zeros.  dither = a > 0 adds a g to every sample, g a standard Gaussian
 * (Box-Muller) keyed by (seed, b, global sample index), so overlapping frames and every
 * chunking see the same noise; a = 0 adds nothing.  A frame's values depend on its 400
 * samples only, not on the launch.  Refused before any launch: 160 t0 < s0, n_limit beyond
 * the buffer, rows outside [0, Ts), t1 > 13421764.
 *
 * srf_fbank_deltas: frames [t0, t1) of feats [B][To][123], row r = frame o0 + r, from
 * statics [B][Ts][41], row r = frame f0 + r.  T_b = min(max(n_frames[b], 0), t_limit).
 * Rows t < T_b: [static | delta | delta-delta] with the taps [-2 -1 0 1 2] / 10 and their
 * self-convolution, both applied to the statics at frame indices clamped to [0, T_b - 1];
 * then, with cmvn_rows = 1 (mean, stdev [123]) or B ([B][123]),
 * y = (x - mean + 1e-14) / (stdev + 1e-14).  Rows T_b <= t < t1: zeros.  The statics frames
 * max(t0 - 4, 0) .. min(t1 + 3, t_limit - 1) must lie in the statics buffer.
 *
 * srf_fbank_stats: sums [2 D + 1] doubles (device) += [sum x | sum x^2 | frame count] over
 * the rows t < min(n_frames[b], T) of feats [B][T][D].  One launch, one workgroup per
 * dimension, no atomics; nothing is read back. */
#define SRF_FBANK_FRAME_LEN 400
#define SRF_FBANK_FRAME_SHIFT 160
#define SRF_FBANK_MEL 40
#define SRF_FBANK_STATIC 41
#define SRF_FBANK_FEAT 123
int srf_fbank_num_frames(int n_samples);
size_t srf_fbank_table_floats(void);
int srf_fbank_tables(float* tables, size_t n_floats);
int srf_fbank_static(const void* samples, int is_int16, const int* n_samples, const float* tables, int B, int stride,
                     int width, int s0, int n_limit, int t0, int t1, int f0, int Ts, float dither,
                     unsigned long long seed, float* statics, void* stream);
int srf_fbank_deltas(const float* statics, const int* n_frames, int B, int Ts, int f0, int t_limit, int t0, int t1,
                     const float* mean, const float* stdev, int cmvn_rows, float* feats, int To, int o0, void* stream);
int srf_fbank_stats(const float* feats, const int* n_frames, int B, int T, int D, double* sums, void* stream);

/* ---- Online CMVN: sliding-window normalisation of feature rows ---------------
 * What a live stream applies in place of the per-speaker CMVN above, whose statistics
 * need the speaker's utterances in advance (Kaldi's OnlineCmvn in spirit; DESIGN.md
 * section 20 is the definition).  For stream b, frame t < T_b = max(n_frames[b], 0) and
 * dimension d, in fp64 with one rounding to fp32 at the end, W = window:
 *   lo = max(0, t - W + 1), n = t - lo + 1, S1 = sum_{u = lo .. t} x[u], S2 = sum x[u]^2,
 *   c = min(W - n, prior_count[b]) (0 without a prior),
 *   m = (S1 + c mean_p) / (n + c), q = (S2 + c (std_p^2 + mean_p^2)) / (n + c),
 *   y = (x[t] - m) / sqrt(max(q - m m, 1e-10)) with norm_vars, else y = x[t] - m.
 * The prior: prior_rows = 0 (none), 1 (prior_mean, prior_std [D] and prior_count [1],
 * shared) or B ([B][D] and [B]), doubles on the device.
 *
 * srf_cmvn_sliding: frames [t0, t1) of out [B][To][D], row r = frame o0 + r, from feats
 * [B][rows][D], row r = frame f0 + r; rows of frames T_b <= t < t1 get zeros.  The sums
 * are taken per tile of SRF_CMVN_TILE absolute frames: in ascending frame order over the
 * window of the tile's first frame, then slid frame by frame, "- x[t - W]" before
 * "+ x[t]".  A launch that starts inside a tile recomputes from the tile's first frame, so
 * a frame's bits depend on its stream's frames and on t alone, not on t0, t1, f0, B or the
 * chunking, and the input must hold the frames from
 * max(0, t0 / SRF_CMVN_TILE * SRF_CMVN_TILE - W + 1) to t1 - 1; anything else is refused
 * before the launch.  last (device, or NULL) [B][2 D + 1] doubles: a stream whose frame
 * min(T_b, t1) - 1 lies in [t0, t1) gets [m | q | n + c] of that frame, what its last
 * frame so far was normalised with (the speaker carry reads it); other streams' rows are
 * left alone.  One launch, no workspace, no atomics, nothing read back. */
#define SRF_CMVN_TILE 32
#define SRF_CMVN_MAX_DIM 128
#define SRF_CMVN_MAX_WINDOW 4096
int srf_cmvn_sliding(const float* feats, const int* n_frames, int B, int rows, int D, int f0, int t0, int t1,
                     const double* prior_mean, const double* prior_std, const double* prior_count, int prior_rows,
                     int window, int norm_vars, float* out, int To, int o0, double* last, void* stream);

/* ---- Resampler: audio at any rate to another (16 kHz for the front end) ------
 * Kaldi's LinearResample as ResampleWaveform configures it (what compute-fbank-feats applies
 * to input whose rate is not --sample-frequency); DESIGN.md section 19 has the definition.
 * Rates fin, fout are integers in [4000, 192000]; g = gcd, iu = fin / g, ou = fout / g;
 * cutoff fc = 0.99 * 0.5 * min(fin, fout), half width ww = 6 / (2 fc) seconds.  Output o has
 * phase p = o mod ou and unit u = o div ou; with t = p / fout, first[p] = ceil((t - ww) fin),
 * w[p][j] = win(d) filt(d) / fin at d = (first[p] + j) / fin - t, win(d) = (1 + cos(2 pi fc
 * d / 6)) / 2 inside |d| < ww (else 0), filt(d) = sin(2 pi fc d) / (pi d) (2 fc at 0); taps
 * is the longest row, shorter rows end in zeros.  y[o] = sum_{j < taps} w[p][j] x[first[p] +
 * u iu + j] with x zero outside [0, n), summed in fp32 in the order of j, one fma per tap.
 * n input samples give ceil(n ou / iu) outputs (srf_resample_num_out, 64-bit arithmetic).
 * fin == fout is the exact copy: one tap of weight 1.
 *
 * tables: one block for a bank of up to SRF_RESAMPLE_MAX_RATES input rates and one output
 * rate, srf_resample_table_floats floats (0 and a message if refused), filled on the host
 * by srf_resample_tables in double, rounded once, and copied to the device by the caller.
 * Layout (every entry a float): [0] the number of rates, [1] fout, [2 .. 7] zero; rate r has
 * the 8 floats at SRF_RESAMPLE_HEADER + 8 r = [iu, ou, taps, offset of first, offset of w,
 * fin, 0, 0]; from SRF_RESAMPLE_HEADER + 8 SRF_RESAMPLE_MAX_RATES on, per rate first[ou] and
 * w[ou][taps].  Refused: a rate outside the range, more than SRF_RESAMPLE_MAX_RATES rates, a
 * bank whose weights exceed 2^20 floats.
 *
 * srf_resample: outputs [o0, o1) of every row, one launch.  samples [B][stride], int16
 * (is_int16 = 1) or float32, of which columns [0, width) hold the global samples s0 .. s0 +
 * width - 1; n_samples [B] (device) the rows' lengths; choice [B] (device) a row's index
 * into the bank, clamped to it, or NULL: 0 for every row; rates_in [n_rates] (host) and
 * rate_out are the rates the block was built for.  n_b = min(max(n_samples[b], 0), n_limit),
 * n_limit <= s0 + width the samples that have arrived.  out [B][stride_out], column c =
 * output q0 + c: outputs o < num_out(n_b) get y[o] with inputs at indices >= n_b read as
 * zero, outputs num_out(n_b) <= o < o1 get 0; n_out [B] (device, or NULL) receives
 * num_out(n_b), capped at 2^31 - 1, from the same launch.  Refused before any launch: n_limit beyond the
 * buffer, outputs outside the output buffer, o1 > 2^31 - 2049, and, for any rate of the
 * bank, a first tap of output o0 that lies below s0 > 0.  No workspace, no atomics. */
#define SRF_RESAMPLE_MAX_RATES 8
#define SRF_RESAMPLE_HEADER 8
size_t srf_resample_table_floats(const int* rates_in, int n_rates, int rate_out);
int srf_resample_tables(const int* rates_in, int n_rates, int rate_out, float* tables, size_t n_floats);
size_t srf_resample_num_out(size_t n, int rate_in, int rate_out);
int srf_resample(const void* samples, int is_int16, const int* n_samples, const int* choice, const float* tables,
                 const int* rates_in, int n_rates, int rate_out, int B, int stride, int width, int s0, int n_limit,
                 int o0, int o1, float* out, int stride_out, int q0, int* n_out, void* stream);

/* ---- Fused Adam over one flat parameter buffer ----------------------------
 * Replaces the Keras Adam apply of trainer_sr.py:71 / train_helper.py:60-70:
 * m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2; p -= alpha m / (sqrt(v) + eps),
 * alpha = lr(step) sqrt(1-b2^t)/(1-b1^t) computed by the caller.  All four
 * buffers 16-byte aligned, n floats each. */
int srf_adam_step(float* params, const float* grads, float* m, float* v, size_t n, float alpha, float b1,
                  float b2, float eps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SRF_H_ */
