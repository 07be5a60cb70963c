/* srf_data_lm.h -- the host CTC prefix beam search with a fused language model
 * (libsrf_data.so, csrc/data/ctc_beam.cpp).  Next to srf_data.h, whose entry points and
 * their count stay as they are.
 */
#ifndef SRF_DATA_LM_H_
#define SRF_DATA_LM_H_
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* srf_ctc_beam_search (srf_data.h) with a language model fused into the beam (shallow
 * fusion); defines the result of srf_ctc_beam_lm_* in srf.h.  The model is a deterministic
 * automaton over the classes: bonus [n_states][C] (finite; what extending a prefix in
 * state s by class c adds to its score, the blank's column unused) and next [n_states][C]
 * (the state after it, in [0, n_states)); state 0 belongs to the empty prefix.  The one
 * change to the search:
 *   extend c:  log P_nb(l+c) gets ((c == last(l) ? log P_b(l) : log P(l)) + lp[c]) + bonus[s(l)][c]
 * in fp32 and in this order; the blank and repeat steps add nothing, so a prefix is ranked
 * by log p_ctc(prefix) + the sum of its bonuses.  *out_score is that score of the best
 * prefix, *out_lm_score its sum of bonuses, added in label order (either may be NULL).
 * Returns 0, or -1 on a bad argument, a table entry out of range included. */
int srf_ctc_beam_search_lm(const float* logits, int T, int C, int blank, int beam_width, const float* bonus,
                           const int32_t* next, int n_states, int32_t* out_labels, int* out_len, float* out_score,
                           float* out_lm_score);

#ifdef __cplusplus
}
#endif
#endif /* SRF_DATA_LM_H_ */
