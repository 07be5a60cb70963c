"""The endpoint rule without a GPU: the float64 restatement (tests/endpoint_ref.py) on the
inputs the GPU tests use and on hand cases, the argument checks of srf_amd/endpoint.py, of
ctc.BeamState(segmented=True) and of StreamingRouter(endpoint=...), and the refusals of the
C entry points before any launch."""
import ctypes
import types

import numpy as np
import pytest
import torch

from srf_amd import ctc, endpoint, streaming
from tests import endpoint_ref as R


@pytest.mark.parametrize('C,plan', sorted(R.ANCHORS))
def test_anchors(C, plan):
    """The generator is the one described: its cuts under rules (12, 5, 40, 0.8)."""
    assert R.cuts(R.plan_logits(plan, C), C - 1, R.RULES) == R.ANCHORS[(C, plan)]


def test_all_three_reasons_occur_at_every_width():
    for C in R.WIDTHS:
        reasons = {r for i in range(len(R.PLANS)) for _, _, r in R.cuts(R.plan_logits(i, C), C - 1, R.RULES)}
        assert reasons == {1, 2, 3}, (C, reasons)


@pytest.mark.parametrize('C', R.WIDTHS)
def test_no_flag_is_decided_by_rounding(C):
    """A condition on the inputs, not a tolerance on the result: every frame's lp_blank is
    further than 1e-4 from log 0.8, a hundred times what an fp32 log-softmax is off by."""
    worst = min(R.margin(R.plan_logits(i, C), C - 1, R.RULES[3]) for i in range(len(R.PLANS)))
    print(f'C={C}: smallest |lp_blank - log 0.8| = {worst:.4g}')
    assert worst > 1e-4
    assert abs(worst - R.MARGINS[C]) <= 0.01 * R.MARGINS[C]   # (the figures on record, to their digits)


def test_argmax_ties_take_the_lowest_index():
    x = np.zeros((3, 4))
    x[1, [1, 3]] = 2.0   # class 1 ties with the blank: class 1 is the arg-max, the frame is speech
    x[2, 3] = 9.0
    is_sil, is_sp, _ = R.flags(x, 3, 0.8)
    assert is_sp.tolist() == [True, True, False] and is_sil.tolist() == [False, False, True]


def _frames(classes, C=4, blank=3):
    """Frames that say ``classes`` with probability ~1 (a blank frame is silent at 0.8)."""
    x = np.zeros((len(classes), C))
    x[np.arange(len(classes)), classes] = 20.0
    return x


def test_hand_silence_after_speech():
    """rules (50, 4, 100): 3 blanks between two labels give no cut, 4 give one at the 4th."""
    rules = (50, 4, 100, 0.8)
    assert R.cuts(_frames([0, 3, 3, 3, 1, 3, 3]), 3, rules) == []
    assert R.cuts(_frames([0, 3, 3, 3, 3, 1, 3]), 3, rules) == [(0, 4, 2)]
    # the machine starts over after the cut: label 1 at frame 5 opens a segment of its own
    assert R.cuts(_frames([0, 3, 3, 3, 3, 1, 3, 3, 3, 3]), 3, rules) == [(0, 4, 2), (5, 9, 2)]


def test_hand_silence_only():
    rules = (6, 2, 100, 0.8)
    assert R.cuts(_frames([3] * 5), 3, rules) == []
    assert R.cuts(_frames([3] * 6), 3, rules) == [(0, 5, 1)]
    assert R.cuts(_frames([3] * 13), 3, rules) == [(0, 5, 1), (6, 11, 1)]


def test_hand_priority():
    """2 beats 1 beats 3 on a frame where several hold."""
    # frame 3: speech and sil = 3 >= 3 (2), sil >= 3 (1) and n = 4 >= 4 (3)
    assert R.cuts(_frames([0, 3, 3, 3]), 3, (3, 3, 4, 0.8)) == [(0, 3, 2)]
    # nothing decoded: 1 and 3 hold on frame 3
    assert R.cuts(_frames([3, 3, 3, 3]), 3, (4, 9, 4, 0.8)) == [(0, 3, 1)]
    # 3 alone: speech without a pause
    assert R.cuts(_frames([0, 1, 0, 1, 0]), 3, (4, 2, 4, 0.8)) == [(0, 3, 3)]


def test_chunking_the_restatement_changes_nothing():
    x = R.plan_logits(0, 8)
    st, got, pos = [0, 0, False, 0], [], 0
    for n in [1, 3, 5, 4] + [5] * 40:
        got += R.cuts(x[pos:pos + n], 7, R.RULES, st)
        pos += n
    assert pos >= R.T and got == R.ANCHORS[(8, 0)] and st[3] == R.T


def test_rules_argument_errors():
    r = endpoint.EndpointRules()
    assert r.counts == (125, 25, 500) and r.blank_threshold == 0.8
    assert r.log_threshold == np.log(0.8)
    for kw, word in [(dict(silence_only=0), 'silence_only'), (dict(silence_after_speech=-1), 'silence_after_speech'),
                     (dict(max_segment=0), 'max_segment'), (dict(max_segment=2.5), 'max_segment'),
                     (dict(blank_threshold=0.0), 'blank_threshold'), (dict(blank_threshold=1.0), 'blank_threshold')]:
        with pytest.raises(ValueError, match=word):
            endpoint.EndpointRules(**kw)
    with pytest.raises(ValueError, match='EndpointRules'):
        endpoint.Endpointer((12, 5, 40, 0.8), 2, 8, 7, 'cpu')
    with pytest.raises(ValueError, match='n_streams'):
        endpoint.Endpointer(r, 0, 8, 7, 'cpu')
    with pytest.raises(ValueError, match='classes'):
        endpoint.Endpointer(r, 2, 1, 0, 'cpu')
    with pytest.raises(ValueError, match='blank'):
        endpoint.Endpointer(r, 2, 8, 8, 'cpu')
    with pytest.raises(ValueError, match='device tensor'):
        endpoint.endpoints(torch.zeros(1, 3, 4), [3], 3, r)
    assert endpoint.REASONS[0] == 'end' and sorted(endpoint.REASONS) == [0, 1, 2, 3]


def test_push_cut_needs_a_segmented_state():
    with pytest.raises(ValueError, match='blank'):
        ctc.BeamState(1, 8, 8, beam_width=4, device='cpu', segmented=True)
    s = types.SimpleNamespace(segmented=False)
    with pytest.raises(ValueError, match='segmented'):
        ctc.BeamState.push_cut(s, torch.zeros(1, 2, 8), [2], [-1])


def _model(L=2, rpad=2):
    return types.SimpleNamespace(caps_type='naive', pose_fp8=False, enc_num=L, lpad=2, rpad=rpad, class_n=32,
                                 flat_params=torch.zeros(1), feat_dim_in=123)


def test_router_refuses_rules_that_allow_two_cuts_in_a_step():
    """nmax = max(max_chunk // 4, lookahead): 6 for L = 2, rpad = 2 at max_chunk 12, 16 at 64."""
    with pytest.raises(ValueError, match='at most one cut'):
        streaming.StreamingRouter(_model(), 2, max_chunk=12, endpoint=endpoint.EndpointRules(16, 5, 30))
    with pytest.raises(ValueError, match='at most one cut'):
        streaming.StreamingRouter(_model(), 2, max_chunk=64, endpoint=endpoint.EndpointRules(15, 16, 30))
    with pytest.raises(ValueError, match='EndpointRules'):
        streaming.StreamingRouter(_model(), 2, max_chunk=12, endpoint=(16, 6, 30, 0.8))


def test_router_refuses_a_beam_too_short_for_a_segment():
    with pytest.raises(ValueError, match='max_frames >= 36'):
        streaming.StreamingRouter(_model(), 2, max_chunk=12, beam_width=8, max_frames=35,
                                  endpoint=endpoint.EndpointRules(16, 6, 30))


def test_abi_refusals():
    """The new entry points are bound as include/srf.h declares them and refuse bad arguments
    before any launch."""
    from srf_amd import _lib
    L = _lib.lib()
    for name, n_args in [('srf_ctc_endpoint_state_bytes', 1), ('srf_ctc_endpoint_reset', 3), ('srf_ctc_endpoint_n', 17),
                         ('srf_ctc_beam_cut', 17), ('srf_ctc_beam_lm_cut', 18)]:
        assert len(_lib._SIGNATURES[name][1]) == n_args and hasattr(L, name), name
    assert L.srf_ctc_endpoint_state_bytes(28) == 28 * 16
    assert L.srf_ctc_endpoint_state_bytes(0) == 0 and b'B >= 1' in L.srf_last_error()
    one = ctypes.c_void_p(4096)   # never dereferenced: every call below is refused or launches nothing

    def ep(B=2, n=4, C=8, blank=7, thr=np.log(0.8), counts=(12, 5, 40), max_cuts=1, logits=one, state=one):
        return L.srf_ctc_endpoint_n(logits, one, B, n, C, blank, thr, *counts, state, max_cuts, one, one, one, one,
                                    None)
    assert ep(n=0) == 0   # nothing to do is no error
    for kw, msg in [(dict(B=0), b'B >= 1'), (dict(C=1), b'C >= 2'), (dict(n=-1), b'n >= 0'), (dict(blank=8), b'blank'),
                    (dict(counts=(0, 5, 40)), b'counts'), (dict(counts=(12, 5, 0)), b'counts'),
                    (dict(thr=0.0), b'log_thr'), (dict(thr=-np.inf), b'log_thr'), (dict(max_cuts=0), b'max_cuts'),
                    (dict(state=None), b'null'), (dict(logits=None), b'null')]:
        assert ep(**kw) == -1, kw
        assert msg in L.srf_last_error(), (kw, L.srf_last_error())
    assert L.srf_ctc_endpoint_reset(None, 2, None) == -1

    need = L.srf_ctc_beam_state_bytes(1, 8, 4, 10)
    assert L.srf_ctc_beam_cut(one, need - 1, 1, 8, 4, 10, one, 10, one, one, one, None, None, 0, None, None, None) == -1
    assert b'state block' in L.srf_last_error()
    assert L.srf_ctc_beam_cut(one, need, 1, 8, 4, 10, one, 0, one, one, one, None, None, 0, None, None, None) == -1
    assert b'max_len' in L.srf_last_error()
    assert L.srf_ctc_beam_cut(one, need, 1, 8, 4, 10, None, 10, one, one, one, None, None, 0, None, None, None) == -1
    assert b'null' in L.srf_last_error()
    assert L.srf_ctc_beam_cut(one, need, 1, 8, 4, 10, one, 10, one, one, one, None, one, 2, one, one, None) == -1
    assert b'after the cut' in L.srf_last_error()
    need = L.srf_ctc_beam_lm_state_bytes(1, 8, 4, 10)
    assert L.srf_ctc_beam_lm_cut(one, need, 1, 8, 4, 10, one, 10, one, one, one, None, None, None, 0, None, None,
                                 None) == -1
    assert b'null' in L.srf_last_error()
