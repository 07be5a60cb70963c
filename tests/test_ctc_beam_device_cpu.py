"""The case list of the device beam search (tests/beam_ref.py) is one on which rounding
does not decide the answer: on every case the float64 restatement of the algorithm and
the fp32 host decoder (srf_ctc_beam_search) return the same labelling, and their log
probabilities agree within 1e-4 * (1 + |logp|).  The GPU tests compare the device decoder
with the host decoder on the same cases (tests/test_ctc_beam_device_gpu.py).

Also here, without a device: the argument checks of the device entry points.
"""
import ctypes

import numpy as np
import pytest
import torch

from srf_amd import ctc
from tests import beam_ref


@pytest.mark.parametrize('T,C,W', beam_ref.CASES)
def test_case_list_is_decided_beyond_rounding(T, C, W):
    blank = C - 1
    for seed in beam_ref.SEEDS:
        x = beam_ref.case_logits(seed, T, C)
        want, want_lp, gap = beam_ref.beam_search(x, blank, W)
        hyps, logp = ctc.beam_search_decode(torch.tensor(x)[None], [T], blank, beam_width=W)
        print(f'T={T} C={C} W={W} seed={seed}: logp {logp[0]:.6f} vs {want_lp:.6f}, gap to the second {gap:.2e}')
        assert hyps[0] == want, (seed, T, C, W)
        assert abs(logp[0] - want_lp) <= 1e-4 * (1 + abs(want_lp)), (seed, T, C, W)


def test_readopt_cases_are_decided_beyond_rounding_and_exercise_readoption():
    """The flat, narrow-beam cases: float64 restatement and host decoder agree, the best
    prefix leads the second by more than 1e-3, and prefixes really are made again next to
    a child that stayed in the beam (seeds 36 and 38 among them)."""
    T, C, W = beam_ref.READOPT_CASE
    events = {}
    for seed in beam_ref.READOPT_SEEDS:
        x = beam_ref.readopt_logits(seed)
        stats = {}
        want, want_lp, gap = beam_ref.beam_search(x, C - 1, W, stats)
        events[seed] = stats['readopted']
        hyps, logp = ctc.beam_search_decode(torch.tensor(x)[None], [T], C - 1, beam_width=W)
        assert hyps[0] == want, seed
        assert abs(logp[0] - want_lp) <= 1e-4 * (1 + abs(want_lp)), seed
        assert gap > 1e-3, (seed, gap)
    print('readoptions per seed:', events)
    assert events[36] > 0 and events[38] > 0
    assert sum(1 for v in events.values() if v) >= 5


def test_reference_breaks_ties_by_creation_order():
    """Equal logits in every frame: all extensions of a prefix tie, and the totals of
    whole groups of prefixes tie.  The restatement and the host decoder keep the same
    ones (the earlier-created), so they return the same labelling."""
    for T, C, W in beam_ref.TIE_CASES:
        x = np.zeros((T, C), np.float32)
        want, want_lp, _ = beam_ref.beam_search(x, C - 1, W)
        hyps, logp = ctc.beam_search_decode(torch.tensor(x)[None], [T], C - 1, beam_width=W)
        assert hyps[0] == want
        assert abs(logp[0] - want_lp) <= 1e-4 * (1 + abs(want_lp))


def test_device_entry_points_refuse_bad_shapes_without_gpu():
    from srf_amd import _lib
    L = _lib.lib()
    assert L.srf_ctc_beam_state_bytes(2, 63, 100, 50) >= 2 * 4 * (5 * 100 + 2 * (1 + 50 * 100))
    for B, C, W, F, word in ((1, 63, 129, 10, b'beam_width'), (1, 129, 100, 10, b'C <= 128'), (1, 1, 4, 10, b'2 <= C'),
                             (1, 8, 0, 10, b'beam_width'), (0, 8, 4, 10, b'B >= 1'), (1, 8, 4, 0, b'max_frames')):
        assert L.srf_ctc_beam_state_bytes(B, C, W, F) == 0
        assert word in L.srf_last_error(), (L.srf_last_error(), word)
    pushed = ctypes.c_int(0)
    need = L.srf_ctc_beam_state_bytes(1, 8, 4, 10)
    fake = ctypes.c_void_p(4096)   # never dereferenced: every call below is refused before a launch
    assert L.srf_ctc_beam_reset(fake, need - 1, 1, 8, 4, 10, ctypes.byref(pushed), None) == -1
    assert b'state block' in L.srf_last_error()
    assert L.srf_ctc_beam_push_n(fake, need, 1, 8, 4, 10, 8, fake, fake, 1, ctypes.byref(pushed), None) == -1
    assert b'blank' in L.srf_last_error()
    pushed.value = 7
    assert L.srf_ctc_beam_push_n(fake, need, 1, 8, 4, 10, 7, fake, fake, 4, ctypes.byref(pushed), None) == -1
    assert b'max_frames' in L.srf_last_error() and pushed.value == 7
    assert L.srf_ctc_beam_best(fake, need - 1, 1, 8, 4, 10, fake, fake, fake, None) == -1
    assert b'state block' in L.srf_last_error()


def test_python_wrappers_refuse_outside_the_range():
    with pytest.raises(ValueError, match='beam width'):
        ctc.BeamState(1, 63, 62, beam_width=129, device='cpu')
    with pytest.raises(ValueError, match='classes'):
        ctc.BeamState(1, 129, 128, beam_width=100, device='cpu')
    with pytest.raises(ValueError, match='blank'):
        ctc.BeamState(1, 8, 8, beam_width=4, device='cpu')
    with pytest.raises(ValueError, match='device tensor'):
        ctc.beam_search_decode_device(torch.zeros(1, 3, 4), [3], 3, beam_width=4)
