"""The forced-alignment reference (tests/align_ref.py) pinned on the host, and the
conditions under which tests/test_ctc_align_gpu.py may ask the device for the reference's
path exactly.  Needs no GPU.  Each test prints its figures before it asserts.

Observed: short cases, smallest (score - second best) / bound 3.54; the float32 run
returns the float64 path on all 40; long cases, the float32 run returns the float64 path
on all 48 too, so its float64 score lies 0 bounds below the optimum."""
import itertools

import numpy as np
import pytest

from tests import align_ref as ar


@pytest.mark.parametrize('T,C,labels', [(5, 3, [0, 1]), (6, 3, [0, 0]), (4, 4, [2]), (5, 3, [])])
def test_exhaustive_pin(T, C, labels):
    """All C^T frame sequences that collapse to the labels: the reference's score is
    their maximum and its path the arg-max."""
    blank = C - 1
    lp = ar.log_softmax(np.random.default_rng(T * 100 + C).standard_normal((T, C)) * 3)
    best, best_seq, n = -np.inf, None, 0
    for seq in itertools.product(range(C), repeat=T):
        if ar.collapse(seq, blank) == labels:
            n += 1
            sc = sum(lp[t, c] for t, c in enumerate(seq))
            if sc > best:
                best, best_seq = sc, list(seq)
    states, score = ar.viterbi(lp, labels, blank)
    ext = ar.extended(labels, blank)
    print(f'T={T} C={C} labels={labels}: {n} paths, best {best:.6f}, reference {score:.6f}')
    assert n > 0
    assert abs(score - best) < 1e-12
    assert [int(ext[s]) for s in states] == best_seq
    assert ar.is_valid_path(states, labels, blank)
    assert abs(ar.path_score(lp, labels, blank, states) - score) < 1e-12


@pytest.mark.parametrize('T,C,labels,want', ar.TIE_CASES)
def test_tie_rule_on_zero_logits(T, C, labels, want):
    lp = ar.log_softmax(np.zeros((T, C)))
    states, score = ar.viterbi(lp, labels, C - 1)
    print(f'T={T} labels={labels}: {states} score {score}')
    assert states == want
    if want is None:
        assert score == -np.inf
    else:
        assert abs(score - T * -np.log(C)) < 1e-12
    # the float32 run ties exactly too
    assert ar.viterbi(ar.log_softmax(np.zeros((T, C)), np.float32), labels, C - 1, np.float32)[0] == want


def test_edge_cases():
    lp = ar.log_softmax(np.zeros((0, 3)))
    assert ar.viterbi(lp, [], 2) == ([], 0.0)
    assert ar.viterbi(lp, [1], 2) == (None, -np.inf)
    assert ar.viterbi(ar.log_softmax(np.zeros((3, 3))), [1, 1, 1], 2) == (None, -np.inf)
    assert ar.viterbi(ar.log_softmax(np.zeros((1, 3))), [1], 2)[0] == [1]


@pytest.mark.parametrize('T,C,L', ar.SHORT_CASES)
def test_short_cases_have_a_unique_best_path(T, C, L):
    """What the GPU test relies on: the best path leads every other path by more than the
    fp32 bound, and carrying the sums in float32 returns the same path."""
    ratios = []
    for seed in ar.SEEDS:
        logits, labels, blank = ar.case(seed, T, C, L)
        states, score = ar.viterbi(ar.log_softmax(logits), labels, blank)
        assert ar.is_valid_path(states, labels, blank)
        gap = score - ar.second_best(ar.log_softmax(logits), labels, blank, states)
        ratios.append(gap / ar.bound(T, score))
        s32, sc32 = ar.viterbi(ar.log_softmax(logits, np.float32), labels, blank, np.float32)
        assert s32 == states, seed
        assert abs(sc32 - score) <= ar.bound(T, score)
    print(f'(T, C, L) = {(T, C, L)}: gap / bound {min(ratios):.2f} .. {max(ratios):.2f}')
    assert min(ratios) > 1.0


@pytest.mark.parametrize('T,C,L', ar.LONG_CASES)
def test_long_cases_float32_path_is_optimal_within_the_bound(T, C, L):
    worst, same = 0.0, 0
    for seed in ar.SEEDS:
        logits, labels, blank = ar.case(seed, T, C, L)
        lp = ar.log_softmax(logits)
        states, score = ar.viterbi(lp, labels, blank)
        assert ar.is_valid_path(states, labels, blank)
        s32, _ = ar.viterbi(ar.log_softmax(logits, np.float32), labels, blank, np.float32)
        assert ar.is_valid_path(s32, labels, blank)
        worst = max(worst, (score - ar.path_score(lp, labels, blank, s32)) / ar.bound(T, score))
        same += s32 == states
    print(f'(T, C, L) = {(T, C, L)}: float32 path below the optimum by at most {worst:.4f} bounds, '
          f'{same} of {len(ar.SEEDS)} paths equal')
    assert 0.0 <= worst <= 1.0


def test_second_best_by_enumeration():
    """second_best against the enumeration of all paths of a small case."""
    T, C, labels = 6, 3, [0, 1]
    blank = C - 1
    lp = ar.log_softmax(np.random.default_rng(5).standard_normal((T, C)) * 3)
    states, score = ar.viterbi(lp, labels, blank)
    S = 2 * len(labels) + 1
    scores = sorted((ar.path_score(lp, labels, blank, p) for p in itertools.product(range(S), repeat=T)
                     if ar.is_valid_path(list(p), labels, blank)), reverse=True)
    print(f'best {scores[0]:.6f} second {scores[1]:.6f}')
    assert abs(scores[0] - score) < 1e-12
    assert abs(scores[1] - ar.second_best(lp, labels, blank, states)) < 1e-12


def test_spans():
    assert ar.spans([0, 1, 1, 2, 3, 5, 5, 6], 3) == ([1, 4, 5], [3, 5, 7])
    assert ar.spans([1, 3], 2) == ([0, 1], [1, 2])
    assert ar.spans([0, 0, 0], 0) == ([], [])


def _onehot(path, C):
    x = np.full((len(path), C), -1.0, dtype=np.float32)
    x[np.arange(len(path)), path] = 2.0
    return x


def test_greedy_frames_restatement():
    """A repeat across a chunk edge (emitted in the earlier chunk), with a blank between
    (emitted again), blank-only chunks and n_valid = 0; any chunking gives the frames of
    the whole."""
    C, blank, a, b = 4, 3, 0, 1
    # [a a | a blank a | blank blank blank | b blank | blank a]
    path = [a, a, a, blank, a, blank, blank, blank, b, blank, blank, a]
    x = _onehot(path, C)
    labels, frames = ar.greedy_frames(x, len(path), blank)
    assert labels == [a, a, b, a] and frames == [0, 4, 8, 11]
    assert labels == ar.collapse(path, blank)
    for split in ([2, 3, 3, 2, 2], [12], [1] * 12, [3, 0, 1, 4, 4], [5, 7]):
        got_l, got_f, prev, pos = [], [], -1, 0
        for n in split:
            l, f, prev = ar.greedy_frames_chunk(x[pos:pos + n], n, blank, prev, pos)
            got_l += l
            got_f += f
            pos += n
        assert (got_l, got_f) == (labels, frames), split
    # a stream that ended: n_valid = 0 adds nothing and keeps prev; a short n_valid stops early
    assert ar.greedy_frames_chunk(x[:5], 0, blank, a, 40) == ([], [], a)
    assert ar.greedy_frames_chunk(x[3:8], 2, blank, a, 3) == ([a], [4], a)
    assert ar.greedy_frames_chunk(x[5:8], 3, blank, a, 5) == ([], [], blank)
    assert ar.greedy_frames(x, 9, blank) == ([a, a, b], [0, 4, 8])
