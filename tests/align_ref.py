"""Float64 restatement of the CTC forced alignment (srf_ctc_align) and of the greedy
label frames (srf_ctc_greedy_frames_n), and the case list both test files share.

Definition.  lp = log_softmax(logits[t, :]).  The extended label ext has S = 2 L + 1
states, even states the blank, state 2k + 1 label k.  A path pi_0 .. pi_{T-1} starts in
state 0 or 1, ends in S - 1 or S - 2, moves by 0 or +1 per frame, and by +2 only into a
label state whose label differs from the label two states back.  The alignment is the
path that maximises sum_t lp[t, ext[pi_t]].

Ties.  Among equal predecessors the lowest source state wins (+2 before +1 before stay);
at the last frame S - 2 unless S - 1 is strictly larger; a state at -inf never wins.
"""
import math

import numpy as np

NEG_INF = -math.inf

SEEDS = range(8)
# (T, C, L): on all 8 seeds of each the best path leads the second best by more than
# bound(T, score), so the device must return the reference's states exactly
SHORT_CASES = [(12, 5, 3), (40, 8, 10), (60, 32, 20), (64, 33, 31), (50, 63, 25)]
# (T, C, L), one per kernel variant: S > 128, S > 256, S > 512 (the workgroup loop),
# log-probabilities past the 96 KiB LDS budget, a wide row in LDS, and back-pointers past
# the budget (T * 8 * 16 bytes with S > 256).  Their best-path gaps lie below the bound.
LONG_CASES = [(200, 32, 90), (300, 32, 140), (300, 32, 260), (300, 128, 20), (30, 128, 14), (800, 4, 140)]
# all-zero logits (T, C, labels) -> states, None = infeasible
TIE_CASES = [(6, 3, [0, 0, 1], [0, 0, 1, 2, 3, 5]),
             (7, 4, [0, 1, 0], [0, 0, 0, 0, 1, 3, 5]),
             (5, 3, [1], [0, 0, 0, 0, 1]),
             (4, 3, [], [0, 0, 0, 0]),
             (2, 3, [0, 0], None)]


def bound(T, v):
    """fp32 bound on a path score or a difference of two: half an ulp per addition on
    each of two compared paths, doubled for the log-softmax's own rounding."""
    return 4.0 * T * 2.0 ** -23 * max(1.0, abs(float(v)))


def case(seed, T, C, L):
    """(logits [T, C] float32, labels, blank): repeats are always present for L >= 4."""
    rng = np.random.default_rng(2000 + seed)
    logits = (rng.standard_normal((T, C)) * 3).astype(np.float32)
    lab = rng.integers(0, C - 1, L)
    if L >= 4:
        lab[1] = lab[0]
        lab[L - 1] = lab[L - 2]
    return logits, [int(v) for v in lab], C - 1


def log_softmax(x, dtype=np.float64):
    x = np.asarray(x, dtype=dtype)
    m = x.max(axis=-1, keepdims=True)
    return (x - (m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True, dtype=dtype)))).astype(dtype)


def extended(labels, blank):
    ext = np.full(2 * len(labels) + 1, blank, dtype=np.int64)
    ext[1::2] = labels
    return ext


def _skip(ext, blank):
    skip = np.zeros(len(ext), dtype=bool)
    skip[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
    return skip


def viterbi(lp, labels, blank, dtype=np.float64):
    """lp [T, C] log-probabilities -> (states, score); (None, -inf) when no path exists,
    ([], 0.0) for T = 0 without labels.  dtype: the precision the sums are carried in."""
    lp = np.asarray(lp, dtype=dtype)
    T = lp.shape[0]
    ext = extended(labels, blank)
    S = len(ext)
    if T == 0:
        return ([], 0.0) if S == 1 else (None, NEG_INF)
    skip = _skip(ext, blank)
    ninf = np.array([NEG_INF], dtype=dtype)
    v = np.full(S, NEG_INF, dtype=dtype)
    v[:2] = lp[0, ext[:2]]
    back = np.zeros((T, S), dtype=np.int64)
    for t in range(1, T):
        p1 = np.concatenate([ninf, v[:-1]])
        p2 = np.where(skip, np.concatenate([ninf, ninf, v[:-2]])[:S], NEG_INF).astype(dtype)
        c2 = skip & (p2 >= p1) & (p2 >= v) & (p2 > NEG_INF)
        c1 = ~c2 & (p1 >= v) & (p1 > NEG_INF)
        back[t] = 2 * c2 + c1
        v = (np.maximum(np.maximum(v, p1), p2) + lp[t, ext]).astype(dtype)
    s = S - 1 if S == 1 or v[S - 1] > v[S - 2] else S - 2
    score = float(v[s])
    if score == NEG_INF:
        return None, NEG_INF
    states = [0] * T
    for t in range(T - 1, 0, -1):
        states[t] = s
        s -= int(back[t, s])
    states[0] = s
    return states, score


def path_score(lp, labels, blank, states):
    """Float64 score of a path of states."""
    lp = np.asarray(lp, dtype=np.float64)
    ext = extended(labels, blank)
    return float(sum(lp[t, ext[s]] for t, s in enumerate(states)))


def is_valid_path(states, labels, blank):
    """The path starts in 0 or 1, ends in S - 1 or S - 2 and moves legally."""
    ext = extended(labels, blank)
    S = len(ext)
    if not states or states[0] not in (0, 1) or states[-1] not in (S - 1, S - 2) or min(states) < 0:
        return False
    skip = _skip(ext, blank)
    for a, b in zip(states[:-1], states[1:]):
        if b - a not in (0, 1, 2) or b >= S or (b - a == 2 and not skip[b]):
            return False
    return True


def collapse(classes, blank):
    out, prev = [], -1
    for k in classes:
        if k != prev and k != blank:
            out.append(int(k))
        prev = k
    return out


def spans(states, L):
    """(starts, ends): label k occupies frames [starts[k], ends[k]) of the path."""
    starts, ends = [-1] * L, [-1] * L
    for t, s in enumerate(states):
        if s % 2 == 1:
            k = s // 2
            if starts[k] < 0:
                starts[k] = t
            ends[k] = t + 1
    return starts, ends


def second_best(lp, labels, blank, states):
    """The best score among paths that differ from ``states`` in at least one frame: the
    maximum over (t, s != states[t]) of the best path through state s at frame t, i.e.
    the forward plus the backward Viterbi score there.  -inf if there is none."""
    lp = np.asarray(lp, dtype=np.float64)
    T = lp.shape[0]
    ext = extended(labels, blank)
    S = len(ext)
    skip = _skip(ext, blank)
    ninf = np.array([NEG_INF])
    fwd = np.full((T, S), NEG_INF)
    fwd[0, :2] = lp[0, ext[:2]]
    for t in range(1, T):
        v = fwd[t - 1]
        p1 = np.concatenate([ninf, v[:-1]])
        p2 = np.where(skip, np.concatenate([ninf, ninf, v[:-2]])[:S], NEG_INF)
        fwd[t] = np.maximum(np.maximum(v, p1), p2) + lp[t, ext]
    bwd = np.full((T, S), NEG_INF)   # best continuation after frame t, frame t's emission excluded
    bwd[T - 1, max(0, S - 2):] = 0.0
    for t in range(T - 2, -1, -1):
        w = bwd[t + 1] + lp[t + 1, ext]
        q1 = np.concatenate([w[1:], ninf])
        q2 = np.concatenate([np.where(skip, w, NEG_INF)[2:], ninf, ninf])[:S]
        bwd[t] = np.maximum(np.maximum(w, q1), q2)
    through = fwd + bwd
    through[np.arange(T), states] = NEG_INF
    return float(through.max())


def greedy_frames_chunk(logits, n_valid, blank, prev, frame0):
    """srf_ctc_greedy_frames_n for one stream: logits [n, C] of which the first n_valid
    count -> (labels, frames, prev).  A label is emitted at the first frame of its
    arg-max run; a run that began in an earlier chunk (arg-max == prev) emits nothing."""
    labels, frames = [], []
    n = max(0, min(int(n_valid), len(logits)))
    for f in range(n):
        k = int(np.argmax(logits[f]))
        if k != prev and k != blank:
            labels.append(k)
            frames.append(frame0 + f)
        prev = k
    return labels, frames, prev


def greedy_frames(logits, length, blank):
    """The greedy labels of logits [T, C] up to ``length`` and the frame of each."""
    labels, frames, _ = greedy_frames_chunk(logits, length, blank, -1, 0)
    return labels, frames
