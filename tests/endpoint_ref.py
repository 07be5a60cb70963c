"""The endpoint rule (srf_amd/endpoint.py, csrc/endpoint.hip) restated
in float64 numpy, and the inputs both endpoint test files share.

Per stream the state is n (frames in the open segment), sil (trailing silence run), speech
(a flag) and t (frames consumed); for every frame, in order:

    lp_blank = x[blank] - logsumexp(x);  is_sil = lp_blank > log(blank_threshold)
    is_sp    = argmax(x) != blank        (lowest index wins a tie)
    n += 1;  sil = sil + 1 if is_sil else 0;  speech |= is_sp
    reason = 2 if speech and sil >= silence_after_speech else 1 if sil >= silence_only
             else 3 if n >= max_segment else 0
    if reason: emit (t - n + 1, t, reason) with t this frame's index;  n = sil = 0;  speech = False
"""
import numpy as np

RULES = (12, 5, 40, 0.8)   # silence_only, silence_after_speech, max_segment, blank_threshold
T = 160
M = 8.0
WIDTHS = (8, 33, 128)
PLANS = [
    [('speech', 30), ('sil', 8), ('speech', 25), ('sil', 20), ('speech', 40), ('sil', 4), ('speech', 33)],
    [('speech', 160)],
    [('sil', 160)],
    [('sil', 3), ('speech', 12), ('sil', 5), ('speech', 9), ('sil', 4), ('speech', 60), ('sil', 67)],
]


def flags(x, blank, blank_threshold):
    """(is_sil [T] bool, is_sp [T] bool, margin [T] = |lp_blank - log threshold|) of the
    frames x [T, C], in float64."""
    x = np.asarray(x, np.float64)
    if x.shape[0] == 0:
        return np.zeros(0, bool), np.zeros(0, bool), np.zeros(0)
    mx = x.max(axis=-1)
    lp_blank = x[:, blank] - (mx + np.log(np.exp(x - mx[:, None]).sum(axis=-1)))
    thr = np.log(np.float64(blank_threshold))
    return lp_blank > thr, np.argmax(x, axis=-1) != blank, np.abs(lp_blank - thr)


def cuts(x, blank, rules, state=None):
    """The cuts [(start, end, reason)] of the frames x [T, C] under rules =
    (silence_only, silence_after_speech, max_segment, blank_threshold).  ``state``: a list
    [n, sil, speech, t] to continue from, updated in place (None: a stream's start)."""
    silence_only, silence_after_speech, max_segment, thr = rules
    st = [0, 0, False, 0] if state is None else state
    is_sil, is_sp, _ = flags(x, blank, thr)
    out = []
    n, sil, speech, t = st
    for f in range(len(is_sil)):
        n += 1
        sil = sil + 1 if is_sil[f] else 0
        speech = bool(speech or is_sp[f])
        reason = (2 if speech and sil >= silence_after_speech else 1 if sil >= silence_only
                  else 3 if n >= max_segment else 0)
        if reason:
            out.append((t - n + 1, t, reason))
            n, sil, speech = 0, 0, False
        t += 1
    st[:] = [n, sil, speech, t]
    return out


def margin(x, blank, blank_threshold):
    """The smallest |lp_blank - log(blank_threshold)| over the frames of x (inf for none)."""
    m = flags(x, blank, blank_threshold)[2]
    return float(m.min()) if m.size else float('inf')


def plan_logits(i, C, plan=None):
    """Stream i of width C: float32 [T, C], noise plus M on the class each frame speaks."""
    g = np.random.default_rng(11000 + i)
    x = g.standard_normal((T, C))
    blank = C - 1
    pos = 0
    for kind, n in (PLANS[i] if plan is None else plan):
        end = pos + n
        if kind == 'sil':
            x[pos:end, blank] += M
        else:
            q = pos
            while q < end:
                c, d = int(g.integers(0, C - 1)), int(g.integers(1, 3))
                x[q:min(q + d, end), c] += M
                q += d
                b = int(g.integers(1, 4))
                x[min(q, end):min(q + b, end), blank] += M
                q += b
        pos = end
    assert pos == T
    return x.astype(np.float32)


def batch(C):
    """The four plans at width C as one batch [4, T, C] float32."""
    return np.stack([plan_logits(i, C) for i in range(len(PLANS))])


# What the rule gives on the inputs above (checked in float64; tests/test_endpoint_cpu.py).
ANCHORS = {
    (8, 0): [(0, 33, 2), (34, 66, 2), (67, 78, 1), (79, 118, 3), (119, 126, 2)],
    (8, 1): [(40 * k, 40 * k + 39, 3) for k in range(4)],
    (8, 2): [(12 * k, 12 * k + 11, 1) for k in range(13)],
    (128, 3): [(0, 17, 2), (18, 32, 2), (33, 72, 3), (73, 100, 2), (101, 140, 3), (141, 152, 1)],
}
# smallest |lp_blank - log 0.8| over the four streams of a width (C = 8: 0.162 on plan 0, 0.133 on plan 2)
MARGINS = {8: 0.1326, 33: 0.0382, 128: 1.072e-3}
