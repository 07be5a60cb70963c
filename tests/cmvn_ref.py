"""Float64 numpy restatement of the sliding-window CMVN: the oracle of
tests/test_cmvn_gpu.py, pinned by the hand-computed anchors of tests/test_cmvn_cpu.py.

For frame t of one stream, with W the window:
    lo = max(0, t - W + 1), n = t - lo + 1, S1 = sum x[lo .. t], S2 = sum x[lo .. t]^2,
    c = min(W - n, count_p) (0 without a prior),
    m = (S1 + c mean_p) / (n + c), q = (S2 + c (std_p^2 + mean_p^2)) / (n + c),
    y = (x[t] - m) / sqrt(max(q - m m, 1e-10)), or x[t] - m without norm_vars.
Every sum is taken directly over its window, frame by frame, in ascending order (or, for
the conditioning check, descending); nothing is slid and nothing is rounded to float32.
"""
import numpy as np


def stream(x, window, norm_vars=True, prior=None, descending=False):
    """One stream: x [T, D] -> (y [T, D] float64, last) with last = (m [D], q [D], n + c) of
    frame T - 1, or None if T = 0.  prior: None or (mean [D], std [D], count)."""
    x = np.asarray(x, dtype=np.float64)
    T, D = x.shape
    W = int(window)
    y, last = np.zeros((T, D)), None
    pm = pq = np.zeros(D)
    pc = 0.0
    if prior is not None:
        pm, ps, pc = np.asarray(prior[0], dtype=np.float64), np.asarray(prior[1], dtype=np.float64), float(prior[2])
        pq = ps * ps + pm * pm
    for t in range(T):
        lo = max(0, t - W + 1)
        n = t - lo + 1
        s1, s2 = np.zeros(D), np.zeros(D)
        for u in (range(t, lo - 1, -1) if descending else range(lo, t + 1)):
            s1 = s1 + x[u]
            s2 = s2 + x[u] * x[u]
        c = min(float(W - n), pc)
        m, q = (s1 + c * pm) / (n + c), (s2 + c * pq) / (n + c)
        y[t] = (x[t] - m) / np.sqrt(np.maximum(q - m * m, 1e-10)) if norm_vars else x[t] - m
        last = (m, q, n + c)
    return y, last


def row_prior(prior, b):
    """Stream b's (mean [D], std [D], count) of a batch prior (mean, std, count): mean and
    std [D] or [B, D], count a number or [B]."""
    if prior is None:
        return None
    mean, std, count = np.asarray(prior[0]), np.asarray(prior[1]), np.asarray(prior[2], dtype=np.float64)
    return (mean if mean.ndim == 1 else mean[b], std if std.ndim == 1 else std[b],
            float(count) if count.ndim == 0 else float(count[b]))


def batch(x, lens, window, norm_vars=True, prior=None, descending=False):
    """x [B, Tmax, D], lens [B] -> (y [B, Tmax, D] float64 with zero rows past each length,
    lasts [B]: each stream's last-frame (m, q, n + c), None for a stream without frames)."""
    x = np.asarray(x)
    y, lasts = np.zeros(x.shape), []
    for b, T in enumerate(lens):
        y[b, :T], last = stream(x[b, :T], window, norm_vars, row_prior(prior, b), descending)
        lasts.append(last)
    return y, lasts


def carry(lasts, prior, speaker_frames, B, D):
    """The per-stream prior (mean [B, D], std [B, D], count [B]) of the next utterance: a
    stream with a last frame takes m, sqrt(max(q - m m, 0)) and min(speaker_frames, n + c);
    a stream without one keeps what ``prior`` gives it (None: a count of 0)."""
    mean, std, count = np.zeros((B, D)), np.ones((B, D)), np.zeros(B)
    for b in range(B):
        if lasts[b] is not None:
            m, q, k = lasts[b]
            mean[b], std[b], count[b] = m, np.sqrt(np.maximum(q - m * m, 0.0)), min(float(speaker_frames), k)
        elif prior is not None:
            mean[b], std[b], count[b] = row_prior(prior, b)
    return mean, std, count


def unit(y):
    """u = 2^-24 max(1, |y|): the rounding unit of the float32 result."""
    return 2.0 ** -24 * np.maximum(1.0, np.abs(y))


# ---- the fixed inputs of tests/test_cmvn_gpu.py (the conditioning check of
# tests/test_cmvn_cpu.py runs the oracle on the same ones)

def _params(rng, shape, D):
    k = (D + 2) // 3                      # static-like dimensions, then delta-like ones
    mean = np.concatenate([rng.uniform(8, 16, shape + (k,)), rng.uniform(-0.2, 0.2, shape + (D - k,))], axis=-1)
    std = np.concatenate([rng.uniform(2, 5, shape + (k,)), rng.uniform(0.4, 1.5, shape + (D - k,))], axis=-1)
    return mean, std


def features(B, T, D=123, seed=0):
    """[B, T, D] float32: every dimension Gaussian, static-like (means 8 .. 16, deviations
    2 .. 5) or delta-like (means +-0.2, deviations 0.4 .. 1.5)."""
    rng = np.random.default_rng(seed)
    mean, std = _params(rng, (), D)
    return (mean + std * rng.standard_normal((B, T, D))).astype(np.float32)


def prior_stats(D=123, rows=None, seed=11):
    """(mean, std) float32, [D] or [rows, D], from the same ranges."""
    mean, std = _params(np.random.default_rng(seed), () if rows is None else (rows,), D)
    return mean.astype(np.float32), std.astype(np.float32)


LENS3 = [50, 7, 0]
PRIOR_FRAMES = 5
# name -> (B, T, D, lens, window, prior rows: None (no prior), 0 (shared [D]) or B, prior_frames, seed)
SHAPES = {
    'acc': (3, 50, 123, LENS3, 16, None, PRIOR_FRAMES, 1),
    'acc_shared': (3, 50, 123, LENS3, 16, 0, PRIOR_FRAMES, 1),
    'acc_rows': (3, 50, 123, LENS3, 16, 3, PRIOR_FRAMES, 1),
    'chunk': (3, 130, 123, [130, 7, 0], 16, None, PRIOR_FRAMES, 1),     # long enough for the chunked runs
    'chunk_rows': (3, 130, 123, [130, 7, 0], 16, 3, PRIOR_FRAMES, 1),
    'w600': (1, 700, 123, [700], 600, 0, 200, 2),
    'long': (1, 2000, 123, [2000], 8, None, 0, 3),
    'w1': (2, 40, 123, [40, 33], 1, None, 0, 4),
    'd5': (2, 40, 5, [40, 33], 16, 2, PRIOR_FRAMES, 5),
    'd128': (2, 40, 128, [40, 33], 16, 2, PRIOR_FRAMES, 6),
}


def case(name):
    """dict(x float32 [B, T, D], lens, window, prior (mean, std) or None, prior_frames)."""
    B, T, D, lens, W, rows, frames, seed = SHAPES[name]
    prior = None if rows is None else prior_stats(D, rows or None)
    return dict(x=features(B, T, D, seed), lens=lens, window=W, prior=prior, prior_frames=frames)
