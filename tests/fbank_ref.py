"""numpy restatement of the waveform front end: Kaldi's
``compute-fbank-feats --num-mel-bins=40 --sample-frequency=16000 --use-energy=True``
(snip-edges, no dither), ``add-deltas`` (order 2, window 2) and the reference's CMVN.

``dtype=np.float64`` is the oracle.  ``dtype=np.float32`` is the error yardstick: the
same formulas with every array float32, the DFT a float32 matrix product with cosine
and sine tables rounded from float64.
"""
import numpy as np

FRAME_LEN, FRAME_SHIFT, N_FFT, N_BINS, N_MEL = 400, 160, 512, 256, 40
SAMPLE_RATE, LOW_FREQ, HIGH_FREQ, PREEMPH = 16000.0, 20.0, 8000.0, 0.97
N_STATIC, N_FEAT = N_MEL + 1, 3 * (N_MEL + 1)
FLT_EPSILON = float(np.finfo(np.float32).eps)
DELTA1 = np.array([-2, -1, 0, 1, 2], dtype=np.float64) / 10.0
DELTA2 = np.convolve(DELTA1, DELTA1)


def n_frames(n_samples):
    n = int(n_samples)
    return 0 if n < FRAME_LEN else 1 + (n - FRAME_LEN) // FRAME_SHIFT


def mel(f):
    return 1127.0 * np.log(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


def povey_window():
    i = np.arange(FRAME_LEN, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * i / (FRAME_LEN - 1))) ** 0.85


def mel_weights():
    """[40, 256] float64 triangular weights; bin k sits at mel(31.25 k)."""
    lo, hi = mel(LOW_FREQ), mel(HIGH_FREQ)
    step = (hi - lo) / (N_MEL + 1)
    m = mel(SAMPLE_RATE / N_FFT * np.arange(N_BINS))
    w = np.zeros((N_MEL, N_BINS))
    for f in range(N_MEL):
        left, center, right = lo + f * step, lo + (f + 1) * step, lo + (f + 2) * step
        inside = (m > left) & (m < right)
        up = (m - left) / (center - left)
        down = (right - m) / (right - center)
        w[f] = np.where(inside, np.where(m <= center, up, down), 0.0)
    return w


def _dft_tables():
    n = np.arange(N_FFT, dtype=np.float64)[:, None]
    k = np.arange(N_BINS, dtype=np.float64)[None, :]
    ang = 2.0 * np.pi * ((n * k) % N_FFT) / N_FFT
    return np.cos(ang), np.sin(ang)


def static(samples, dtype=np.float64):
    """samples [n] (int16 scale) -> [T, 41]: log energy, then the 40 log-mel values."""
    x = np.asarray(samples).astype(dtype)
    T = n_frames(x.shape[0])
    out = np.zeros((T, N_STATIC), dtype=dtype)
    if T == 0:
        return out
    idx = FRAME_SHIFT * np.arange(T)[:, None] + np.arange(FRAME_LEN)[None, :]
    fr = x[idx]
    fr = fr - fr.mean(axis=1, keepdims=True, dtype=dtype)
    energy = (fr * fr).sum(axis=1, dtype=dtype)
    pre = fr.copy()
    pre[:, 1:] = fr[:, 1:] - dtype(PREEMPH) * fr[:, :-1]
    pre[:, 0] = fr[:, 0] - dtype(PREEMPH) * fr[:, 0]
    pre = pre * povey_window().astype(dtype)
    padded = np.zeros((T, N_FFT), dtype=dtype)
    padded[:, :FRAME_LEN] = pre
    c, s = _dft_tables()
    re, im = padded @ c.astype(dtype), padded @ s.astype(dtype)
    power = re * re + im * im
    melE = power @ mel_weights().T.astype(dtype)
    eps = dtype(FLT_EPSILON)
    out[:, 0] = np.log(np.maximum(energy, eps))
    out[:, 1:] = np.log(np.maximum(melE, eps))
    assert out.dtype == dtype
    return out


def add_deltas(st, dtype=np.float64):
    """[T, 41] -> [T, 123] = [static | delta | delta-delta], frame index clamped."""
    st = np.asarray(st, dtype=dtype)
    T = st.shape[0]
    out = np.zeros((T, N_FEAT), dtype=dtype)
    if T == 0:
        return out
    t = np.arange(T)
    out[:, :N_STATIC] = st
    for j, c in enumerate(DELTA1):
        out[:, N_STATIC:2 * N_STATIC] += dtype(c) * st[np.clip(t + j - 2, 0, T - 1)]
    for j, c in enumerate(DELTA2):
        out[:, 2 * N_STATIC:] += dtype(c) * st[np.clip(t + j - 4, 0, T - 1)]
    return out


def cmvn(feats, mean, std, dtype=np.float64):
    return ((feats - np.asarray(mean, dtype=dtype) + dtype(1e-14)) / (np.asarray(std, dtype=dtype) + dtype(1e-14))
            ).astype(dtype)


def features(samples, mean=None, std=None, dtype=np.float64):
    f = add_deltas(static(samples, dtype), dtype)
    return f if mean is None else cmvn(f, mean, std, dtype)


def batch(samples, n_samples, mean=None, std=None, dtype=np.float64, statics_only=False):
    """samples [B, N], n_samples [B] -> ([B, Tmax, 41 or 123] zero padded, n_frames [B]);
    mean / std are [123] or [B, 123]."""
    B = len(n_samples)
    T = [n_frames(n) for n in n_samples]
    D = N_STATIC if statics_only else N_FEAT
    out = np.zeros((B, max(T), D), dtype=dtype)
    for b in range(B):
        x = np.asarray(samples[b])[:int(n_samples[b])]
        if statics_only:
            out[b, :T[b]] = static(x, dtype)
        else:
            m = None if mean is None else (np.asarray(mean)[b] if np.ndim(mean) == 2 else mean)
            s = None if std is None else (np.asarray(std)[b] if np.ndim(std) == 2 else std)
            out[b, :T[b]] = features(x, m, s, dtype)
    return out, np.array(T, dtype=np.int64)


def signal_noise(n):
    """Signal 1: integer noise, x[n] = (7 n^2 + 13 n) mod 4001 - 1900."""
    i = np.arange(n, dtype=np.int64)
    return ((7 * i * i + 13 * i) % 4001 - 1900).astype(np.int16)


def signal_wide(n):
    """Signal 2: two tones (one swept) over weak integer noise and a DC offset."""
    i = np.arange(n, dtype=np.int64)
    t = i / SAMPLE_RATE
    x = (3000.0 * np.sin(2 * np.pi * 440.0 * t) + 1500.0 * np.sin(2 * np.pi * (300.0 + 4000.0 * t) * t)
         + ((7 * i * i + 13 * i) % 401 - 200) + 120.0)
    return np.round(x).astype(np.int16)
