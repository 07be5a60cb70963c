"""numpy restatement of the resampler: Kaldi's ``LinearResample`` as
``ResampleWaveform`` configures it (cutoff 0.99 of the lower Nyquist frequency, 6 zeros).

``dtype=np.float64`` is the oracle.  ``dtype=np.float32`` is the error yardstick: the
weights rounded once to float32 and the sum taken in float32 in tap order (a product, then
an add, per tap).  ``bound`` is the per-output sum of |w x| that the rounding limit of
tests/test_resample_gpu.py scales.
"""
import math

import numpy as np

from tests.fbank_ref import signal_noise, signal_wide  # noqa: F401  (the test signals are shared)

ZEROS = 6


class Filter:
    """``iu``, ``ou``, ``taps``, ``first`` [ou] int64 and ``w`` [ou, taps] float64 of fin -> fout."""

    def __init__(self, fin, fout):
        fin, fout = int(fin), int(fout)
        g = math.gcd(fin, fout)
        self.fin, self.fout, self.iu, self.ou = fin, fout, fin // g, fout // g
        if fin == fout:   # Kaldi's tools resample only when the rates differ: the exact copy
            self.fc, self.ww, self.taps = None, 0.0, 1
            self.first, self.w = np.zeros(1, dtype=np.int64), np.ones((1, 1))
            return
        self.fc = 0.99 * 0.5 * min(fin, fout)
        self.ww = ZEROS / (2.0 * self.fc)
        t = np.arange(self.ou) / float(fout)
        self.first = np.ceil((t - self.ww) * fin).astype(np.int64)
        last = np.floor((t + self.ww) * fin).astype(np.int64)
        self.taps = int((last - self.first + 1).max())
        d = (self.first[:, None] + np.arange(self.taps)[None, :]) / float(fin) - t[:, None]
        win = np.where(np.abs(d) < self.ww, 0.5 * (1.0 + np.cos(2.0 * np.pi * self.fc / ZEROS * d)), 0.0)
        safe = np.where(d == 0.0, 1.0, d)
        filt = np.where(d == 0.0, 2.0 * self.fc, np.sin(2.0 * np.pi * self.fc * safe) / (np.pi * safe))
        self.w = win * filt / fin

    def n_out(self, n):
        return -((-int(n) * self.ou) // self.iu)   # ceil(n ou / iu), exact in Python ints


def _gather(f, x):
    """x [n] -> (inputs [M, taps] float64 with zeros outside [0, n), phase [M]), M = n_out(n)."""
    x = np.asarray(x).astype(np.float64)
    n, M = x.shape[0], f.n_out(x.shape[0])
    o = np.arange(M, dtype=np.int64)
    p, u = o % f.ou, o // f.ou
    idx = (f.first[p] + u * f.iu)[:, None] + np.arange(f.taps)[None, :]
    inside = (idx >= 0) & (idx < n)
    xp = np.concatenate([x, [0.0]])
    return np.where(inside, xp[np.clip(idx, 0, n)], 0.0), p


def resample(f, x, dtype=np.float64):
    """x [n] (int16 scale) -> [n_out(n)] of ``dtype``."""
    xi, p = _gather(f, x)
    if dtype == np.float64:
        return (f.w[p] * xi).sum(axis=1)
    w, xi = f.w[p].astype(np.float32), xi.astype(np.float32)
    acc = np.zeros(xi.shape[0], dtype=np.float32)
    for j in range(f.taps):
        acc = acc + w[:, j] * xi[:, j]
    assert acc.dtype == np.float32
    return acc


def bound(f, x, dtype=np.float64):
    """Per output sample: sum_j |w64[p][j] x_j| (float64 whatever ``dtype``)."""
    xi, p = _gather(f, x)
    return np.abs(f.w[p] * xi).sum(axis=1)


def batch(filters, choice, samples, n_samples, dtype=np.float64, what=resample):
    """samples [B, N], row b through filters[choice[b]] at length n_samples[b] ->
    ([B, Mmax] zero padded, n_out [B]); Mmax is n_out(N) at the lowest input rate."""
    N = np.asarray(samples).shape[1]
    lowest = min(filters, key=lambda f: f.fin)
    n_out = [filters[c].n_out(n) for c, n in zip(choice, n_samples)]
    out = np.zeros((len(n_samples), lowest.n_out(N)), dtype=dtype)
    for b, (c, n) in enumerate(zip(choice, n_samples)):
        out[b, :n_out[b]] = what(filters[c], np.asarray(samples[b])[:int(n)], dtype)
    return out, np.array(n_out, dtype=np.int64)


def stream_final_brute(f, pushed):
    """Outputs whose last padded tap has arrived after ``pushed`` inputs, counted one by one."""
    o = 0
    while f.first[o % f.ou] + (o // f.ou) * f.iu + f.taps - 1 <= pushed - 1:
        o += 1
    return o
