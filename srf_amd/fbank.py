"""Device front end: 16 kHz waveform to the 123-d filterbank features the model reads.

The reference prepares its input with Kaldi (``egs/script/fbank123.sh``):
``compute-fbank-feats --num-mel-bins=40 --sample-frequency=16000 --use-log-fbank=True
--use-energy=True``, ``add-deltas`` and per-speaker CMVN, which ``save_speech_data.py:163``
applies as ``(feats - mean + 1e-14) / (std + 1e-14)``.  This module is that recipe as HIP
kernels (``csrc/fbank.hip``): ``Fbank`` offline, ``FbankStream`` in
chunks, ``CmvnStats`` for the mean and the deviation.  Samples are in int16 scale, int16
or float32; everything stays on the device.

A live stream has no per-speaker statistics: ``SlidingCmvn`` (``csrc/cmvn.hip``, DESIGN.md
section 20) normalises every frame with the frames before it, offline and, as
``SlidingCmvnStream``, in chunks with the same bits; ``Fbank(cmvn=SlidingCmvn(...))`` puts it
behind the deltas.
"""
import ctypes

import numpy as np
import torch

from . import _lib, ops
from .streaming import check_ended

FRAME_LEN, FRAME_SHIFT = 400, 160      # SRF_FBANK_FRAME_LEN, SRF_FBANK_FRAME_SHIFT
N_STATIC, N_FEAT = 41, 123             # SRF_FBANK_STATIC, SRF_FBANK_FEAT
DELTA_CONTEXT = 4                      # the delta-delta of frame t reads statics t - 4 .. t + 4
_NO_END = 1 << 30                      # length of a stream whose end is not known yet (device side)


def n_frames(n_samples):
    """Frames of an utterance of ``n_samples`` samples (snip-edges: 25 ms frames every
    10 ms, whole frames only): 0 below 400 samples, else 1 + (n - 400) // 160.  An int, a
    sequence or a tensor."""
    if isinstance(n_samples, torch.Tensor):
        n = n_samples.to(torch.int64)
        return torch.where(n < FRAME_LEN, torch.zeros_like(n), 1 + (n - FRAME_LEN) // FRAME_SHIFT)
    if isinstance(n_samples, (list, tuple, np.ndarray)):
        return [n_frames(int(n)) for n in n_samples]
    n = int(n_samples)
    return 0 if n < FRAME_LEN else 1 + (n - FRAME_LEN) // FRAME_SHIFT


def tables():
    """The kernels' constant tables (float32 numpy), as srf_fbank_tables computes them on
    the host in double: dict of ``window`` [400], ``twiddle`` [256, 2] (cos, -sin of
    2 pi k / 512), ``mel_first`` [40], ``mel_count`` [40] and ``mel_weights`` [40, slots]."""
    flat = _tables_flat()
    slots = (flat.size - 992) // 40
    return {'window': flat[:400].copy(), 'twiddle': flat[400:912].reshape(256, 2).copy(),
            'mel_first': flat[912:952].astype(np.int64), 'mel_count': flat[952:992].astype(np.int64),
            'mel_weights': flat[992:].reshape(40, slots).copy()}


def _tables_flat():
    L = _lib.lib()
    n = L.srf_fbank_table_floats()
    buf = np.empty(n, dtype=np.float32)
    _lib.check(L.srf_fbank_tables(buf.ctypes.data_as(ctypes.c_void_p), n), 'srf_fbank_tables')
    return buf


def _samples_arg(samples, device, what):
    if samples.dim() != 2:
        raise ValueError(f'{what} must be [B, n], got {tuple(samples.shape)}')
    if samples.dtype not in (torch.int16, torch.float32):
        raise ValueError(f'{what} must be int16 or float32 (int16 scale), got {samples.dtype}')
    return samples.to(device).contiguous()


def _require_device(t, what):
    if not t.is_cuda:
        raise ValueError(f'{what} must be on a HIP device (no CPU path exists)')


class Fbank:
    """``fe(samples [B, N], n_samples [B])`` -> ``(feats [B, Tmax, 123], n_frames [B])`` on
    the device, usable as ``model(feats, input_lengths=n_frames, ...)``: per frame the log
    energy and 40 log-mel values, their deltas and delta-deltas, then the CMVN.  Rows past
    an utterance's last frame are zero; Tmax is ``n_frames(N)``.

    ``cmvn``: None, or ``(mean, std)``, each [123] or [B, 123] (per stream or speaker):
    ``y = (x - mean + 1e-14) / (std + 1e-14)``; or a ``SlidingCmvn``, the online
    normalisation of a live stream, applied to the finished features by a launch of its own.

    ``dither``: amplitude of the Gaussian noise added to every sample before anything
    else.  It is OFF by default (0.0): Kaldi's own default of 1.0 draws from the C
    library's generator and cannot be reproduced, so a default that matches it in name only
    would make features depend on an unstated seed.  With ``dither = a > 0`` the noise is
    ``a * g``, g a standard Gaussian keyed by ``(seed, stream row, global sample index)``:
    a property of the signal, the same for overlapping frames and for every chunking."""

    def __init__(self, dither=0.0, seed=0, cmvn=None, device='cuda'):
        if not (float(dither) >= 0.0 and float(dither) < float('inf')):
            raise ValueError(f'dither must be finite and >= 0, got {dither}')
        self.dither, self.seed, self.device = float(dither), int(seed) & (2 ** 64 - 1), torch.device(device)
        self.tables = torch.from_numpy(_tables_flat()).to(self.device)
        self.mean = self.std = self.sliding = None
        if isinstance(cmvn, SlidingCmvn):
            if cmvn.dim != N_FEAT or cmvn.device.type != self.device.type:
                raise ValueError(f'the sliding CMVN is for {cmvn.dim}-d features on {cmvn.device}, the front end makes '
                                 f'{N_FEAT}-d features on {self.device}')
            self.sliding = cmvn
        elif cmvn is not None:
            mean, std = (torch.as_tensor(np.asarray(c.detach().cpu() if isinstance(c, torch.Tensor) else c,
                                                    dtype=np.float32)) for c in cmvn)
            if mean.shape != std.shape or mean.dim() not in (1, 2) or mean.shape[-1] != N_FEAT:
                raise ValueError(f'cmvn mean and std must both be [{N_FEAT}] or [B, {N_FEAT}], got '
                                 f'{tuple(mean.shape)} and {tuple(std.shape)}')
            self.mean, self.std = mean.to(self.device).contiguous(), std.to(self.device).contiguous()

    def cmvn_rows(self, B):
        """srf_fbank_deltas' cmvn_rows for a batch of B streams."""
        if self.mean is None:
            return 0
        if self.mean.dim() == 1:
            return 1
        if self.mean.shape[0] != B:
            raise ValueError(f'the CMVN has {self.mean.shape[0]} rows, the batch {B} streams')
        return B

    # the two launches, on buffers with an origin (the streaming path calls them too)
    def _static(self, samples, n_samples, width, s0, n_limit, t0, t1, statics, f0):
        _require_device(samples, 'samples')
        B, stride = samples.shape
        _lib.check(_lib.lib().srf_fbank_static(
            ops._ptr(samples), int(samples.dtype == torch.int16), ops._ptr(n_samples), ops._ptr(self.tables), B, stride,
            width, s0, n_limit, t0, t1, f0, statics.shape[1], self.dither, self.seed, ops._ptr(statics),
            ops._stream()), 'srf_fbank_static')

    def _deltas(self, statics, n_fr, f0, t_limit, t0, t1, feats, o0):
        B = statics.shape[0]
        rows = self.cmvn_rows(B)
        _lib.check(_lib.lib().srf_fbank_deltas(
            ops._ptr(statics), ops._ptr(n_fr), B, statics.shape[1], f0, t_limit, t0, t1,
            ops._ptr(self.mean) if rows else None, ops._ptr(self.std) if rows else None, rows, ops._ptr(feats),
            feats.shape[1], o0, ops._stream()), 'srf_fbank_deltas')

    def _lengths(self, samples, n_samples):
        B, N = samples.shape
        n = torch.as_tensor(n_samples).to(self.device).reshape(-1)
        if n.shape[0] != B:
            raise ValueError(f'n_samples has {n.shape[0]} entries for {B} utterances')
        return n.clamp(0, N).to(torch.int32).contiguous()

    def static(self, samples, n_samples):
        """The 41-d statics alone: ``([B, Tmax, 41], n_frames [B])``."""
        samples = _samples_arg(samples, self.device, 'samples')
        n = self._lengths(samples, n_samples)
        B, N = samples.shape
        T = n_frames(N)
        statics = torch.empty((B, T, N_STATIC), device=self.device, dtype=torch.float32)
        if T:
            self._static(samples, n, N, 0, N, 0, T, statics, 0)
        return statics, n_frames(n).to(torch.int32)

    def __call__(self, samples, n_samples):
        statics, n_fr = self.static(samples, n_samples)
        B, T, _ = statics.shape
        feats = torch.empty((B, T, N_FEAT), device=self.device, dtype=torch.float32)
        if T:
            self._deltas(statics, n_fr, 0, T, 0, T, feats, 0)
        if self.sliding is not None:
            feats = self.sliding(feats, n_fr)
        return feats, n_fr


class CmvnStats:
    """Mean and deviation of feature rows, accumulated on the device in fp64.
    ``update_state(feats [B, T, D], n_frames [B])`` is one launch over the rows
    ``t < n_frames[b]`` and reads nothing back; ``result()`` -> ``(mean, std)`` float64 numpy,
    ``std = sqrt(sum x^2 / n - mean^2)``.  ``save`` / ``load`` use the reference's text format:
    two rows, ``np.loadtxt`` gives ``[mean; std]`` (misc_helper.load_cmvn)."""

    def __init__(self, dim=N_FEAT, device='cuda'):
        self.dim, self.device = int(dim), torch.device(device)
        self.sums = torch.zeros(2 * self.dim + 1, device=self.device, dtype=torch.float64)

    def reset_state(self):
        self.sums.zero_()

    def update_state(self, feats, n_frames):
        _require_device(feats, 'feats')
        if feats.dim() != 3 or feats.shape[2] != self.dim or feats.dtype != torch.float32:
            raise ValueError(f'feats must be float32 [B, T, {self.dim}], got {feats.dtype} {tuple(feats.shape)}')
        B, T, D = feats.shape
        n = ops._i32(torch.as_tensor(n_frames).to(self.device).reshape(-1))
        if n.shape[0] != B:
            raise ValueError(f'n_frames has {n.shape[0]} entries for {B} utterances')
        feats = feats.contiguous()
        _lib.check(_lib.lib().srf_fbank_stats(ops._ptr(feats), ops._ptr(n), B, T, D, ops._ptr(self.sums),
                                              ops._stream()), 'srf_fbank_stats')

    def result(self):
        s = self.sums.cpu().numpy()
        n = s[-1]
        if n <= 0:
            raise ValueError('no frames were accumulated')
        mean = s[:self.dim] / n
        return mean, np.sqrt(np.maximum(s[self.dim:2 * self.dim] / n - mean * mean, 0.0))

    def save(self, path):
        save_cmvn(path, *self.result())


def save_cmvn(path, mean, std):
    np.savetxt(path, np.stack([np.asarray(mean, dtype=np.float64), np.asarray(std, dtype=np.float64)]), fmt='%.17g')


def load_cmvn(path):
    """``(mean, std)`` of a CMVN file in the reference's format."""
    m = np.loadtxt(path)
    if m.ndim != 2 or m.shape[0] != 2:
        raise ValueError(f'{path}: a CMVN file holds two rows (mean, std), got shape {m.shape}')
    return m[0], m[1]


CMVN_TILE, CMVN_MAX_DIM, CMVN_MAX_WINDOW = 32, 128, 4096   # SRF_CMVN_TILE, SRF_CMVN_MAX_DIM, SRF_CMVN_MAX_WINDOW


def _frame_counts(n_frames, B, device):
    """n_frames [B] as an int32 device tensor.  Counts given on the host are checked here;
    a device tensor is not read back: the kernel takes a negative count as 0."""
    if not (isinstance(n_frames, torch.Tensor) and n_frames.is_cuda):
        host = np.asarray(n_frames.cpu() if isinstance(n_frames, torch.Tensor) else n_frames).reshape(-1)
        if host.size and host.min() < 0:
            raise ValueError(f'n_frames must be >= 0, got {host.tolist()}')
        n_frames = torch.as_tensor(host.astype(np.int32))
    n = n_frames.reshape(-1)
    if n.shape[0] != B:
        raise ValueError(f'n_frames has {n.shape[0]} entries for {B} streams')
    return ops._i32(n.to(device))


class SlidingCmvn:
    """Online (sliding-window) CMVN: ``sc(feats [B, T, D] float32, n_frames [B])`` -> the
    normalised [B, T, D] on the device, one launch (csrc/cmvn.hip).

    Frame t is normalised with the mean and, with ``norm_vars``, the deviation of the
    ``window`` frames that end with it, nothing after it.  While the window holds n < window
    frames, a ``prior`` ``(mean, std)``, each [D] or [B, D] (what ``load_cmvn`` returns),
    stands in for ``min(window - n, prior_frames)`` of the missing ones.  In fp64, rounded
    once: with S1, S2 the sums of x and x^2 over the window and c that count,
    ``m = (S1 + c mean_p) / (n + c)``, ``q = (S2 + c (std_p^2 + mean_p^2)) / (n + c)``,
    ``y = (x - m) / sqrt(max(q - m^2, 1e-10))``, or ``x - m`` without ``norm_vars``.
    Rows at ``t >= n_frames[b]`` are zero.  ``speaker_frames`` caps what a
    ``SlidingCmvnStream`` carries from one utterance of a speaker into the next.

    Counts given on the host are checked (negative: ``ValueError``); a device tensor is not
    read back, the kernel takes a negative count as 0."""

    def __init__(self, window=600, norm_vars=True, prior=None, prior_frames=200, speaker_frames=600, dim=N_FEAT,
                 device='cuda'):
        if int(window) != window or not 1 <= int(window) <= CMVN_MAX_WINDOW:
            raise ValueError(f'window must be an integer in 1 .. {CMVN_MAX_WINDOW}, got {window}')
        if int(dim) != dim or not 1 <= int(dim) <= CMVN_MAX_DIM:
            raise ValueError(f'dim must be an integer in 1 .. {CMVN_MAX_DIM}, got {dim}')
        if not (0 <= float(prior_frames) < float('inf') and 0 <= float(speaker_frames) < float('inf')):
            raise ValueError(f'prior_frames and speaker_frames must be finite and >= 0, got {prior_frames} and '
                             f'{speaker_frames}')
        self.window, self.norm_vars, self.dim, self.device = int(window), bool(norm_vars), int(dim), torch.device(device)
        self.prior_frames, self.speaker_frames = float(prior_frames), float(speaker_frames)
        self.mean = self.std = self.count = None
        if prior is not None:
            mean, std = (np.asarray(c.detach().cpu() if isinstance(c, torch.Tensor) else c, dtype=np.float64)
                         for c in prior)
            if mean.shape != std.shape or mean.ndim not in (1, 2) or mean.shape[-1] != self.dim or 0 in mean.shape:
                raise ValueError(f'the prior mean and std must both be [{self.dim}] or [B, {self.dim}], got '
                                 f'{mean.shape} and {std.shape}')
            if not (np.isfinite(mean).all() and np.isfinite(std).all() and (std > 0).all()):
                raise ValueError('the prior must be finite and its std positive')
            rows = 1 if mean.ndim == 1 else mean.shape[0]
            self.mean = torch.from_numpy(mean.reshape(rows, self.dim).copy()).to(self.device)
            self.std = torch.from_numpy(std.reshape(rows, self.dim).copy()).to(self.device)
            self.count = torch.full((rows,), self.prior_frames, dtype=torch.float64, device=self.device)
            self._shared = mean.ndim == 1

    def prior_rows(self, B):
        """srf_cmvn_sliding's prior_rows for a batch of B streams."""
        if self.mean is None:
            return 0
        if self._shared:
            return 1
        if self.mean.shape[0] != B:
            raise ValueError(f'the prior has {self.mean.shape[0]} rows, the batch {B} streams')
        return B

    # the launch, on buffers with an origin (the streaming path calls it too)
    def _launch(self, feats, n_fr, f0, t0, t1, prior, out, o0, last):
        B, rows, D = feats.shape
        mean, std, count = prior if prior is not None else (None, None, None)
        _lib.check(_lib.lib().srf_cmvn_sliding(
            ops._ptr(feats), ops._ptr(n_fr), B, rows, D, f0, t0, t1,
            None if mean is None else ops._ptr(mean), None if mean is None else ops._ptr(std),
            None if mean is None else ops._ptr(count), 0 if mean is None else count.shape[0], self.window,
            int(self.norm_vars), ops._ptr(out), out.shape[1], o0, None if last is None else ops._ptr(last),
            ops._stream()), 'srf_cmvn_sliding')

    def _check_feats(self, feats, lead):
        if feats.dim() != 3 or feats.shape[0] != lead or feats.shape[2] != self.dim or feats.dtype != torch.float32:
            raise ValueError(f'feats must be float32 [{lead}, T, {self.dim}], got {feats.dtype} {tuple(feats.shape)}')

    def __call__(self, feats, n_frames):
        if not isinstance(feats, torch.Tensor) or feats.dim() != 3:
            raise ValueError(f'feats must be float32 [B, T, {self.dim}]')
        self._check_feats(feats, feats.shape[0])
        B, T, _ = feats.shape
        n = _frame_counts(n_frames, B, self.device)
        _require_device(feats, 'feats')
        rows = self.prior_rows(B)
        feats = feats.contiguous()
        out = torch.empty_like(feats)
        if B and T:
            self._launch(feats, n, 0, 0, T, (self.mean, self.std, self.count) if rows else None, out, 0, None)
        return out


class SlidingCmvnStream:
    """``sc`` over ``n_streams`` feature streams that arrive in chunks, in lock step.

    ``push(feats [B, m, D], n_frames_total=None)`` takes the next m <= ``max_frames`` frames
    of every stream and returns the same m frames normalised: no latency.  The concatenated
    output equals ``sc`` on the whole streams bit for bit, whatever the chunking.
    ``n_frames_total`` follows ``StreamingRouter.push``'s ``ended``: the total frame count of
    a stream whose end lies in this chunk, else -1 (rows past a stream's end come out zero);
    or an int32 device tensor [B] of total counts that is used as it is and not read back,
    any value beyond the frames pushed meaning "not yet".

    ``reset()`` puts every stream back at its start with the constructor's prior;
    ``reset(carry=True)`` makes what each stream's last frame was normalised with the prior
    of its next utterance: mean m, deviation sqrt(max(q - m^2, 0)), worth
    ``min(speaker_frames, n + c)`` frames.  A stream that had no frames keeps its prior.

    Device-resident state: ``history`` [B, window - 1 + CMVN_TILE + max_frames, D], the raw
    frames later frames still need (at most window - 1 frames plus one tile after a chunk,
    slid to the front by srf_stream_advance_n); ``last`` [B, 2 D + 1] fp64, [m | q | n + c]
    of each stream's latest frame; the per-stream prior ``prior_mean``, ``prior_std``
    [B, D] and ``prior_count`` [B], fp64."""

    def __init__(self, sc, n_streams, max_frames):
        if int(n_streams) < 1 or int(max_frames) < 1:
            raise ValueError(f'n_streams and max_frames must be >= 1, got {n_streams} and {max_frames}')
        self.sc, self.B, self.max_frames = sc, int(n_streams), int(max_frames)
        sc.prior_rows(self.B)
        dev, D = sc.device, sc.dim
        self.rows = sc.window - 1 + CMVN_TILE + self.max_frames
        self.history = torch.zeros((self.B, self.rows, D), device=dev, dtype=torch.float32)
        self.last = torch.zeros((self.B, 2 * D + 1), device=dev, dtype=torch.float64)
        self.prior_mean = torch.zeros((self.B, D), device=dev, dtype=torch.float64)
        self.prior_std = torch.ones((self.B, D), device=dev, dtype=torch.float64)
        self.prior_count = torch.zeros((self.B,), device=dev, dtype=torch.float64)
        self._nfr_dev = torch.full((self.B,), _NO_END, device=dev, dtype=torch.int32)
        self.reset()

    def reset(self, carry=False):
        sc, D = self.sc, self.sc.dim
        if carry:
            m, q, cnt = self.last[:, :D], self.last[:, D:2 * D], self.last[:, 2 * D]
            had = cnt > 0
            self.prior_mean = torch.where(had[:, None], m, self.prior_mean)
            self.prior_std = torch.where(had[:, None], torch.sqrt(torch.clamp(q - m * m, min=0.0)), self.prior_std)
            self.prior_count = torch.where(had, torch.clamp(cnt, max=sc.speaker_frames), self.prior_count)
        elif sc.mean is not None:
            self.prior_mean.copy_(sc.mean.expand(self.B, D))
            self.prior_std.copy_(sc.std.expand(self.B, D))
            self.prior_count.copy_(sc.count.expand(self.B))
        else:
            self.prior_count.zero_()   # a count of 0 takes the prior out of every frame
        self.last.zero_()
        self._nfr_dev.fill_(_NO_END)
        self.lengths = [None] * self.B   # declared frame counts
        self.pushed = 0                  # frames taken (and returned) per stream
        self._f0 = 0                     # the history's first frame

    def _normalise(self, t0, t1, n_fr):
        """Frames [t0, t1), which the history holds, normalised: [B, t1 - t0, D]."""
        out = torch.empty((self.B, t1 - t0, self.sc.dim), device=self.sc.device, dtype=torch.float32)
        self.sc._launch(self.history, n_fr, self._f0, t0, t1, (self.prior_mean, self.prior_std, self.prior_count),
                        out, t0, self.last)
        self.pushed = t1
        return out

    def _slide(self):
        """The history's entry of a stream_advance call: drop the frames that no frame from
        ``pushed`` on reads, those before the window of its tile's first frame."""
        f0 = max(0, self.pushed // CMVN_TILE * CMVN_TILE - self.sc.window + 1)
        shift, self._f0 = f0 - self._f0, f0
        return self.history, self.rows, shift, self.pushed - f0

    def push(self, feats, n_frames_total=None):
        if not isinstance(feats, torch.Tensor) or feats.dim() != 3:
            raise ValueError(f'feats must be float32 [{self.B}, m, {self.sc.dim}]')
        self.sc._check_feats(feats, self.B)
        m = feats.shape[1]
        if m > self.max_frames:
            raise ValueError(f'a chunk holds at most max_frames = {self.max_frames} frames, got {m}')
        n_fr = self._nfr_dev
        if isinstance(n_frames_total, torch.Tensor) and n_frames_total.is_cuda:
            n_fr = _frame_counts(n_frames_total, self.B, self.sc.device)
        elif n_frames_total is not None:
            lengths = check_ended(self.lengths, n_frames_total, self.pushed, m)
            if lengths != self.lengths:
                self.lengths = lengths
                self._nfr_dev.copy_(torch.tensor([_NO_END if e is None else e for e in lengths], dtype=torch.int32))
        _require_device(feats, 'feats')
        if not m:
            return feats.new_empty((self.B, 0, self.sc.dim))
        t0 = self.pushed
        self.history[:, t0 - self._f0:t0 - self._f0 + m] = feats
        out = self._normalise(t0, t0 + m, n_fr)
        ops.stream_advance([self._slide()])
        return out


class FbankStream:
    """``fe`` over ``n_streams`` signals that arrive in chunks, in lock step.

    ``push(samples [B, n], ended=None)`` takes the next n <= ``max_samples`` samples of
    every stream and returns the feature frames [B, m, 123] that became final, frames
    ``frames_out - m .. frames_out - 1`` of every stream; ``ended`` follows
    ``StreamingRouter.push``: the total sample count of a stream whose end lies in this
    chunk, else -1 (what a chunk holds past a stream's end is ignored).  The concatenated
    output equals ``fe`` on the whole signals bit for bit, whatever the chunking.

    A frame is final once the four frames after it are (its delta-delta reads statics
    t - 4 .. t + 4), so an unfinished stream holds back 4 frames (40 ms) besides the
    samples of its incomplete frame; a stream that ended clamps at its last frame.  While
    a stream is unfinished the output runs to 4 frames short of the frames the pushed
    samples hold; rows past an ended stream's last frame are zero, as in ``fe``'s padding.
    Once every stream has ended the output runs to the longest stream's end.
    ``finish()`` ends every stream that has not declared an end at what was pushed.

    Device-resident state: the sample tail (at most 399 samples) and the last 8 static
    frames, each slid to the front of its buffer after a chunk (srf_stream_advance_n); on a
    front end with a ``SlidingCmvn`` also a ``SlidingCmvnStream``, through which every batch of
    final frames goes (one more launch per chunk, its history slid by the same call)."""

    def __init__(self, fe, n_streams, max_samples):
        if int(n_streams) < 1 or int(max_samples) < 1:
            raise ValueError(f'n_streams and max_samples must be >= 1, got {n_streams} and {max_samples}')
        self.fe, self.B, self.max_samples = fe, int(n_streams), int(max_samples)
        fe.cmvn_rows(self.B)
        dev = fe.device
        self._cap = FRAME_LEN - 1 + self.max_samples
        self._max_new = self.max_samples // FRAME_SHIFT + 1          # static frames one chunk completes
        self._rows = self._max_new + 3 * DELTA_CONTEXT
        self._buf = torch.zeros((self.B, self._cap), device=dev, dtype=torch.float32)
        self._st = torch.zeros((self.B, self._rows, N_STATIC), device=dev, dtype=torch.float32)
        self._len_dev = torch.full((self.B,), _NO_END, device=dev, dtype=torch.int32)
        self._nfr_dev = torch.full((self.B,), _NO_END, device=dev, dtype=torch.int32)
        # with a sliding CMVN the deltas go into its stream's history and every batch of final
        # frames (at most _max_new, plus the 4 held back once the streams end) through it
        self._cmvn = None
        if fe.sliding is not None:
            self._cmvn = SlidingCmvnStream(fe.sliding, self.B, self._max_new + DELTA_CONTEXT)
        self.reset()

    def reset(self, carry=False):
        """Every stream back at its start; ``carry``: the sliding CMVN takes what it learnt
        about each stream's speaker along as the next utterance's prior
        (``SlidingCmvnStream.reset``)."""
        if self._cmvn is not None:
            self._cmvn.reset(carry=carry)
        elif carry:
            raise ValueError('there is nothing to carry: the front end has no sliding CMVN')
        self._len_dev.fill_(_NO_END)
        self._nfr_dev.fill_(_NO_END)
        self.lengths = [None] * self.B   # declared sample counts
        self.pushed = 0                  # samples taken per stream
        self.frames_out = 0              # feature frames returned per stream
        self._tail = 0                   # samples held: the global samples pushed - _tail .. pushed - 1
        self._static_done = 0            # static frames computed
        self._done = False               # every stream has ended and its frames are out

    def _empty(self):
        return torch.empty((self.B, 0, N_FEAT), device=self.fe.device, dtype=torch.float32)

    def push(self, samples, ended=None):
        if samples.dim() != 2 or samples.shape[0] != self.B:
            raise ValueError(f'samples must be [{self.B}, n], got {tuple(samples.shape)}')
        n = samples.shape[1]
        if n > self.max_samples:
            raise ValueError(f'a chunk holds at most max_samples = {self.max_samples} samples, got {n}')
        lengths = check_ended(self.lengths, ended, self.pushed, n, unit='samples')
        samples = _samples_arg(samples, self.fe.device, 'samples')
        _require_device(samples, 'samples')
        return self._step(samples, lengths)

    def finish(self):
        """Ends every stream that has not declared an end; returns the frames held back."""
        lengths = [self.pushed if e is None else e for e in self.lengths]
        _require_device(self._buf, 'the stream state')
        return self._step(None, lengths)

    def _step(self, samples, lengths):
        fe, B = self.fe, self.B
        n = 0 if samples is None else samples.shape[1]
        if lengths != self.lengths:
            self.lengths = lengths
            self._len_dev.copy_(torch.tensor([_NO_END if e is None else e for e in lengths], dtype=torch.int32))
            self._nfr_dev.copy_(torch.tensor([_NO_END if e is None else n_frames(e) for e in lengths],
                                             dtype=torch.int32))
        if self._done:
            self.pushed += n
            return self._empty()
        if n:
            self._buf[:, self._tail:self._tail + n] = samples   # int16 -> float32 is exact
        s0, width = self.pushed - self._tail, self._tail + n
        self.pushed += n
        all_ended = all(e is not None for e in lengths)
        avail = n_frames(self.pushed)
        if all_ended:
            avail = min(avail, max(n_frames(e) for e in lengths))
        S0, S1 = self._static_done, max(avail, self._static_done)
        E0 = self.frames_out
        E1 = max(E0, avail if all_ended else avail - DELTA_CONTEXT)
        f0 = E0 - DELTA_CONTEXT                                  # the statics buffer's first frame
        if S1 > S0:
            fe._static(self._buf, self._len_dev, width, s0, self.pushed, S0, S1, self._st, f0)
        out = self._empty()
        cs = self._cmvn
        if E1 > E0 and cs is None:
            out = torch.empty((B, E1 - E0, N_FEAT), device=fe.device, dtype=torch.float32)
            fe._deltas(self._st, self._nfr_dev, f0, S1, E0, E1, out, E0)
        elif E1 > E0:
            fe._deltas(self._st, self._nfr_dev, f0, S1, E0, E1, cs.history, cs._f0)
            out = cs._normalise(E0, E1, self._nfr_dev)
        self._static_done, self.frames_out = S1, E1
        if all_ended:
            self._done = True
            return out
        # slide: the samples from the next frame's first on, the statics from E1 - 4 on, and
        # the sliding CMVN's history
        keep = self.pushed - FRAME_SHIFT * S1 if S1 else self.pushed
        shift = width - keep
        ops.stream_advance([(self._buf, self._cap, shift, keep),
                            (self._st, self._rows, E1 - E0, min(2 * DELTA_CONTEXT, self._rows - (E1 - E0)))]
                           + ([cs._slide()] if cs is not None else []))
        self._tail = keep
        return out
