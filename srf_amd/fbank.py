"""Device front end: 16 kHz waveform to the 123-d filterbank features the model reads.

The reference prepares its input with Kaldi (``egs/script/fbank123.sh``):
``compute-fbank-feats --num-mel-bins=40 --sample-frequency=16000 --use-log-fbank=True
--use-energy=True``, ``add-deltas`` and per-speaker CMVN, which ``save_speech_data.py:163``
applies as ``(feats - mean + 1e-14) / (std + 1e-14)``.  This module is that recipe as HIP
kernels (``csrc/fbank.hip``): ``Fbank`` offline, ``FbankStream`` in
chunks, ``CmvnStats`` for the mean and the deviation.  Samples are in int16 scale, int16
or float32; everything stays on the device.
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
    ``y = (x - mean + 1e-14) / (std + 1e-14)``.

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
        self.mean = self.std = None
        if cmvn is not None:
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
    frames, each slid to the front of its buffer after a chunk (srf_stream_advance_n)."""

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
        self.reset()

    def reset(self):
        """Every stream back at its start."""
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
        if E1 > E0:
            out = torch.empty((B, E1 - E0, N_FEAT), device=fe.device, dtype=torch.float32)
            fe._deltas(self._st, self._nfr_dev, f0, S1, E0, E1, out, E0)
        self._static_done, self.frames_out = S1, E1
        if all_ended:
            self._done = True
            return out
        # slide: the samples from the next frame's first on, and the statics from E1 - 4 on
        keep = self.pushed - FRAME_SHIFT * S1 if S1 else self.pushed
        shift = width - keep
        ops.stream_advance([(self._buf, self._cap, shift, keep),
                            (self._st, self._rows, E1 - E0, min(2 * DELTA_CONTEXT, self._rows - (E1 - E0)))])
        self._tail = keep
        return out
