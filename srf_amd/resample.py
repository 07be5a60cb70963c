"""Device resampler: audio at any rate to 16 kHz (or another rate), offline and in chunks.

Kaldi's ``LinearResample`` as ``ResampleWaveform`` configures it -- what
``compute-fbank-feats --sample-frequency=16000`` applies to input at another rate -- as one
HIP kernel (``csrc/resample.hip``): ``Resampler`` offline,
``SpeedPerturb`` for the 3-way speed perturbation of the training side, ``ResampleStream``
in chunks.  Samples are int16 or float32; the output is float32 in the input's scale, not
rounded, and stays on the device: ``fe(*rs(x, n))`` is the whole front end.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib, ops
from .fbank import _require_device, _samples_arg
from .streaming import check_ended

RATE_MIN, RATE_MAX, MAX_RATES = 4000, 192000, 8   # SRF_RESAMPLE_MAX_RATES
_HEADER, _HEADER_FLOATS = 8, 8 + 8 * MAX_RATES    # SRF_RESAMPLE_HEADER
_NO_END = 1 << 30                                 # length of a stream whose end is not known yet
_MAX_OUT = 2 ** 31 - 2049                         # srf_resample's largest output index


def _check_rates(rates_in, rate_out):
    for r in list(rates_in) + [rate_out]:
        if isinstance(r, bool) or not isinstance(r, (int, np.integer)) or not RATE_MIN <= int(r) <= RATE_MAX:
            raise ValueError(f'a rate is an integer in [{RATE_MIN}, {RATE_MAX}] Hz, got {r!r}')
    if not 1 <= len(rates_in) <= MAX_RATES:
        raise ValueError(f'a bank holds 1 .. {MAX_RATES} input rates, got {len(rates_in)}')


def _int_array(rates):
    return (ctypes.c_int * len(rates))(*[int(r) for r in rates])


def n_out(n, rate_in, rate_out=16000):
    """Output samples of ``n`` input samples: ceil(n * ou / iu) (every output whose time lies
    before the input's end, Kaldi's count with flush).  An int, a sequence or a tensor."""
    _check_rates([rate_in], rate_out)
    g = math.gcd(int(rate_in), int(rate_out))
    iu, ou = int(rate_in) // g, int(rate_out) // g
    if isinstance(n, torch.Tensor):
        return (n.to(torch.int64) * ou + (iu - 1)) // iu
    if isinstance(n, (list, tuple, np.ndarray)):
        return [(int(v) * ou + iu - 1) // iu for v in n]
    return (int(n) * ou + iu - 1) // iu


def tables(rates_in, rate_out=16000):
    """The kernel's table block as srf_resample_tables fills it on the host in double:
    ``(flat float32 numpy, [dict(iu, ou, taps, first [ou] int64, w [ou, taps] float32)])``,
    one dict per input rate.  ValueError for what the library refuses."""
    rates_in = [rates_in] if np.isscalar(rates_in) else list(rates_in)
    _check_rates(rates_in, rate_out)
    L, arr = _lib.lib(), _int_array(rates_in)
    n = L.srf_resample_table_floats(arr, len(rates_in), int(rate_out))
    if n == 0:
        raise ValueError(L.srf_last_error().decode(errors='replace'))
    flat = np.empty(n, dtype=np.float32)
    _lib.check(L.srf_resample_tables(arr, len(rates_in), int(rate_out), flat.ctypes.data_as(ctypes.c_void_p), n),
               'srf_resample_tables')
    per_rate = []
    for r in range(len(rates_in)):
        iu, ou, taps, off_first, off_w = (int(v) for v in flat[_HEADER + 8 * r:_HEADER + 8 * r + 5])
        per_rate.append({'iu': iu, 'ou': ou, 'taps': taps, 'first': flat[off_first:off_first + ou].astype(np.int64),
                         'w': flat[off_w:off_w + ou * taps].reshape(ou, taps).copy()})
    return flat, per_rate


def stream_final(pushed, first, taps, iu):
    """Outputs that are final after ``pushed`` input samples: output o = u * ou + p is final
    once its last padded tap has arrived, first[p] + u * iu + taps - 1 <= pushed - 1.  Per
    phase that is (pushed - taps - first[p]) // iu + 1 units where non-negative; the first tap
    grows with o, so the final outputs are a prefix and the sum over the phases is their
    count.  Pure host arithmetic; monotone in ``pushed``."""
    room = int(pushed) - int(taps) - np.asarray(first, dtype=np.int64)
    return int(np.where(room >= 0, room // int(iu) + 1, 0).sum())


def stream_tail(pushed, n_final, first, iu):
    """Input samples a stream keeps once outputs [0, n_final) are out: those from the first
    tap of output n_final on, at most taps - 1 of them when n_final = stream_final(pushed)."""
    ou = len(first)
    lo = int(first[n_final % ou]) + (n_final // ou) * int(iu)
    return int(pushed) - max(lo, 0)


def stream_hold(first, taps, iu):
    """Most outputs a stream holds back: an output o with o * iu / ou < pushed (it counts in
    n_out(pushed)) waits while first[p] + u * iu + taps - 1 >= pushed; with first[p] + u * iu =
    o * iu / ou + delta_p those o span less than taps - 1 + max delta_p input samples, ou / iu
    outputs each."""
    first = np.asarray(first, dtype=np.int64)
    ou = len(first)
    num = (int(taps) - 1) * ou + int((first * ou - np.arange(ou, dtype=np.int64) * int(iu)).max())
    return max(0, -((-num) // int(iu)))


class Resampler:
    """``rs(samples [B, N], n_samples [B], choice=None)`` -> ``(out [B, Mmax] float32, n_out [B]
    int32)`` on the device.  ``rate_in`` is an int, or a sequence of up to 8 ints (a bank):
    row b is then resampled from ``rate_in[choice[b]]`` (``choice`` None: entry 0 for every
    row).  Columns past ``n_out[b]`` are zero; ``Mmax`` is the count for N at the bank's lowest
    input rate.  An entry equal to ``rate_out`` is the exact copy, int16 -> float32."""

    def __init__(self, rate_in, rate_out=16000, device='cuda'):
        self.rates_in = [rate_in] if np.isscalar(rate_in) else list(rate_in)
        _check_rates(self.rates_in, rate_out)
        self.rates_in, self.rate_out = [int(r) for r in self.rates_in], int(rate_out)
        self.device = torch.device(device)
        flat, self.filters = tables(self.rates_in, self.rate_out)
        self.tables = torch.from_numpy(flat).to(self.device)
        self._rates_c = _int_array(self.rates_in)

    def n_out(self, n, choice=0):
        """Output samples of ``n`` (an int, a list or a tensor) input samples at bank entry ``choice``."""
        return n_out(n, self.rates_in[self._entry(choice)], self.rate_out)

    def _entry(self, c):
        if not 0 <= int(c) < len(self.rates_in):
            raise ValueError(f'choice {c} outside the bank of {len(self.rates_in)} rates')
        return int(c)

    # the launch, on buffers with an origin (the streaming path calls it too)
    def _launch(self, samples, n_samples, choice, width, s0, n_limit, o0, o1, out, q0, n_out=None):
        _require_device(samples, 'samples')
        B, stride = samples.shape
        _lib.check(_lib.lib().srf_resample(
            ops._ptr(samples), int(samples.dtype == torch.int16), ops._ptr(n_samples),
            None if choice is None else ops._ptr(choice), ops._ptr(self.tables), self._rates_c, len(self.rates_in),
            self.rate_out, B, stride, width, s0, n_limit, o0, o1, ops._ptr(out), out.shape[1], q0,
            None if n_out is None else ops._ptr(n_out), ops._stream()), 'srf_resample')

    def _choice(self, choice, B):
        """A call's ``choice`` as a device int32 [B] (None stays None), checked against the bank."""
        if choice is None:
            return None
        host = [int(c) for c in (choice.tolist() if hasattr(choice, 'tolist') else choice)]
        if len(host) != B:
            raise ValueError(f'choice has {len(host)} entries for {B} rows')
        for c in host:
            self._entry(c)
        return torch.tensor(host, dtype=torch.int32).to(self.device)

    def __call__(self, samples, n_samples, choice=None):
        if not isinstance(samples, torch.Tensor):
            raise ValueError('samples must be a device tensor [B, N]')
        _require_device(samples, 'samples')
        samples = _samples_arg(samples, self.device, 'samples')
        B, N = samples.shape
        n = torch.as_tensor(n_samples).to(self.device).reshape(-1)
        if n.shape[0] != B:
            raise ValueError(f'n_samples has {n.shape[0]} entries for {B} rows')
        n = ops._i32(n)   # the launch clamps a length to [0, N]
        choice_dev = self._choice(choice, B)
        M = n_out(N, min(self.rates_in), self.rate_out)
        if M > _MAX_OUT:
            raise ValueError(f'{N} samples give {M} outputs, more than one call takes ({_MAX_OUT})')
        out = torch.empty((B, M), device=self.device, dtype=torch.float32)
        counts = torch.zeros(B, device=self.device, dtype=torch.int32) if M == 0 else \
            torch.empty(B, device=self.device, dtype=torch.int32)
        if M:
            self._launch(samples, n, choice_dev, N, 0, N, 0, M, out, 0, counts)
        return out, counts


class SpeedPerturb:
    """Speed perturbation (the standard 3-way WSJ augmentation): a ``Resampler`` bank of
    ``round(rate * f)`` -> ``rate`` for each factor -- speed 0.9 of 16 kHz audio is 14 400 ->
    16 000 Hz, longer and lower.  ``sp(samples [B, N], n_samples [B], step)`` draws each row's
    factor from a generator keyed by ``(seed, step)`` and returns ``(out, n_out, choice)``,
    ``choice`` [B] int64 (host) the factor index of every row.  Factor 1.0 rows are bit
    copies."""

    def __init__(self, factors=(0.9, 1.0, 1.1), rate=16000, seed=0, device='cuda'):
        self.factors = [float(f) for f in factors]
        if not self.factors or any(not (f > 0.0 and f < float('inf')) for f in self.factors):
            raise ValueError(f'factors must be finite and > 0, got {factors}')
        self.rate, self.seed = int(rate), int(seed)
        self.resampler = Resampler([int(round(self.rate * f)) for f in self.factors], self.rate, device)

    def draw(self, B, step):
        """The factor indices of a batch of B rows at ``step``: a pure function of (seed, step, B)."""
        g = torch.Generator().manual_seed((self.seed * 0x9E3779B1 + int(step)) % (2 ** 63))
        return torch.randint(0, len(self.factors), (int(B),), generator=g)

    def __call__(self, samples, n_samples, step):
        if not isinstance(samples, torch.Tensor) or samples.dim() != 2:
            raise ValueError('samples must be a device tensor [B, N]')
        choice = self.draw(samples.shape[0], step)
        out, n = self.resampler(samples, n_samples, choice)
        return out, n, choice


class ResampleStream:
    """``rs`` (a single-rate ``Resampler``) over ``n_streams`` signals that arrive in chunks,
    in lock step, like ``fbank.FbankStream``.

    ``push(samples [B, n], ended=None)`` takes the next n <= ``max_samples`` input samples of
    every stream and returns the output samples [B, m] that became final, outputs
    ``out_done - m .. out_done - 1`` of every stream; ``ended``: the total input sample count
    of a stream whose end lies in this chunk, else -1.  ``finish()`` ends every stream that
    has not declared an end and returns the rest.  The concatenated output equals ``rs`` on
    the whole signals bit for bit, whatever the chunking.

    An output is final once its last padded tap has arrived (``stream_final``), so an
    unfinished stream holds back at most ``hold`` outputs (``stream_hold``; 13 at the most for
    48, 44.1 and 8 kHz and the speed bank).  Once every stream has ended the output runs to
    the longest stream's ``n_out``; columns past an ended stream's ``n_out`` are zero.

    Device-resident state: the input tail and nothing else, at most taps - 1 samples, slid
    to the front of its buffer after a chunk (srf_stream_advance_n)."""

    def __init__(self, rs, n_streams, max_samples):
        if len(rs.rates_in) != 1:
            raise ValueError(f'a stream resamples from one rate, the resampler holds {len(rs.rates_in)}')
        if int(n_streams) < 1 or int(max_samples) < 1:
            raise ValueError(f'n_streams and max_samples must be >= 1, got {n_streams} and {max_samples}')
        self.rs, self.B, self.max_samples = rs, int(n_streams), int(max_samples)
        f = rs.filters[0]
        self._first, self._taps, self._iu, self._ou = f['first'], f['taps'], f['iu'], f['ou']
        self.hold = stream_hold(self._first, self._taps, self._iu)
        self._cap = self._taps - 1 + self.max_samples
        self._buf = torch.zeros((self.B, self._cap), device=rs.device, dtype=torch.float32)
        self._len_dev = torch.full((self.B,), _NO_END, device=rs.device, dtype=torch.int32)
        self.reset()

    def reset(self):
        """Every stream back at its start."""
        self._len_dev.fill_(_NO_END)
        self.lengths = [None] * self.B   # declared input sample counts
        self.pushed = 0                  # input samples taken per stream
        self.out_done = 0                # output samples returned per stream
        self._tail = 0                   # samples held: the global samples pushed - _tail .. pushed - 1
        self._done = False               # every stream has ended and its outputs are out

    def _empty(self):
        return torch.empty((self.B, 0), device=self.rs.device, dtype=torch.float32)

    def push(self, samples, ended=None):
        if not isinstance(samples, torch.Tensor) or samples.dim() != 2 or samples.shape[0] != self.B:
            raise ValueError(f'samples must be [{self.B}, n], got {tuple(getattr(samples, "shape", ()))}')
        n = samples.shape[1]
        if n > self.max_samples:
            raise ValueError(f'a chunk holds at most max_samples = {self.max_samples} samples, got {n}')
        if self.pushed + n >= _NO_END:
            raise ValueError(f'a stream holds fewer than {_NO_END} samples')
        lengths = check_ended(self.lengths, ended, self.pushed, n, unit='samples')
        _require_device(samples, 'samples')
        samples = _samples_arg(samples, self.rs.device, 'samples')
        return self._step(samples, lengths)

    def finish(self):
        """Ends every stream that has not declared an end; returns the outputs held back."""
        return self._step(None, [self.pushed if e is None else e for e in self.lengths])

    def _step(self, samples, lengths):
        rs = self.rs
        n = 0 if samples is None else samples.shape[1]
        if lengths != self.lengths:
            self.lengths = lengths
            self._len_dev.copy_(torch.tensor([_NO_END if e is None else e for e in lengths], dtype=torch.int32))
        if self._done:
            self.pushed += n
            return self._empty()
        if n:
            self._buf[:, self._tail:self._tail + n] = samples   # int16 -> float32 is exact
        s0, width = self.pushed - self._tail, self._tail + n
        self.pushed += n
        all_ended = all(e is not None for e in lengths)
        if all_ended:
            E1 = max(rs.n_out(e) for e in lengths)
        else:
            E1 = stream_final(self.pushed, self._first, self._taps, self._iu)
        E0, E1 = self.out_done, max(self.out_done, E1)
        out = self._empty()
        if E1 > E0:
            out = torch.empty((self.B, E1 - E0), device=rs.device, dtype=torch.float32)
            rs._launch(self._buf, self._len_dev, None, width, s0, self.pushed, E0, E1, out, E0)
        self.out_done = E1
        if all_ended:
            self._done = True
            return out
        keep = stream_tail(self.pushed, E1, self._first, self._iu)
        ops.stream_advance([(self._buf, self._cap, width - keep, keep)])
        self._tail = keep
        return out
