"""Endpointing on the device: where each stream's utterance ends.

The rule is WeNet's and Kaldi's without the relative-cost term, on the CTC logits alone.
Per stream the state is n (frames in the open segment), sil (trailing silence run), speech
(a flag) and t (frames consumed since the reset); for every consumed frame x, in order:

    lp_blank = log_softmax(x)[blank];  is_sil = lp_blank > log(blank_threshold)
    is_sp    = argmax(x) != blank       (lowest index wins a tie)
    n += 1;  sil = sil + 1 if is_sil else 0;  speech |= is_sp
    reason = 2 if speech and sil >= silence_after_speech
        else 1 if sil >= silence_only
        else 3 if n >= max_segment
        else 0
    if reason: emit (t - n + 1, t, reason);  n = sil = 0;  speech = False

A segment is [start, end], inclusive, in output frames (40 ms each).  The flags are fp32 on
the device (srf_ctc_endpoint_n), everything after them is integer: the cuts are a function of
the stream's frames and depend neither on the chunking nor on the other streams.
"""
import math
from typing import NamedTuple

import torch

from . import ops

REASONS = {0: 'end', 1: 'silence', 2: 'silence_after_speech', 3: 'max_segment'}


class EndpointRules:
    """The rule's options: ``silence_only`` (5 s), ``silence_after_speech`` (1 s) and
    ``max_segment`` (20 s, the forced cut) in output frames of 40 ms, each at least 1, and
    ``blank_threshold`` in (0, 1): a frame is silent when the blank's probability exceeds it."""

    def __init__(self, silence_only=125, silence_after_speech=25, max_segment=500, blank_threshold=0.8):
        for name, v in (('silence_only', silence_only), ('silence_after_speech', silence_after_speech),
                        ('max_segment', max_segment)):
            if isinstance(v, bool) or int(v) != v or int(v) < 1:
                raise ValueError(f'{name} is a count of output frames, at least 1; got {v!r}')
        if not 0.0 < float(blank_threshold) < 1.0:
            raise ValueError(f'blank_threshold must lie strictly between 0 and 1, got {blank_threshold!r}')
        self.silence_only, self.silence_after_speech = int(silence_only), int(silence_after_speech)
        self.max_segment, self.blank_threshold = int(max_segment), float(blank_threshold)

    @property
    def counts(self):
        return self.silence_only, self.silence_after_speech, self.max_segment

    @property
    def log_threshold(self):
        """log(blank_threshold), in double; the device takes it rounded to a float."""
        return math.log(self.blank_threshold)

    def __repr__(self):
        return (f'EndpointRules(silence_only={self.silence_only}, silence_after_speech={self.silence_after_speech}, '
                f'max_segment={self.max_segment}, blank_threshold={self.blank_threshold})')


class Cuts(NamedTuple):
    """What one endpointer call closed, on the device: ``start``, ``end``, ``reason``
    [B, max_cuts] int32 (-1 past a stream's number) and ``n_cuts`` [B] int32, the true
    number even where it exceeds max_cuts."""
    start: torch.Tensor
    end: torch.Tensor
    reason: torch.Tensor
    n_cuts: torch.Tensor

    def lists(self):
        """Per stream a list of (start, end, reason), the cuts stored.  One copy to the host."""
        B, K = self.start.shape
        packed = torch.cat([self.start, self.end, self.reason, self.n_cuts[:, None]], dim=1).cpu().tolist()
        return [[(row[k], row[K + k], row[2 * K + k]) for k in range(min(row[-1], K))] for row in packed]


class Segment(NamedTuple):
    """One closed segment of a stream (``StreamingRouter.segments``): output frames [start,
    end], inclusive; ``reason`` 1 silence, 2 silence after speech, 3 forced at max_segment,
    0 the stream's end (``REASONS``).  ``labels``: the greedy labels emitted in those frames;
    ``beam_labels``, ``beam_score``: the beam search's best prefix of the segment and its
    score, ``lm_score`` its accumulated language-model bonus (None without a beam / model)."""
    start: int
    end: int
    reason: int
    labels: list
    beam_labels: list = None
    beam_score: float = None
    lm_score: float = None


def _check_shape(n_classes, blank):
    if int(n_classes) < 2:
        raise ValueError(f'the endpointer takes at least 2 classes, got {n_classes}')
    if not 0 <= int(blank) < int(n_classes):
        raise ValueError(f'blank index {blank} outside [0, {n_classes})')


class Endpointer:
    """The endpoint state of ``n_streams`` streams on the device, carried from chunk to chunk.

    ``push(logits [B, n, C], n_valid [B], max_cuts=1)`` consumes the first n_valid[b] frames
    of stream b and returns the segments they closed as ``Cuts`` (device tensors; nothing is
    copied to the host); ``reset()`` starts every stream over."""

    def __init__(self, rules, n_streams, n_classes, blank, device='cuda'):
        if not isinstance(rules, EndpointRules):
            raise ValueError(f'rules must be an EndpointRules, got {type(rules).__name__}')
        if int(n_streams) < 1:
            raise ValueError(f'n_streams must be >= 1, got {n_streams}')
        _check_shape(n_classes, blank)
        self.rules, self.B, self.C, self.blank = rules, int(n_streams), int(n_classes), int(blank)
        self.device = torch.device(device)
        self._state = ops.ctc_endpoint_state(self.B, self.device)

    def reset(self):
        ops.ctc_endpoint_reset(self._state, self.B)

    def push(self, logits, n_valid, max_cuts=1):
        if not torch.is_tensor(logits) or logits.dim() != 3 or tuple(logits.shape[::2]) != (self.B, self.C):
            raise ValueError(f'logits must be [{self.B}, n, {self.C}], got {tuple(getattr(logits, "shape", ()))}')
        if int(max_cuts) < 1:
            raise ValueError(f'max_cuts must be at least 1, got {max_cuts}')
        n_valid = torch.as_tensor(n_valid).to(device=self.device, dtype=torch.int32).contiguous()
        r = self.rules
        return Cuts(*ops.ctc_endpoint(logits.detach().float().contiguous(), n_valid, self.blank, r.log_threshold,
                                      r.counts, self._state, int(max_cuts)))


def endpoints(logits, lengths, blank, rules):
    """The offline call: every cut of logits [B, T, C] (device) with ``lengths`` [B] frames
    per utterance, in one launch with max_cuts = T // min(counts) + 1, which no utterance
    can exceed.  Returns ``Cuts`` (start, end, reason, n_cuts)."""
    if not torch.is_tensor(logits) or logits.dim() != 3 or not logits.is_cuda:
        shape, where = tuple(getattr(logits, 'shape', ())), getattr(logits, 'device', 'the host')
        raise ValueError(f'logits must be a device tensor [B, T, C], got {shape} on {where}')
    B, T, C = logits.shape
    if B < 1:
        raise ValueError('logits hold no utterance')
    ep = Endpointer(rules, B, C, blank, logits.device)
    return ep.push(logits, lengths, max_cuts=T // min(rules.counts) + 1)
