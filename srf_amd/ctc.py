"""CTC loss and decoding at the trainer boundary (trainer_sr.py:64-66, :109-112).

``ctc_loss`` keeps tf.nn.ctc_loss's calling convention as the reference uses it
(dense labels, batch-major logits, explicit blank index) and returns the
per-utterance negative log likelihood.  This revision computes it with
the HIP kernel srf_ctc_loss (loss and logit gradient in one launch).
"""
import ctypes

import numpy as np
import torch

from . import ops


def ctc_loss(labels, logits, label_length, logit_length, logits_time_major=False, blank_index=0):
    if logits_time_major:
        logits = logits.transpose(0, 1)
    return ops.ctc_loss(logits.contiguous(), labels, label_length, logit_length, blank_index)


def ctc_loss_and_grad(labels, logits, label_length, logit_length, blank_index, grad_scale):
    """Per-utterance NLL and grad_scale * d(sum nll)/d logits from one launch
    (batch-major logits); the training step's loss head."""
    return ops.ctc_loss_and_grad(logits.contiguous(), labels, label_length, logit_length, blank_index, grad_scale)


def greedy_decode(logits, lengths, blank_index):
    """Best-path decoding: per-frame argmax, merge repeats, drop blanks.
    logits [B, T, C] batch-major; returns a list of label lists."""
    best = torch.argmax(logits, dim=-1).cpu()
    lengths = lengths.cpu()
    out = []
    for b in range(best.shape[0]):
        seq, prev = [], -1
        for k in best[b, :int(lengths[b])].tolist():
            if k != prev and k != blank_index:
                seq.append(k)
            prev = k
        out.append(seq)
    return out


def greedy_decode_device(logits, n_valid, blank_index, prev):
    """Incremental best-path decoding on the device (srf_ctc_greedy_n): the labels that
    the first n_valid[b] frames of this chunk of logits [B, n, C] add to stream b's
    hypothesis.  prev [B] int32 carries the last frame's arg-max from chunk to chunk
    (-1 at a stream's start) and is updated in place, so a label repeated across a chunk
    edge is merged as greedy_decode merges it.  Returns device tensors (labels [B, n]
    int32, each stream's compacted to the front, and count [B] int32): the logits are
    not copied to the host."""
    n_valid = n_valid.to(device=logits.device, dtype=torch.int32).contiguous()
    return ops.ctc_greedy_chunk(logits.contiguous(), n_valid, blank_index, prev)


def greedy_decode_frames_device(logits, n_valid, blank_index, prev, frame0=0):
    """greedy_decode_device with the time of every label (srf_ctc_greedy_frames_n):
    returns (labels [B, n], frames [B, n], count [B]) int32 on the device, frames[b, i] =
    frame0 + the chunk frame at which labels[b, i] was emitted, i.e. the first frame of
    its arg-max run; a run that continues across a chunk edge belongs to the earlier
    chunk.  labels, count and prev are those of greedy_decode_device."""
    n_valid = n_valid.to(device=logits.device, dtype=torch.int32).contiguous()
    return ops.ctc_greedy_frames_chunk(logits.contiguous(), n_valid, blank_index, prev, frame0)


class Alignment:
    """Result of ``forced_align``, on the device: ``states`` [B, T] int32 (the extended-
    label state per frame: even = blank, 2k + 1 = label k; -1 past the utterance's end and
    for an infeasible utterance), ``token_start`` / ``token_end`` [B, Lmax] int32 (first
    frame of label k's run and one past its last; -1 where there is no label),
    ``token_logp`` [B, Lmax] (sum of the log-probabilities over the run) and ``score`` [B]
    (the path's log-probability, -inf for an infeasible utterance).  ``classes`` is the
    class per frame (-1 where ``states`` is -1); ``spans()`` the host view."""

    def __init__(self, labels, label_lengths, blank_index, states, token_start, token_end, token_logp, score):
        self.labels, self.label_lengths, self.blank_index = labels, label_lengths, int(blank_index)
        self.states, self.token_start, self.token_end = states, token_start, token_end
        self.token_logp, self.score = token_logp, score
        self._classes = self._spans = None

    @property
    def classes(self):
        if self._classes is None:
            st = self.states.to(torch.int64)
            cls = torch.full_like(st, self.blank_index)
            if self.labels.shape[1] > 0:
                lab = torch.gather(self.labels.to(torch.int64), 1, (st.clamp(min=1) - 1) // 2)
                cls = torch.where(st % 2 == 1, lab, cls)
            self._classes = torch.where(st < 0, st, cls).to(torch.int32)
        return self._classes

    def spans(self):
        """Per utterance a list of (label, start, end): label k sits at frames [start,
        end).  Empty for an infeasible utterance.  One copy to the host, kept."""
        if self._spans is None:
            Lmax = self.labels.shape[1]
            packed = torch.cat([self.labels.to(torch.int32), self.token_start, self.token_end,
                                self.label_lengths.to(torch.int32)[:, None]], dim=1).cpu().tolist()
            self._spans = []
            for row in packed:
                n = min(max(row[-1], 0), Lmax)
                lab, st, en = row[:Lmax], row[Lmax:2 * Lmax], row[2 * Lmax:3 * Lmax]
                self._spans.append([(lab[k], st[k], en[k]) for k in range(n) if st[k] >= 0])
        return [list(s) for s in self._spans]

    def words(self, separator, fold=None):
        """The words of the aligned labels at the label ``separator`` with their frames
        (srf_word_split; ``scoring.split_words`` with this alignment): a ``scoring.Words``
        whose ``spans()`` are (labels tuple, start_frame, end_frame) per word."""
        from . import scoring
        return scoring.split_words(self.labels, self.label_lengths, separator, fold=fold, alignment=self)


def forced_align(logits, logit_lengths, labels, label_lengths=None, blank_index=0):
    """CTC forced alignment on the device (srf_ctc_align): the most probable frame-level
    path of each utterance's labels through logits [B, T, C].  ``labels``: a tensor
    [B, Lmax] with ``label_lengths`` [B], or a list of B label lists.  Returns an
    ``Alignment``; the logits are not copied to the host."""
    if not torch.is_tensor(logits) or logits.dim() != 3 or not logits.is_cuda:
        shape, where = tuple(getattr(logits, 'shape', ())), getattr(logits, 'device', 'the host')
        raise ValueError(f'logits must be a device tensor [B, T, C], got {shape} on {where}')
    B, T, C = logits.shape
    if B < 1 or T < 1 or C < 2:
        raise ValueError(f'logits [B, T, C] need B >= 1, T >= 1 and C >= 2, got {tuple(logits.shape)}')
    if not 0 <= int(blank_index) < C:
        raise ValueError(f'blank index {blank_index} outside [0, {C})')
    dev = logits.device
    if torch.is_tensor(labels):
        if labels.dim() != 2 or labels.shape[0] != B or label_lengths is None:
            raise ValueError(f'a label tensor must be [{B}, Lmax] and come with label_lengths')
        lab = labels.to(device=dev, dtype=torch.int32).contiguous()
        lab_len = torch.as_tensor(label_lengths).to(device=dev, dtype=torch.int32).contiguous()
    else:
        if len(labels) != B or label_lengths is not None:
            raise ValueError(f'a label list must hold {B} label lists and come without label_lengths')
        Lmax = max([len(l) for l in labels] + [0])
        rows = [list(l) + [0] * (Lmax - len(l)) for l in labels]
        lab = torch.tensor(rows, dtype=torch.int32).reshape(B, Lmax).to(dev)
        lab_len = torch.tensor([len(l) for l in labels], dtype=torch.int32, device=dev)
    if tuple(lab_len.shape) != (B,):
        raise ValueError(f'label_lengths must have shape ({B},), got {tuple(lab_len.shape)}')
    lens = torch.as_tensor(logit_lengths).to(device=dev, dtype=torch.int32).contiguous()
    if tuple(lens.shape) != (B,):
        raise ValueError(f'logit_lengths must have shape ({B},), got {tuple(lens.shape)}')
    out = ops.ctc_align(logits.detach().float().contiguous(), lab, lab_len, lens, int(blank_index))
    return Alignment(lab, lab_len, blank_index, *out)


BEAM_MAX_WIDTH = 128     # SRF_CTC_BEAM_MAX_WIDTH
BEAM_MAX_CLASSES = 128   # SRF_CTC_BEAM_MAX_CLASSES


def _check_lm(lm, n_classes, blank_index):
    """A fused language model must be made for these classes and this blank."""
    if lm is None:
        return
    if lm.n_classes != int(n_classes):
        raise ValueError(f'the language model has {lm.n_classes} classes, the logits {n_classes}')
    if lm.blank != int(blank_index):
        raise ValueError(f'the language model was fused with blank {lm.blank}, the decoder uses {blank_index}')


def _check_beam_range(n_classes, blank_index, beam_width):
    if not 2 <= int(n_classes) <= BEAM_MAX_CLASSES:
        raise ValueError(f'the device beam search takes 2 .. {BEAM_MAX_CLASSES} classes, got {n_classes}')
    if not 1 <= int(beam_width) <= BEAM_MAX_WIDTH:
        raise ValueError(f'the device beam search takes a beam width of 1 .. {BEAM_MAX_WIDTH}, got {beam_width}')
    if not 0 <= int(blank_index) < int(n_classes):
        raise ValueError(f'blank index {blank_index} outside [0, {n_classes})')


class BeamState:
    """Resumable CTC prefix beam search on the device (srf_ctc_beam_*): the beams of
    ``n_utts`` utterances, kept in one device block between chunks.

    ``push(logits [B, n, C], n_valid [B])`` extends utterance b's beam by the first
    n_valid[b] frames of the chunk (one launch for the whole chunk); ``best()`` returns
    (list of label lists, numpy log probabilities) of the most probable prefixes so far
    and leaves the state as it is; ``reset()`` starts over.  At most ``max_frames``
    frames may be pushed between two resets.  The result is that of beam_search_decode
    on the frames pushed, however they were cut into chunks.

    With ``lm`` (a ``srf_amd.lm.FusedLM`` for the same classes and blank, its tables on
    this device) the language model is fused into the beam (srf_ctc_beam_lm_*, DESIGN.md
    section 17): scores are log p_ctc + the prefix's bonuses, and ``best_device()`` returns
    a fourth tensor, the accumulated bonus.

    ``segmented=True`` is for a stream without an end that an
    endpointer cuts into segments: ``push_cut(logits, n_valid, cut)`` closes, on the device,
    the segment of every utterance whose cut[b] >= 0 and starts its next one, that utterance
    alone.  The bound on the trie is then the caller's: between two cuts of an utterance at
    most ``max_frames`` frames (the endpointer's forced cut sees to that), so the host counter
    no longer adds up -- every push gets a fresh one, ``frames_pushed`` stays 0 -- and one
    push takes at most max_frames frames.  This holds for ``push`` called directly as well:
    nothing on the host or the device refuses the frame that passes the bound.  An
    utterance that gets more than max_frames frames between two cuts writes nothing outside
    its block (the kernel stores no trie node past the capacity), but its result is then
    wrong without a sign of it: ``count`` is the prefix's true length while the labels whose
    nodes were not stored are missing, and their slots hold whatever the output buffer held.
    Without ``segmented`` nothing changes."""

    def __init__(self, n_utts, n_classes, blank_index, beam_width=100, max_frames=4096, device='cuda', lm=None,
                 segmented=False):
        _check_beam_range(n_classes, blank_index, beam_width)
        if int(n_utts) < 1 or int(max_frames) < 1:
            raise ValueError(f'need n_utts >= 1 and max_frames >= 1, got {n_utts} and {max_frames}')
        self.shape = (int(n_utts), int(n_classes), int(beam_width), int(max_frames))
        self.blank = int(blank_index)
        self.device = torch.device(device)
        _check_lm(lm, self.shape[1], self.blank)
        self.lm = lm
        self.segmented = bool(segmented)
        self._pushed = ctypes.c_int(0)
        n_bytes = ops.ctc_beam_state_bytes(*self.shape) if lm is None else ops.ctc_beam_lm_state_bytes(*self.shape)
        self._state = torch.empty(n_bytes, device=self.device, dtype=torch.uint8)
        self.reset()

    @property
    def frames_pushed(self):
        return self._pushed.value

    def reset(self):
        if self.lm is None:
            ops.ctc_beam_reset(self._state, self.shape, self._pushed)
        else:
            ops.ctc_beam_lm_reset(self._state, self.shape, self._pushed)

    def push(self, logits, n_valid):
        n_valid = torch.as_tensor(n_valid).to(device=self.device, dtype=torch.int32).contiguous()
        logits = logits.detach().float().contiguous()
        pushed = ctypes.c_int(0) if self.segmented else self._pushed
        if self.lm is None:
            ops.ctc_beam_push(self._state, self.shape, pushed, logits, n_valid, self.blank)
        else:
            ops.ctc_beam_lm_push(self._state, self.shape, pushed, logits, n_valid, self.blank, self.lm.bonus,
                                 self.lm.next)

    def push_cut(self, logits, n_valid, cut, max_len=None):
        """One chunk with at most one cut per utterance, on the current stream, with no
        host read.  ``cut`` [B] int32: the chunk frame that is the last of utterance b's
        segment (below n_valid[b]), or -1.  The frames up to the cut are pushed, the
        segment is closed (srf_ctc_beam_cut: its hypothesis is kept, the utterance alone
        starts over) and the chunk's frames after the cut open the next segment, from a
        copy shifted left per utterance that the cut kernel writes.  Returns device tensors
        (labels [B, max_len] int32, count [B] int32, score [B] float32, lm_score [B] float32
        or None without a model): the closed segments' best prefixes, count = -1 for an
        utterance without a cut.  ``max_len`` bounds the label rows (labels beyond it are
        dropped, count stays the true length); None takes max_frames."""
        if not self.segmented:
            raise ValueError('push_cut needs a segmented state: build it with segmented=True')
        dev = self.device
        n_valid = torch.as_tensor(n_valid).to(device=dev, dtype=torch.int32).contiguous()
        cut = torch.as_tensor(cut).to(device=dev, dtype=torch.int32).contiguous()
        if tuple(cut.shape) != (self.shape[0],):
            raise ValueError(f'cut must have shape ({self.shape[0]},), got {tuple(cut.shape)}')
        logits = logits.detach().float().contiguous()
        max_len = self.shape[3] if max_len is None else int(max_len)
        self.push(logits, torch.where(cut >= 0, torch.minimum(cut + 1, n_valid), n_valid))
        if logits.dim() == 3 and logits.shape[1] == 0:
            return ops.ctc_beam_cut(self._state, self.shape, cut, max_len, lm=self.lm is not None)
        *out, rest, n_rest = ops.ctc_beam_cut(self._state, self.shape, cut, max_len, lm=self.lm is not None,
                                              logits=logits, n_valid=n_valid)
        self.push(rest, n_rest)
        return tuple(out)

    def best_device(self):
        """(labels [B, max_frames] int32, count [B] int32, log_prob [B] float32), on the
        device; with a language model log_prob is the fused score and a fourth tensor,
        lm_score [B] float32, the accumulated bonus."""
        if self.lm is None:
            return ops.ctc_beam_best(self._state, self.shape)
        return ops.ctc_beam_lm_best(self._state, self.shape)

    def best(self):
        labels, count, log_prob = self.best_device()[:3]
        count = count.cpu().tolist()
        labels = labels[:, :max(count + [1])].cpu().tolist()
        return [labels[b][:count[b]] for b in range(self.shape[0])], log_prob.cpu().double().numpy()


    def nbest(self, n, max_len=None):
        """The ``n`` most probable prefixes of every utterance so far, in the beam's rank
        order (srf_ctc_beam_nbest), as an ``NBest`` on the device; the state stays as it
        is.  1 <= n <= beam_width.  ``max_len`` bounds the label rows (a longer prefix
        gets length -1); None takes max_frames, which always suffices."""
        if not 1 <= int(n) <= self.shape[2]:
            raise ValueError(f'n must lie in 1 .. beam_width = {self.shape[2]}, got {n}')
        max_len = self.shape[3] if max_len is None else int(max_len)
        if max_len < 1:
            raise ValueError(f'max_len must be at least 1, got {max_len}')
        if self.lm is None:
            return NBest(*ops.ctc_beam_nbest(self._state, self.shape, int(n), max_len))
        return NBest(*ops.ctc_beam_lm_nbest(self._state, self.shape, int(n), max_len))


class NBest:
    """N-best list of a device beam search, all on the device: ``labels`` [B, N, max_len]
    int32 (the first ``lengths`` entries of a row are defined), ``lengths`` [B, N] int32
    (0 past ``count``; -1 for a prefix longer than max_len), ``log_prob`` [B, N] float32
    (the beam's log(p_b + p_nb), non-increasing along N, -inf past ``count``) and
    ``count`` [B] int32, the hypotheses the beam held (at most N).  ``lists()`` is the
    host view.  From a beam with a fused language model ``log_prob`` is the ranking score,
    log p_ctc + the bonuses, and ``lm_score`` [B, N] float32 the bonuses (0 past
    ``count``); ``lm_score`` is None without a model."""

    def __init__(self, labels, lengths, log_prob, count, lm_score=None):
        self.labels, self.lengths, self.log_prob, self.count = labels, lengths, log_prob, count
        self.lm_score = lm_score

    def lists(self):
        """Per utterance a list of (label list, log probability), ``count`` long.  One
        copy to the host."""
        B, N, Lmax = self.labels.shape
        packed = torch.cat([self.labels.reshape(B, N * Lmax), self.lengths, self.count[:, None]], dim=1).cpu().tolist()
        logp = self.log_prob.cpu().double().tolist()
        out = []
        for row, lp in zip(packed, logp):
            lens, n = row[N * Lmax:N * Lmax + N], row[-1]
            out.append([(row[i * Lmax:i * Lmax + max(lens[i], 0)], lp[i]) for i in range(n)])
        return out


def beam_search_nbest_device(logits, lengths, blank_index, beam_width, n, lm=None):
    """The ``n`` best prefixes of a device beam search over logits [B, T, C] (one reset,
    one push, one N-best call), as an ``NBest`` on the device: nothing is copied to the
    host.  ValueError outside 2 <= C <= 128, 1 <= n <= beam_width <= 128.  ``lm``: a
    ``FusedLM`` to fuse into the beam (``NBest.lm_score`` is then set)."""
    if not torch.is_tensor(logits) or logits.dim() != 3 or not logits.is_cuda:
        shape, where = tuple(getattr(logits, 'shape', ())), getattr(logits, 'device', 'the host')
        raise ValueError(f'logits must be a device tensor [B, T, C], got {shape} on {where}')
    B, T, C = logits.shape
    _check_beam_range(C, blank_index, beam_width)
    if B < 1:
        raise ValueError('logits hold no utterance')
    state = BeamState(B, C, blank_index, beam_width, max(T, 1), logits.device, lm=lm)
    state.push(logits, torch.as_tensor(lengths))
    return state.nbest(n)


def beam_search_decode_device(logits, lengths, blank_index, beam_width=100, lm=None):
    """beam_search_decode on the device: one reset, one push and one best call of the HIP
    prefix beam search; the labels, counts and scores are copied to the host, the logits
    are not.  logits [B, T, C] on the device, 2 <= C <= 128, 1 <= beam_width <= 128
    (ValueError otherwise); returns (list of label lists, numpy log probabilities).
    ``lm``: a ``FusedLM`` to fuse into the beam; the scores are then the fused ones."""
    if logits.dim() != 3 or not logits.is_cuda:
        raise ValueError(f'logits must be a device tensor [B, T, C], got {tuple(logits.shape)} on {logits.device}')
    B, T, C = logits.shape
    _check_beam_range(C, blank_index, beam_width)
    if B < 1:
        raise ValueError('logits hold no utterance')
    state = BeamState(B, C, blank_index, beam_width, max(T, 1), logits.device, lm=lm)
    state.push(logits, torch.as_tensor(lengths))
    return state.best()


def beam_search_decode(logits, lengths, blank_index, beam_width=100, lm=None, with_lm_score=False):
    """tf.nn.ctc_beam_search_decoder(time-major logits, lengths, beam_width,
    top_paths=1) as process_test_step calls it (trainer_sr.py:109-112), on the host
    prefix beam search of libsrf_data.so.  logits [B, T, C] batch-major (device or
    host); returns (list of label lists, numpy log probabilities).  With ``lm`` (a
    ``FusedLM``) the search is srf_ctc_beam_search_lm, which defines the fused result, and
    the scores are the fused ones; with_lm_score=True then appends the best prefixes'
    accumulated bonuses (numpy) to the result."""
    from . import load_speech_data as lsd
    if with_lm_score and lm is None:
        raise ValueError('with_lm_score comes with lm')
    L = lsd.lib()
    x = np.ascontiguousarray(logits.detach().float().cpu().numpy())
    lens = [int(v) for v in torch.as_tensor(lengths).cpu().tolist()]
    B, T, C = x.shape
    _check_lm(lm, C, blank_index)
    out, logp, lm_score = [], np.zeros(B, np.float64), np.zeros(B, np.float64)
    buf = np.zeros(max(T, 1), np.int32)
    n = ctypes.c_int()
    lp, lms = ctypes.c_float(), ctypes.c_float()
    for b in range(B):
        t = max(0, min(lens[b], T))
        row = x[b]
        if lm is None:
            rc = L.srf_ctc_beam_search(row.ctypes.data, t, C, int(blank_index), int(beam_width), buf.ctypes.data,
                                       ctypes.byref(n), ctypes.byref(lp))
        else:
            rc = L.srf_ctc_beam_search_lm(row.ctypes.data, t, C, int(blank_index), int(beam_width),
                                          lm.bonus_host.ctypes.data, lm.next_host.ctypes.data, lm.n_states,
                                          buf.ctypes.data, ctypes.byref(n), ctypes.byref(lp), ctypes.byref(lms))
        if rc != 0:
            raise ValueError(f'srf_ctc_beam_search: bad argument (T={t}, C={C}, blank={blank_index}, beam={beam_width})')
        out.append(buf[:n.value].tolist())
        logp[b] = lp.value
        lm_score[b] = lms.value
    if with_lm_score:
        return out, logp, lm_score
    return out, logp
