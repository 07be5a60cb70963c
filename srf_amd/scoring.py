"""Scoring of hypotheses on the device: the edit alignment of hypotheses against their
references (srf_edit_align) and the label error rate it gives, the phone / character
error rate that the reference's pipeline gets from log2utt.py and sclite after the run.

``edit_align`` returns one alignment (counts and the two position maps); ``ErrorRate`` is
the metric: it adds every batch's counts to device-resident int64 sums in the alignment's
own launch, as trainer_sr.Mean keeps the loss, and reads them once in ``result()``.
``fold_table`` builds the optional label fold (TIMIT's 61 -> 39 phones).

For a character model the words: ``split_words`` cuts label rows at a separator label
(srf_word_split; with a ``ctc.Alignment`` also the word times), ``word_align`` aligns the
words of hypotheses and references (srf_word_align: equal words get equal ids, the ids are
aligned as labels are) and ``WordErrorRate`` is the metric next to ``ErrorRate``.
"""
import operator

import torch
import torch.distributed as dist

from . import ops

COUNT_NAMES = ('distance', 'substitutions', 'deletions', 'insertions', 'reference_labels', 'hypothesis_labels')
MAX_LABELS = 8192   # srf_edit_align's Hmax / Rmax


def fold_table(vocab, mapping, device='cuda'):
    """The fold of ``vocab`` (names by class index) through ``mapping`` ({name: name}): a
    name that is absent from the mapping or mapped to '' is dropped, the folded classes are
    numbered by first appearance in vocab order.  Returns (int32 table [len(vocab)] on
    ``device``, -1 for a dropped class; names of the folded classes)."""
    names, index, table = [], {}, []
    for v in vocab:
        to = mapping.get(v, '')
        if to == '':
            table.append(-1)
            continue
        if to not in index:
            index[to] = len(names)
            names.append(to)
        table.append(index[to])
    return torch.tensor(table, dtype=torch.int32, device=device), names


def _dense(seqs, lens, what, batch=None):
    """(labels [B, max], lengths [B]) from a device tensor with lengths or from a list of
    label lists, checked and not yet moved: ValueError before anything runs on the GPU."""
    if torch.is_tensor(seqs):
        if not seqs.is_cuda or seqs.dim() != 2:
            raise ValueError(f'{what} must be a device tensor [B, max] or a list of label lists, got '
                             f'{tuple(seqs.shape)} on {seqs.device}')
        if lens is None:
            raise ValueError(f'a {what} tensor comes with its lengths')
        B, n = seqs.shape
        if torch.is_tensor(lens) and lens.dim() == 1 and lens.shape[0] == B:
            ln = lens
        else:
            ln = torch.as_tensor(lens)
            if tuple(ln.shape) != (B,):
                raise ValueError(f'{what} lengths must have shape ({B},), got {tuple(ln.shape)}')
        lab = seqs
    else:
        if lens is not None:
            raise ValueError(f'a {what} list comes without lengths')
        rows = [list(s) for s in seqs]
        B, n = len(rows), max([len(r) for r in rows] + [0])
        lab = torch.tensor([r + [0] * (n - len(r)) for r in rows], dtype=torch.int32).reshape(B, n)
        ln = torch.tensor([len(r) for r in rows], dtype=torch.int32)
    if B < 1 or (batch is not None and B != batch):
        raise ValueError(f'{what} holds {B} utterances' + (f', expected {batch}' if batch is not None else ''))
    if n > MAX_LABELS:
        raise ValueError(f'{what} holds up to {n} labels, the device alignment takes {MAX_LABELS}')
    return lab, ln


def _fold_tensor(fold, dev):
    if fold is None:
        return None
    t = torch.as_tensor(fold)
    if t.dim() != 1 or t.is_floating_point():
        raise ValueError(f'the fold must be a 1-d integer table, got {t.dtype} {tuple(t.shape)}')
    return t.to(device=dev, dtype=torch.int32).contiguous()


def _operands(hyp, hyp_len, ref, ref_len, dev):
    h, hl = _dense(hyp, hyp_len, 'hyp')
    r, rl = _dense(ref, ref_len, 'ref', batch=h.shape[0])
    if dev is None:
        dev = next((t.device for t in (h, r) if t.is_cuda), torch.device('cuda'))
    if torch.device(dev).type != 'cuda':
        raise ValueError(f'the edit alignment runs on a HIP device, not on {dev} (no CPU path exists)')
    return tuple(t.detach().to(device=dev, dtype=torch.int32).contiguous() for t in (h, hl, r, rl))


class EditAlignment:
    """Result of ``edit_align``, on the device: ``counts`` [B, 6] int32 (distance,
    substitutions, deletions, insertions, reference labels and hypothesis labels after the
    fold), ``hyp_to_ref`` [B, Hmax] and ``ref_to_hyp`` [B, Rmax] int32 by the positions
    before the fold (the partner's position; -1 inserted / deleted; -2 dropped by the fold
    or past the length).  ``ops()`` is the host view."""

    def __init__(self, hyp, hyp_len, ref, ref_len, fold, counts, hyp_to_ref, ref_to_hyp):
        self.hyp, self.hyp_len, self.ref, self.ref_len, self.fold = hyp, hyp_len, ref, ref_len, fold
        self.counts, self.hyp_to_ref, self.ref_to_hyp = counts, hyp_to_ref, ref_to_hyp
        self._ops = None

    def ops(self):
        """Per utterance the list of (kind, hyp_index, ref_index) along the alignment,
        kind 'cor' | 'sub' | 'del' | 'ins', the indices positions before the fold (-1 for
        the side a deletion or an insertion lacks).  One copy to the host, kept."""
        if self._ops is None:
            Hmax, Rmax = self.hyp.shape[1], self.ref.shape[1]
            packed = torch.cat([self.hyp, self.ref, self.hyp_to_ref, self.ref_to_hyp], dim=1).cpu().tolist()
            fold = None if self.fold is None else self.fold.cpu().tolist()

            def cls(x):
                return x if fold is None else fold[x]
            self._ops = []
            for row in packed:
                h, r = row[:Hmax], row[Hmax:Hmax + Rmax]
                h2r, r2h = row[Hmax + Rmax:2 * Hmax + Rmax], row[2 * Hmax + Rmax:]
                out, i, j = [], 0, 0
                while i < Hmax or j < Rmax:
                    if i < Hmax and h2r[i] == -2:
                        i += 1
                    elif j < Rmax and r2h[j] == -2:
                        j += 1
                    elif i < Hmax and h2r[i] == -1:
                        out.append(('ins', i, -1))
                        i += 1
                    elif j < Rmax and r2h[j] == -1:
                        out.append(('del', -1, j))
                        j += 1
                    else:
                        out.append(('cor' if cls(h[i]) == cls(r[j]) else 'sub', i, j))
                        i += 1
                        j += 1
                self._ops.append(out)
        return [list(o) for o in self._ops]


def edit_align(hyp, hyp_len, ref, ref_len, fold=None):
    """Levenshtein alignment with a backtrace on the device (srf_edit_align): ``hyp`` and
    ``ref`` are device tensors [B, max] with lengths [B], or lists of B label lists with
    None as lengths.  ``fold``: an int32 table (``fold_table``), labels mapped to a
    negative entry or outside the table are dropped before the alignment.  Ties: the
    diagonal, then the deletion, then the insertion.  Returns an ``EditAlignment``."""
    h, hl, r, rl = _operands(hyp, hyp_len, ref, ref_len, None)
    f = _fold_tensor(fold, h.device)
    counts, h2r, r2h = ops.edit_align(h, hl, r, rl, f)
    return EditAlignment(h, hl, r, rl, f, counts, h2r, r2h)


class ErrorRate:
    """The label error rate (substitutions + deletions + insertions) / reference labels of
    everything passed to ``update_state``, kept on the device: ``state()`` is the int64
    sums [8] (the six counts of COUNT_NAMES, utterances, utterances with an error) and,
    with ``n_classes`` = K, the confusion matrix [K + 1, K + 1] (row: reference class,
    column: hypothesis class, after the fold; column K deletions, row K insertions).
    ``update_state`` is one launch and nothing on the host; ``result()`` reads once."""

    def __init__(self, n_classes=None, fold=None, device='cuda', name=''):
        if n_classes is not None and int(n_classes) < 1:
            raise ValueError(f'n_classes must be at least 1, got {n_classes}')
        self.name, self.device = name, torch.device(device)
        self.n_classes = None if n_classes is None else int(n_classes)
        self.fold = _fold_tensor(fold, self.device)
        K = self.n_classes
        self._totals = torch.zeros(8, dtype=torch.int64, device=self.device)
        self._confusion = None if K is None else torch.zeros((K + 1, K + 1), dtype=torch.int64, device=self.device)

    def reset_states(self):
        self._totals.zero_()
        if self._confusion is not None:
            self._confusion.zero_()

    def update_state(self, hyp, hyp_len, ref, ref_len):
        h, hl, r, rl = _operands(hyp, hyp_len, ref, ref_len, self.device)
        ops.edit_align(h, hl, r, rl, self.fold, maps=False, totals=self._totals, confusion=self._confusion)

    def state(self):
        return self._totals, self._confusion

    def reduce(self):
        """SUM all-reduce of the state over the process group, in place; every rank calls
        it.  Nothing happens without a group or at world size 1."""
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            dist.all_reduce(self._totals, op=dist.ReduceOp.SUM)
            if self._confusion is not None:
                dist.all_reduce(self._confusion, op=dist.ReduceOp.SUM)

    def result(self):
        t = self._totals.cpu().tolist()
        out = {k: t[q] for q, k in enumerate(COUNT_NAMES) if k != 'distance'}
        out['utterances'] = t[6]
        out['error_rate'] = (t[1] + t[2] + t[3]) / t[4] if t[4] else 0.0
        out['utterance_error_rate'] = t[7] / t[6] if t[6] else 0.0
        return out

    def confusion(self):
        if self._confusion is None:
            raise ValueError('the confusion matrix needs n_classes')
        return self._confusion


def _host_words(labels, fold, start, end, count):
    """Per utterance the tuples of kept classes of its words, from one packed copy."""
    Lmax, W = labels.shape[1], start.shape[1]
    packed = torch.cat([labels, start, end, count[:, None]], dim=1).cpu().tolist()
    table = None if fold is None else fold.cpu().tolist()
    out = []
    for row in packed:
        lab, st, en, n_words = row[:Lmax], row[Lmax:Lmax + W], row[Lmax + W:Lmax + 2 * W], row[-1]
        words = []
        for k in range(n_words):
            seg = lab[st[k]:en[k]]
            if table is not None:
                seg = [table[x] for x in seg if 0 <= x < len(table) and table[x] >= 0]
            words.append(tuple(seg))
        out.append(words)
    return out


class Words:
    """Result of ``split_words``, on the device: ``start`` / ``end`` [B, (Lmax + 1) // 2]
    int32 (the position before the fold of each word's first kept label and one past that
    of its last; -1 past ``count`` [B]).  With an alignment also ``frame_start`` /
    ``frame_end`` int32 (the first output frame of the word's first label and one past the
    last frame of its last label) and ``logp`` float32 (the sum of the labels' log-
    probabilities), -1 / -1 / 0 for an infeasible utterance; None without one.  ``lists()``,
    ``text()`` and ``spans()`` are the host views."""

    def __init__(self, labels, lengths, separator, fold, start, end, count, frame_start=None, frame_end=None,
                 logp=None):
        self.labels, self.lengths, self.separator, self.fold = labels, lengths, int(separator), fold
        self.start, self.end, self.count = start, end, count
        self.frame_start, self.frame_end, self.logp = frame_start, frame_end, logp
        self._lists = self._spans = None

    def lists(self):
        """Per utterance the list of its words, each the tuple of its kept classes (after
        the fold).  One copy to the host, kept."""
        if self._lists is None:
            self._lists = _host_words(self.labels, self.fold, self.start, self.end, self.count)
        return [list(w) for w in self._lists]

    def text(self, vocab):
        """Per utterance its words spelled with ``vocab`` (names by class after the fold)
        and joined by one blank."""
        return [' '.join(''.join(vocab[c] for c in w) for w in words) for words in self.lists()]

    def spans(self):
        """Per utterance a list of (labels tuple, start_frame, end_frame), one per word;
        empty for an infeasible utterance.  Needs an alignment.  One copy to the host, kept."""
        if self.frame_start is None:
            raise ValueError('word spans need the frames of an alignment (split_words(..., alignment=))')
        if self._spans is None:
            W = self.start.shape[1]
            packed = torch.cat([self.frame_start, self.frame_end], dim=1).cpu().tolist()
            self._spans = [[(w, row[k], row[W + k]) for k, w in enumerate(words) if row[k] >= 0]
                           for row, words in zip(packed, self.lists())]
        return [list(s) for s in self._spans]


def _separator(separator):
    try:
        if isinstance(separator, bool):
            raise TypeError
        return operator.index(separator)
    except TypeError:
        raise ValueError(f'the separator is a label index (int), got {separator!r}') from None


def split_words(labels, lengths, separator, fold=None, alignment=None):
    """The words of each label row on the device (srf_word_split): ``labels`` a device
    tensor [B, Lmax] with ``lengths`` [B], or a list of B label lists with None.  A word is
    a maximal run of kept labels between ``separator`` labels; with ``fold`` (an int32
    table, ``fold_table``) the labels it drops neither split a word nor add to it.
    ``alignment``: the ``ctc.Alignment`` of the same labels, for the word times.  Returns
    ``Words``."""
    sep = _separator(separator)
    lab, ln = _dense(labels, lengths, 'labels')
    dev = lab.device if lab.is_cuda else (torch.device('cuda') if alignment is None else alignment.token_start.device)
    if torch.device(dev).type != 'cuda':
        raise ValueError(f'the word split runs on a HIP device, not on {dev} (no CPU path exists)')
    lab, ln = (t.detach().to(device=dev, dtype=torch.int32).contiguous() for t in (lab, ln))
    f = _fold_tensor(fold, dev)
    tok = None
    if alignment is not None:
        tok = (alignment.token_start, alignment.token_end, alignment.token_logp)
        if tuple(tok[0].shape) != tuple(lab.shape):
            raise ValueError(f'the alignment holds labels {tuple(tok[0].shape)}, the split {tuple(lab.shape)}')
    return Words(lab, ln, sep, f, *ops.word_split(lab, ln, sep, f, tok))


class WordAlignment:
    """Result of ``word_align``, on the device: ``counts`` [B, 6] int32 (word distance,
    substituted, deleted and inserted words, reference words, hypothesis words); per side
    ``*_word_start`` / ``*_word_end`` (label positions before the fold) and ``*_word_id``
    (the index, in the list of the utterance's reference words followed by its hypothesis
    words, of the first word equal to this one), -1 past the word count;
    ``hyp_to_ref`` [B, (Hmax + 1) // 2] and ``ref_to_hyp`` [B, (Rmax + 1) // 2] over word
    indices (the partner word; -1 inserted / deleted; -2 past the count)."""

    def __init__(self, hyp, hyp_len, ref, ref_len, separator, fold, counts, hyp_words, ref_words, hyp_to_ref,
                 ref_to_hyp):
        self.hyp, self.hyp_len, self.ref, self.ref_len = hyp, hyp_len, ref, ref_len
        self.separator, self.fold, self.counts = separator, fold, counts
        self.hyp_word_start, self.hyp_word_end, self.hyp_word_id = hyp_words
        self.ref_word_start, self.ref_word_end, self.ref_word_id = ref_words
        self.hyp_to_ref, self.ref_to_hyp = hyp_to_ref, ref_to_hyp
        self._ops = None

    def ops(self):
        """Per utterance the list of (kind, hyp_word, ref_word) along the alignment, kind
        'cor' | 'sub' | 'del' | 'ins', the indices word indices (-1 for the side a deletion
        or an insertion lacks).  One copy to the host, kept."""
        if self._ops is None:
            WH, WR = self.hyp_word_id.shape[1], self.ref_word_id.shape[1]
            packed = torch.cat([self.hyp_word_id, self.ref_word_id, self.hyp_to_ref, self.ref_to_hyp],
                               dim=1).cpu().tolist()
            self._ops = []
            for row in packed:
                hid, rid = row[:WH], row[WH:WH + WR]
                h2r, r2h = row[WH + WR:2 * WH + WR], row[2 * WH + WR:]
                out, i, j = [], 0, 0
                while (i < WH and h2r[i] != -2) or (j < WR and r2h[j] != -2):
                    if i < WH and h2r[i] == -1:
                        out.append(('ins', i, -1))
                        i += 1
                    elif j < WR and r2h[j] == -1:
                        out.append(('del', -1, j))
                        j += 1
                    else:
                        out.append(('cor' if hid[i] == rid[j] else 'sub', i, j))
                        i += 1
                        j += 1
                self._ops.append(out)
        return [list(o) for o in self._ops]


def word_align(hyp, hyp_len, ref, ref_len, separator, fold=None):
    """Word-level Levenshtein alignment on the device (srf_word_align): both sides are cut
    into words at ``separator`` (``split_words``), equal words get equal ids (the labels
    decide, exactly), and the id rows are aligned as ``edit_align`` aligns labels, with its
    tie rule.  Inputs as ``edit_align``'s.  Returns a ``WordAlignment``."""
    sep = _separator(separator)
    h, hl, r, rl = _operands(hyp, hyp_len, ref, ref_len, None)
    f = _fold_tensor(fold, h.device)
    counts, hw, rw, h2r, r2h = ops.word_align(h, hl, r, rl, sep, f)
    return WordAlignment(h, hl, r, rl, sep, f, counts, hw, rw, h2r, r2h)


class WordErrorRate:
    """The word error rate (substituted + deleted + inserted words) / reference words of
    everything passed to ``update_state``, kept on the device as ``ErrorRate`` keeps the
    label error rate: ``state()`` is the int64 sums [8] (the six counts of COUNT_NAMES in
    words, utterances, utterances with a word error).  ``separator`` is the label that
    parts words (for the WSJ character vocabulary the index of <SPACE>), ``fold`` an
    optional ``fold_table`` (dropping <PADDING_MASK>).  ``update_state`` is two launches
    and nothing on the host; ``result()`` reads once."""

    def __init__(self, separator, fold=None, device='cuda', name=''):
        self.separator = _separator(separator)
        self.name, self.device = name, torch.device(device)
        self.fold = _fold_tensor(fold, self.device)
        self._totals = torch.zeros(8, dtype=torch.int64, device=self.device)

    def reset_states(self):
        self._totals.zero_()

    def update_state(self, hyp, hyp_len, ref, ref_len):
        h, hl, r, rl = _operands(hyp, hyp_len, ref, ref_len, self.device)
        ops.word_align(h, hl, r, rl, self.separator, self.fold, words=False, maps=False, totals=self._totals)

    def state(self):
        return self._totals

    def reduce(self):
        """SUM all-reduce of the state over the process group, in place; every rank calls
        it.  Nothing happens without a group or at world size 1."""
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            dist.all_reduce(self._totals, op=dist.ReduceOp.SUM)

    def result(self):
        t = self._totals.cpu().tolist()
        return {'substitutions': t[1], 'deletions': t[2], 'insertions': t[3], 'reference_words': t[4],
                'hypothesis_words': t[5], 'utterances': t[6],
                'word_error_rate': (t[1] + t[2] + t[3]) / t[4] if t[4] else 0.0,
                'sentence_error_rate': t[7] / t[6] if t[6] else 0.0}
