"""Plain-Python restatement of the word definitions of include/srf.h (srf_word_split,
srf_word_align): the classification of a position (separator before the fold, dropped,
kept), words as maximal runs of kept labels between separators, word ids by first
appearance in the list reference words + hypothesis words, and the word alignment, which
is tests/score_ref.py's alignment run on the two id rows.  And the case generator of the
word tests: score_ref's edited pairs over an alphabet in which one label is the separator."""
import numpy as np

from tests import score_ref as sr


def split(seq, sep, fold=None):
    """The words of one label sequence: a list of (classes tuple, start, end), start / end
    the positions before the fold of the first kept label and one past the last."""
    words, cur, start, end = [], [], -1, -1
    for p, x in enumerate(seq):
        x = int(x)
        if x == sep:
            if cur:
                words.append((tuple(cur), start, end))
            cur = []
            continue
        if fold is not None:
            if not 0 <= x < len(fold) or fold[x] < 0:
                continue
            x = int(fold[x])
        if not cur:
            start = p
        cur.append(x)
        end = p + 1
    if cur:
        words.append((tuple(cur), start, end))
    return words


def ids(ref_words, hyp_words):
    """(reference ids, hypothesis ids): the index, in reference words + hypothesis words,
    of the first word equal to each."""
    both = [w[0] for w in ref_words] + [w[0] for w in hyp_words]
    first = [both.index(w) for w in both]
    return first[:len(ref_words)], first[len(ref_words):]


def align(hyp, ref, sep, fold=None, hmax=None, rmax=None):
    """One utterance: dict with counts [6] in words, the word tables (start, end, id; -1
    past the count) at the capacities (hmax + 1) // 2 and (rmax + 1) // 2, the two maps
    over word indices (-1 inserted / deleted, -2 past the count), the words themselves
    and the word-level ops of score_ref."""
    hmax = len(hyp) if hmax is None else hmax
    rmax = len(ref) if rmax is None else rmax
    WH, WR = (hmax + 1) // 2, (rmax + 1) // 2
    hw, rw = split(hyp, sep, fold), split(ref, sep, fold)
    rid, hid = ids(rw, hw)
    a = sr.align(hid, rid, None, WH, WR)

    def pad(v, n):
        return list(v) + [-1] * (n - len(v))
    return {'counts': a['counts'], 'hyp_to_ref': a['hyp_to_ref'], 'ref_to_hyp': a['ref_to_hyp'], 'ops': a['ops'],
            'hyp_words': [w[0] for w in hw], 'ref_words': [w[0] for w in rw],
            'hyp_word_start': pad([w[1] for w in hw], WH), 'hyp_word_end': pad([w[2] for w in hw], WH),
            'hyp_word_id': pad(hid, WH),
            'ref_word_start': pad([w[1] for w in rw], WR), 'ref_word_end': pad([w[2] for w in rw], WR),
            'ref_word_id': pad(rid, WR)}


def align_batch(hyp, hyp_len, ref, ref_len, sep, fold=None):
    """Dense [B][max] rows with lengths (clamped as the kernel clamps them)."""
    hmax = len(hyp[0]) if len(hyp) else 0
    rmax = len(ref[0]) if len(ref) else 0
    out = []
    for b in range(len(hyp)):
        nh, nr = max(0, min(int(hyp_len[b]), hmax)), max(0, min(int(ref_len[b]), rmax))
        out.append(align(list(hyp[b][:nh]), list(ref[b][:nr]), sep, fold, hmax, rmax))
    return out


def split_batch(labels, lengths, sep, fold=None):
    """Per row (start [W], end [W], count, words), W = (Lmax + 1) // 2, -1 past the count."""
    lmax = len(labels[0]) if len(labels) else 0
    W = (lmax + 1) // 2
    out = []
    for b in range(len(labels)):
        n = max(0, min(int(lengths[b]), lmax))
        ws = split(list(labels[b][:n]), sep, fold)
        out.append(([w[1] for w in ws] + [-1] * (W - len(ws)), [w[2] for w in ws] + [-1] * (W - len(ws)), len(ws),
                    [w[0] for w in ws]))
    return out


def word_error_rate(t):
    return {'substitutions': t[1], 'deletions': t[2], 'insertions': t[3], 'reference_words': t[4],
            'hypothesis_words': t[5], 'utterances': t[6],
            'word_error_rate': (t[1] + t[2] + t[3]) / t[4] if t[4] else 0.0,
            'sentence_error_rate': t[7] / t[6] if t[6] else 0.0}


def group_spans(label_spans, sep, fold=None):
    """The word spans of one utterance from its (label, start, end) label spans: (classes
    tuple, first label's start, last label's end) per word."""
    return [(w, label_spans[s][1], label_spans[e - 1][2]) for w, s, e in split([sp[0] for sp in label_spans], sep, fold)]


# (Hmax, Rmax) capacities of the device tests: empty and single labels; a word across a
# wave's edge (64 lanes); across a tile's edge (256 positions); the workload's size.
SHAPES = [(0, 5), (5, 0), (1, 1), (63, 64), (64, 65), (255, 257), (513, 300), (200, 200)]
ALPHABETS = (4, 30)
_REFERENCE = {}


def separator(A):
    return A   # the labels of a case are [0, A]: A ordinary classes and the separator


def with_separators(seq, A):
    """Labels drawn from [0, 6 A) as labels of [0, A]: one draw in six is the separator A,
    the others are spread evenly over the A classes."""
    v = np.asarray(seq, dtype=np.int64)
    return np.where(v % 6 == 5, A, v // 6)


def ragged_batch(seed, H, R, A, B=8):
    """score_ref.ragged_batch drawn from [0, 6 A) and passed through with_separators, so
    that about 1 label in 6 is the separator whatever the alphabet; the padding stays
    poison (-7 in the hypotheses, 10^9 in the references)."""
    hyp, hyp_len, ref, ref_len = sr.ragged_batch(100 + seed, H, R, 6 * A, B)
    for rows, lens in ((hyp, hyp_len), (ref, ref_len)):
        for b, n in enumerate(lens):
            rows[b, :n] = with_separators(rows[b, :n], A)
    return hyp, hyp_len, ref, ref_len


def reference(H, R, A):
    """The ragged batch of a shape and alphabet with its word alignments, computed once
    per process and shared: (hyp, hyp_len, ref, ref_len, results).  Callers leave it
    unchanged."""
    key = (H, R, A)
    if key not in _REFERENCE:
        hyp, hyp_len, ref, ref_len = ragged_batch(SHAPES.index((H, R)), H, R, A)
        _REFERENCE[key] = (hyp, hyp_len, ref, ref_len, align_batch(hyp, hyp_len, ref, ref_len, separator(A)))
    return _REFERENCE[key]


def totals(results):
    return sr.totals(results)
