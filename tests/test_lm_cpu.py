"""srf_amd/lm.py: the ARPA reader, the Witten-Bell estimator, the unfolding of a backoff
n-gram into the beam search's automaton, and the checks of fuse / from_tables."""
import itertools
import math

import numpy as np
import pytest

from srf_amd.lm import BOS, FusedLM, NGramLM

LN10 = math.log(10.0)

# A trigram over a, b, c with backoff weights.  Missing on purpose: the bigram "c a" (and
# every other bigram from c but "c c"), so the trigram contexts "x c" + a back off twice;
# the bigram context "b a" is no listed bigram although the trigram "b a c" is listed (a
# missing bigram context); the trigrams from "a b" but "a b c"; c has no trigram at all.
ARPA = r"""
\data\
ngram 1=6
ngram 2=7
ngram 3=4

\1-grams:
-99     <s>     -0.30
-1.0    </s>
-1.2    <unk>   -0.1
-0.50   a       -0.40
-0.70   b       -0.25
-0.90   c       -0.35

\2-grams:
-0.30   <s> a   -0.20
-0.80   <s> b
-0.40   a b     -0.15
-0.60   a a     -0.05
-0.35   b c     -0.45
-0.55   c c
-0.20   b </s>

\3-grams:
-0.10   <s> a b
-0.25   a b c
-0.45   b a c
-0.15   a a </s>

\end\
"""
SYMBOLS = {'a': 0, 'b': 1, 'c': 2}


def _direct(context, c):
    """log10 p(c | context) straight from the table above, by the ARPA recursion."""
    uni = {0: (-0.50, -0.40), 1: (-0.70, -0.25), 2: (-0.90, -0.35), BOS: (None, -0.30)}
    bi = {(BOS, 0): (-0.30, -0.20), (BOS, 1): (-0.80, 0.0), (0, 1): (-0.40, -0.15), (0, 0): (-0.60, -0.05),
          (1, 2): (-0.35, -0.45), (2, 2): (-0.55, 0.0)}
    tri = {(BOS, 0, 1): -0.10, (0, 1, 2): -0.25, (1, 0, 2): -0.45}
    h = tuple(context)[-2:]
    if len(h) == 2:
        if h + (c,) in tri:
            return tri[h + (c,)]
        return (bi[h][1] if h in bi else 0.0) + _direct(h[1:], c)
    if len(h) == 1:
        if h + (c,) in bi:
            return bi[h + (c,)][0]
        return uni[h[0]][1] + _direct((), c)
    return uni[c][0]


def test_arpa_automaton_equals_the_backoff_recursion():
    lm = NGramLM.from_arpa(ARPA, SYMBOLS)
    assert lm.order == 3 and lm.n_classes == 4
    logp, nxt = lm.automaton()
    listed = lm.contexts()
    assert (1, 0) in listed and (2, 0) not in listed and (2,) in listed   # "b a" only through its trigram
    states = {s: h for h, s in _state_index(lm).items()}
    assert states[0] == (BOS,)
    worst = 0.0
    for n in range(5):
        for seq in itertools.product(range(3), repeat=n):
            s, total, want = 0, 0.0, 0.0
            for i, c in enumerate(seq):
                total += logp[s, c]
                want += _direct((BOS,) + seq[:i], c) * LN10
                assert abs(lm.logp((BOS,) + seq[:i], c) - _direct((BOS,) + seq[:i], c) * LN10) < 1e-12
                s = nxt[s, c]
                # next lands on the longest listed suffix of the history
                h = ((BOS,) + seq[:i + 1])[-2:]
                while h not in listed:
                    h = h[1:]
                assert states[s] == h, (seq, i)
            worst = max(worst, abs(total - want))
    print(f'largest difference between automaton and recursion over 121 sequences: {worst:.2e}')
    assert worst < 1e-12
    # class 3 (the blank) has no unigram: missing_logp, behind the backoff weights of the context
    empty = int(nxt[0, 3])   # no context ends in a class that is not listed
    assert logp[empty, 3] == -30.0 and np.isfinite(logp).all()
    assert abs(logp[0, 3] - (-0.30 * LN10 - 30.0)) < 1e-12
    assert NGramLM.from_arpa(ARPA, SYMBOLS, missing_logp=-12.5).automaton()[0][empty, 3] == -12.5


def _state_index(lm):
    """context -> state, by walking the automaton from the start over all histories."""
    logp, nxt = lm.automaton()
    listed, index, todo = lm.contexts(), {}, [((BOS,), 0)]
    while todo:
        hist, s = todo.pop()
        h = hist[-(lm.order - 1):]
        while h not in listed:
            h = h[1:]
        if h in index:
            assert index[h] == s
            continue
        index[h] = s
        todo += [(hist + (c,), int(nxt[s, c])) for c in range(3)]
    return index


def test_arpa_from_a_file_and_unknown_token(tmp_path):
    path = tmp_path / 'lm.arpa'
    path.write_text(ARPA)
    a, b = NGramLM.from_arpa(str(path), SYMBOLS).automaton(), NGramLM.from_arpa(ARPA, SYMBOLS).automaton()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    with pytest.raises(ValueError, match="'c'"):
        NGramLM.from_arpa(ARPA, {'a': 0, 'b': 1})
    with pytest.raises(ValueError, match='ARPA'):
        NGramLM.from_arpa('no such file and no model', SYMBOLS)


def test_from_sequences_rows_sum_to_one_and_back_off():
    rng = np.random.default_rng(5)
    C, blank = 6, 5
    seqs = [rng.integers(0, 4, rng.integers(1, 9)).tolist() for _ in range(30)]   # class 4 is never seen
    for order in (1, 2, 3, 4):
        lm = NGramLM.from_sequences(seqs, order, C, blank)
        logp, nxt = lm.automaton()
        sums = np.exp(np.delete(logp, blank, axis=1)).sum(axis=1)
        print(f'order {order}: {len(logp)} states, row sums within {np.abs(sums - 1).max():.2e}')
        assert np.abs(sums - 1).max() < 1e-9
        assert np.isfinite(logp).all() and nxt.min() >= 0 and nxt.max() < len(logp)
    # an unseen context scores as the seen shorter one: nothing follows class 4 in the data
    lm = NGramLM.from_sequences(seqs, 3, C, blank)
    assert (0, 4) not in lm.contexts() and (4, 0) not in lm.contexts()
    for c in range(5):
        assert lm.logp((0, 4), c) == lm.logp((), c)
        assert lm.logp((4, 0), c) == lm.logp((0,), c)
    logp, nxt = lm.automaton()
    after0 = int(nxt[0, 0])                       # the context (BOS, 0)
    only4 = int(nxt[after0, 4])                   # (0, 4) is not listed: the context (4,), whatever came before
    assert only4 == int(nxt[int(nxt[int(nxt[after0, 1]), 2]), 4])
    for c in range(5):
        assert abs(logp[only4, c] - lm.logp((), c)) < 1e-12   # and (4,) has no weight and no continuation
    # seen more often, more probable; and the estimate is the interpolation it is said to be
    one = NGramLM.from_sequences([[0, 1], [0, 1], [0, 2]], 2, 4, 3)
    p = lambda h, c: math.exp(one.logp(h, c))
    uni = {c: (n + 3 * (1 / 3)) / (6 + 3) for c, n in ((0, 3), (1, 2), (2, 1))}   # 6 labels, 3 kinds
    assert abs(p((), 1) - uni[1]) < 1e-12
    assert abs(p((0,), 1) - (2 + 2 * uni[1]) / (3 + 2)) < 1e-12
    assert abs(p((0,), 0) - 2 / (3 + 2) * uni[0]) < 1e-12   # unseen after 0: the backoff weight t / (n + t)
    with pytest.raises(ValueError, match='blank'):
        NGramLM.from_sequences([[0, 3]], 2, 4, 3)


def test_fuse_and_from_tables_validate_on_the_host():
    lm = NGramLM.from_arpa(ARPA, SYMBOLS)
    f = lm.fuse(0.7, 0.2, blank=3, device='cpu')
    logp, nxt = lm.automaton()
    assert (f.n_states, f.n_classes) == logp.shape and f.bonus.dtype.is_floating_point
    want = (0.7 * logp + 0.2).astype(np.float32)
    want[:, 3] = 0
    assert np.array_equal(f.bonus_host, want) and np.array_equal(f.next_host, nxt)
    assert np.array_equal(f.bonus.numpy(), want) and f.next.numpy().dtype == np.int32
    assert abs(f.sequence_bonus([0, 1, 2]) - sum(0.7 * _direct((BOS, 0, 1)[:i + 1], c) * LN10 + 0.2
                                                  for i, c in enumerate([0, 1, 2]))) < 1e-5
    with pytest.raises(ValueError, match='blank'):
        lm.fuse(0.7, 0.2, blank=4, device='cpu')
    with pytest.raises(ValueError, match='finite'):
        lm.fuse(float('inf'), 0.2, blank=3, device='cpu')
    with pytest.raises(ValueError, match='finite'):
        lm.fuse(1e38, 0.0, blank=3, device='cpu')   # overflows float32
    bonus, nxt = np.zeros((3, 4), np.float32), np.zeros((3, 4), np.int32)
    FusedLM.from_tables(bonus, nxt, 3, 'cpu')
    for bad in (np.nan, np.inf, -np.inf):
        b = bonus.copy()
        b[1, 1] = bad
        with pytest.raises(ValueError, match='finite'):
            FusedLM.from_tables(b, nxt, 3, 'cpu')
    for bad in (-1, 3):
        n = nxt.copy()
        n[2, 0] = bad
        with pytest.raises(ValueError, match='outside'):
            FusedLM.from_tables(bonus, n, 3, 'cpu')
    with pytest.raises(ValueError, match='n_classes'):
        FusedLM.from_tables(bonus, np.zeros((3, 5), np.int32), 3, 'cpu')   # class counts differ
    with pytest.raises(ValueError, match='n_classes'):
        FusedLM.from_tables(np.zeros((3, 1), np.float32), np.zeros((3, 1), np.int32), 0, 'cpu')
    with pytest.raises(ValueError, match='blank'):
        FusedLM.from_tables(bonus, nxt, 4, 'cpu')
    with pytest.raises(ValueError, match='blank'):
        FusedLM.from_tables(bonus, nxt, -1, 'cpu')
    with pytest.raises(ValueError, match='integers'):
        FusedLM.from_tables(bonus, nxt.astype(np.float32), 3, 'cpu')
    # a non-finite value in the blank's column is never read and is stored as 0
    b = bonus.copy()
    b[:, 3] = np.nan
    assert np.all(FusedLM.from_tables(b, nxt, 3, 'cpu').bonus_host == 0)
