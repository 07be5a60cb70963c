"""The word reference (tests/words_ref.py) pinned on the host: worked examples of the
definition, the reference pipeline's own WER self-check, the host views of scoring.Words,
the invariants of every generated case, and the argument checks of srf_word_split,
srf_word_align and their wrappers.  Needs no GPU.  Each test prints its figures before it
asserts."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tests import score_ref as sr
from tests import words_ref as wr

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
A, B, C, N, S = 1, 2, 3, 7, 9   # three letters, a label the fold drops, the separator
FOLD = [-1, 0, 1, 2]            # 0 and everything from 4 on are dropped


def _words(seq, fold=FOLD):
    return wr.split(seq, S, fold)


def test_worked_examples_of_the_split():
    # leading, trailing and double separators make no words
    assert _words([S, S, A, B, S, S, C, S]) == [((0, 1), 2, 4), ((2,), 6, 7)]
    # a dropped label inside a word neither splits it nor adds to it; at an edge it is outside [start, end)
    assert _words([A, N, B]) == [((0, 1), 0, 3)]
    assert _words([N, A, B, N, S, N, C]) == [((0, 1), 1, 3), ((2,), 6, 7)]
    assert _words([S, S, S]) == [] and _words([N, 0, N]) == [] and _words([N, S, N]) == [] and _words([]) == []
    # the raw label is tested before the fold: a separator the fold would drop stays one
    assert wr.split([A, 0, B], 0, FOLD) == [((0,), 0, 1), ((1,), 2, 3)]
    # without a fold every label that is no separator is kept with its own class
    assert wr.split([5, -3, S, 10 ** 6], S) == [((5, -3), 0, 2), ((10 ** 6,), 3, 4)]


def test_worked_examples_of_ids_and_alignment():
    a = wr.align([A, B], [A, S, B], S, FOLD)            # AB against A B
    assert a['hyp_word_id'] == [2] and a['ref_word_id'] == [0, 1]
    assert a['counts'] == [2, 1, 1, 0, 2, 1] and a['ops'] == [('del', -1, 0), ('sub', 0, 1)]
    a = wr.align([A, B, S, A], [A, S, A, B, C], S, FOLD)   # a word against its own prefix
    assert a['ref_word_id'] == [0, 1, -1] and a['hyp_word_id'] == [2, 0]
    assert a['counts'][0] == 2
    a = wr.align([A, S, A, S, B, S, A], [B, S, A, S, A, N], S, FOLD)
    assert a['ref_word_id'] == [0, 1, 1] and a['hyp_word_id'] == [1, 1, 0, 1]
    assert a['ref_word_start'] == [0, 2, 4] and a['ref_word_end'] == [1, 3, 5]
    a = wr.align([C, S, C], [], S, FOLD)                # only hypothesis words: ids R + i'
    assert a['hyp_word_id'] == [0, 0] and a['counts'] == [2, 0, 0, 2, 0, 2] and a['ref_word_id'] == []
    a = wr.align([S, S], [N, N], S, FOLD)               # all separators against all dropped
    assert a['counts'] == [0] * 6 and a['hyp_to_ref'] == [-2] and a['ref_to_hyp'] == [-2]
    assert wr.align([], [], S)['counts'] == [0] * 6


def _selfcheck():
    with open(os.path.join(GOLD, 'wer_selfcheck.json')) as fh:
        fx = json.load(fh)
    fold = [-1 if c in fx['dropped'] else c for c in range(fx['n_classes'])]
    return fx, fold


def test_selfcheck_fixture_through_the_reference():
    """The four id rows of the reference pipeline's WER self-check: word distances [2, 2],
    reference words [18, 19], rounded WERs [0.111, 0.105]."""
    fx, fold = _selfcheck()
    res = [wr.align(h, r, fx['separator'], fold) for h, r in zip(fx['hyp'], fx['ref'])]
    dist, words = [r['counts'][0] for r in res], [r['counts'][4] for r in res]
    wers = [round(d / w * 1000) / 1000 for d, w in zip(dist, words)]
    print(f'distances {dist} reference words {words} WERs {wers}')
    assert dist == fx['expected_distances'] and words == fx['expected_reference_words']
    assert wers == fx['expected_wers']
    for r in res:
        assert r['counts'][1] + r['counts'][2] + r['counts'][3] == r['counts'][0]


def _wsj():
    with open(os.path.join(GOLD, 'wsj_31.vocab')) as fh:
        vocab = [line.strip() for line in fh]
    return vocab


def test_text_on_wsj_ids_equals_the_log_rule():
    """Words.text() with the WSJ recipe (separator <SPACE>, fold dropping <PADDING_MASK>)
    against the rule of the reference's log converter (<SPACE> becomes a blank, the rest is
    spelled out, the ends are stripped), up to repeated blanks."""
    from srf_amd import scoring
    vocab = _wsj()
    assert len(vocab) == 31 and vocab[0] == '<PADDING_MASK>' and vocab[1] == '<SPACE>' and vocab[4] == 'A'
    sep = vocab.index('<SPACE>')
    table, names = scoring.fold_table(vocab, {v: v for v in vocab if v != '<PADDING_MASK>'}, device='cpu')
    fold = table.tolist()
    assert fold[0] == -1 and len(names) == 30
    rng = np.random.default_rng(5)
    rows = []
    for n in (0, 1, 17, 40, 40):
        rows.append([sep if rng.random() < 0.25 else int(rng.integers(2, 31)) for _ in range(n)])
    rows[3][:2], rows[3][-1] = [sep, sep], sep
    Lmax = max(len(r) for r in rows)
    labels = torch.tensor([r + [0] * (Lmax - len(r)) for r in rows], dtype=torch.int32)
    lengths = torch.tensor([len(r) for r in rows], dtype=torch.int32)
    ref = wr.split_batch(labels.tolist(), lengths.tolist(), sep, fold)
    words = scoring.Words(labels, lengths, sep, table, torch.tensor([r[0] for r in ref], dtype=torch.int32),
                          torch.tensor([r[1] for r in ref], dtype=torch.int32),
                          torch.tensor([r[2] for r in ref], dtype=torch.int32))
    assert words.lists() == [r[3] for r in ref]
    want = []
    for r in rows:
        a = ''.join(' ' if vocab[x] == '<SPACE>' else vocab[x] for x in r)
        want.append(' '.join(a.strip().split()))
    print(want)
    assert words.text(names) == want
    with pytest.raises(ValueError, match='alignment'):
        words.spans()


@pytest.mark.parametrize('H,R', wr.SHAPES)
def test_invariants_on_every_case(H, R):
    n_words = 0
    for alphabet in wr.ALPHABETS:
        hyp, hyp_len, ref, ref_len, results = wr.reference(H, R, alphabet)
        assert hyp_len[0] == H and ref_len[0] == R
        for b, res in enumerate(results):
            d, s, dl, ins, nr, nh = res['counts']
            assert s + dl + ins == d and nr <= (R + 1) // 2 and nh <= (H + 1) // 2
            assert nr == len(res['ref_words']) and nh == len(res['hyp_words'])
            h2r, r2h = res['hyp_to_ref'], res['ref_to_hyp']
            for i, j in enumerate(h2r):
                assert j < 0 or r2h[j] == i
            for j, i in enumerate(r2h):
                assert i < 0 or h2r[i] == j
            for m in (h2r, r2h):
                pos = [v for v in m if v >= 0]
                assert all(x < y for x, y in zip(pos[:-1], pos[1:]))
            assert all(res['ref_word_id'][j] <= j for j in range(nr))
            assert all(res['hyp_word_id'][i] <= nr + i for i in range(nh))
            # the distance is that of the words compared as tuples
            assert d == sr.distance_two_rows(res['hyp_words'], res['ref_words'])
            n_words += nr + nh
    print(f'(H, R) = {(H, R)}: {n_words} words')
    assert n_words > 0 or max(H, R) <= 1


def test_cases_hold_about_one_separator_in_six_and_repeated_words():
    hyp, hyp_len, ref, ref_len, results = wr.reference(200, 200, 30)
    seps = sum(int((ref[b, :ref_len[b]] == 30).sum()) for b in range(8))
    labels = int(sum(ref_len))
    small = wr.reference(200, 200, 4)[4]
    repeated = sum(1 for r in small for j, v in enumerate(r['ref_word_id'][:r['counts'][4]]) if v < j)
    shared = sum(1 for r in small for v in r['hyp_word_id'][:r['counts'][5]] if v < r['counts'][4])
    fresh = sum(1 for r in small for i, v in enumerate(r['hyp_word_id'][:r['counts'][5]]) if v == r['counts'][4] + i)
    print(f'{seps} separators in {labels} labels; at alphabet 4 {repeated} repeated reference words, {shared} '
          f'hypothesis words equal to a reference word, {fresh} new ones')
    assert 0.10 < seps / labels < 0.25 and repeated >= 1 and shared > 10 and fresh > 10


def test_signatures_hold_the_names():
    from srf_amd import _lib
    for name, n in (('srf_word_split_workspace', 2), ('srf_word_split', 19), ('srf_word_align_workspace', 3),
                    ('srf_word_align', 23)):
        assert len(_lib._SIGNATURES[name][1]) == n, name


def test_entry_points_refuse_bad_arguments_without_gpu():
    from srf_amd import _lib
    L = _lib.lib()
    assert L.srf_word_split_workspace(1, 0) >= 16 and L.srf_word_split_workspace(28, 8192) >= 16
    assert L.srf_word_align_workspace(1, 0, 0) >= 16 and L.srf_word_align_workspace(28, 200, 200) >= 16
    # at the capacity the table leaves LDS for the workspace: 2 * 8192 classes and 3 * 8192 word entries
    assert L.srf_word_align_workspace(2, 8192, 8192) >= 2 * 4 * (2 * 8192 + 3 * 8192)
    fake = ctypes.c_void_p(4096)   # never dereferenced: every call below is refused before a launch
    for nb, H, R in ((0, 4, 4), (-1, 4, 4), (1, -1, 4), (1, 4, -1), (1, 8193, 4), (1, 4, 8193)):
        assert L.srf_word_align_workspace(nb, H, R) == 0, (nb, H, R)
        assert b'bad shape' in L.srf_last_error()
        assert L.srf_word_align(fake, fake, H, fake, fake, R, nb, None, 0, 1, fake, *[None] * 9, fake, 1 << 30,
                                None) == -1, (nb, H, R)
        assert b'bad shape' in L.srf_last_error()
    for nb, n in ((0, 4), (1, -1), (1, 8193)):
        assert L.srf_word_split_workspace(nb, n) == 0 and b'bad shape' in L.srf_last_error()
        assert L.srf_word_split(fake, fake, n, nb, None, 0, 1, fake, fake, fake, *[None] * 6, fake, 1 << 30, None) == -1
        assert b'bad shape' in L.srf_last_error()

    def align(hyp=fake, hyp_len=fake, ref=fake, ref_len=fake, fold=None, n_fold=0, counts=fake, ws=fake, wb=1 << 30):
        return L.srf_word_align(hyp, hyp_len, 4, ref, ref_len, 4, 1, fold, n_fold, 1, counts, *[None] * 9, ws, wb, None)
    for kw in (dict(hyp=None), dict(hyp_len=None), dict(ref=None), dict(ref_len=None), dict(counts=None), dict(ws=None)):
        assert align(**kw) == -1, kw
        assert b'null' in L.srf_last_error(), (kw, L.srf_last_error())
    assert align(n_fold=3) == -1 and b'n_fold' in L.srf_last_error()
    assert align(fold=fake, n_fold=-1) == -1 and b'n_fold' in L.srf_last_error()
    assert align(ws=ctypes.c_void_p(4100)) == -1 and b'aligned' in L.srf_last_error()
    assert align(wb=8) == -4 and b'workspace too small' in L.srf_last_error()

    def split(labels=fake, label_len=fake, start=fake, end=fake, count=fake, tok=(None,) * 3, out=(None,) * 3, ws=fake,
              wb=1 << 30):
        return L.srf_word_split(labels, label_len, 4, 1, None, 0, 1, start, end, count, *tok, *out, ws, wb, None)
    for kw in (dict(labels=None), dict(label_len=None), dict(start=None), dict(end=None), dict(count=None),
               dict(ws=None)):
        assert split(**kw) == -1, kw
        assert b'null' in L.srf_last_error(), (kw, L.srf_last_error())
    # a partial tok_* triple, frame outputs without the triple, the triple without all frame outputs
    for tok in ((fake, None, None), (fake, fake, None), (None, fake, fake)):
        assert split(tok=tok, out=(fake,) * 3) == -1 and b'together' in L.srf_last_error()
    assert split(out=(fake,) * 3) == -1 and b'frame outputs' in L.srf_last_error()
    assert split(tok=(fake,) * 3, out=(fake, fake, None)) == -1 and b'frame outputs' in L.srf_last_error()
    assert split(ws=ctypes.c_void_p(4100)) == -1 and b'aligned' in L.srf_last_error()
    assert split(wb=8) == -4 and b'workspace too small' in L.srf_last_error()


def test_wrappers_refuse_host_tensors_and_bad_arguments():
    from srf_amd import ops, scoring
    hyp = torch.zeros((2, 3), dtype=torch.int32)
    n = torch.tensor([3, 3], dtype=torch.int32)
    with pytest.raises(ValueError, match='device tensor'):
        scoring.word_align(hyp, n, [[0], [1]], None, 1)
    with pytest.raises(ValueError, match='device tensor'):
        scoring.split_words(hyp, n, 1)
    with pytest.raises(ValueError, match='takes 8192'):
        scoring.word_align([[0] * 8193], None, [[0]], None, 1)
    with pytest.raises(ValueError, match='takes 8192'):
        scoring.split_words([[0] * 8193], None, 1)
    with pytest.raises(ValueError, match='holds 0 utterances'):
        scoring.split_words([], None, 1)
    with pytest.raises(ValueError, match='separator'):
        scoring.word_align([[0]], None, [[0]], None, None)
    with pytest.raises(ValueError, match='separator'):
        scoring.WordErrorRate(1.5, device='cpu')
    with pytest.raises(ValueError, match='fold'):
        scoring.WordErrorRate(1, fold=[[0, 1]], device='cpu')
    wer = scoring.WordErrorRate(1, device='cpu')
    with pytest.raises(ValueError, match='device tensor'):
        wer.update_state(hyp, n, hyp, n)
    with pytest.raises(ValueError, match='HIP device'):
        wer.update_state([[0]], None, [[0]], None)
    assert wer.result() == wr.word_error_rate([0] * 8)
    wer.reduce()   # no process group: nothing happens
    with pytest.raises(ValueError, match='int32 device tensor'):
        ops.word_align(hyp, n, hyp, n, 1)
    with pytest.raises(ValueError, match='int32 device tensor'):
        ops.word_split(hyp, n, 1)
    with pytest.raises(ValueError, match=r'\[B, Hmax\]'):
        ops.word_align(hyp[0], n, hyp, n, 1)
    with pytest.raises(ValueError, match=r'\[B, Lmax\]'):
        ops.word_split(hyp[0], n, 1)


def test_trainer_refuses_word_arguments_that_do_not_fit():
    from srf_amd import trainer_sr
    with pytest.raises(ValueError, match='word_separator'):
        trainer_sr.process_test_step(4, None, None, word_fold=[0, 1])
    with pytest.raises(ValueError, match='timestamps'):
        trainer_sr.process_test_step(4, None, None, word_separator=1)
