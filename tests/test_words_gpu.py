"""Device words (srf_word_split, srf_word_align, scoring.split_words / word_align /
WordErrorRate, ctc.Alignment.words and the trainer's metric lists and word spans) against
the plain-Python restatement of tests/words_ref.py.  Everything but the words' log-
probabilities is an integer and is compared for exact equality; the log-probabilities are
compared bit for bit with a float32 loop."""
import json
import os

import numpy as np
import pytest
import torch

from tests import score_ref as sr
from tests import words_ref as wr
from tests.helpers import config_from_shape, load_eval_fixture

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
TABLES = ('hyp_word_start', 'hyp_word_end', 'hyp_word_id', 'ref_word_start', 'ref_word_end', 'ref_word_id',
          'hyp_to_ref', 'ref_to_hyp')


def _dev(batch, cuda):
    hyp, hyp_len, ref, ref_len = batch[:4]
    # the poison 10^9 fits int32; -7 and 10^9 are never labels of the cases
    return (torch.tensor(np.asarray(hyp), dtype=torch.int32, device=cuda),
            torch.tensor(hyp_len, dtype=torch.int32, device=cuda),
            torch.tensor(np.asarray(ref), dtype=torch.int32, device=cuda),
            torch.tensor(ref_len, dtype=torch.int32, device=cuda))


def _assert_equal(al, results):
    got = {name: getattr(al, name).cpu().tolist() for name in ('counts',) + TABLES}
    for b, res in enumerate(results):
        for name in ('counts',) + TABLES:
            assert got[name][b] == res[name], (b, name, got[name][b], res[name])


def _assert_same(a, c):
    for name in ('counts',) + TABLES:
        assert torch.equal(getattr(a, name), getattr(c, name)), name


def _assert_split(words, labels, lengths, sep, fold=None):
    want = wr.split_batch(labels, lengths, sep, fold)
    assert words.start.cpu().tolist() == [w[0] for w in want]
    assert words.end.cpu().tolist() == [w[1] for w in want]
    assert words.count.cpu().tolist() == [w[2] for w in want]
    assert words.lists() == [w[3] for w in want]


@pytest.mark.parametrize('A', wr.ALPHABETS)
@pytest.mark.parametrize('H,R', wr.SHAPES)
def test_shapes_exact(cuda, H, R, A):
    """Ragged batches of 8 with poisoned padding (-7 / 10^9 past the lengths), about one
    separator in six labels: the counts, both word tables with their ids and both maps
    equal the reference; srf_word_split gives the same words for either side; the host view
    equals the reference's operations; a second call returns the same bits.  These shapes
    keep the word table in LDS and reach srf_edit_align's first two size classes."""
    from srf_amd import scoring
    batch = wr.reference(H, R, A)
    sep = wr.separator(A)
    hyp, hyp_len, ref, ref_len = _dev(batch, cuda)
    al = scoring.word_align(hyp, hyp_len, ref, ref_len, sep)
    _assert_equal(al, batch[4])
    assert al.ops() == [res['ops'] for res in batch[4]]
    _assert_split(scoring.split_words(hyp, hyp_len, sep), batch[0], batch[1], sep)
    _assert_split(scoring.split_words(ref, ref_len, sep), batch[2], batch[3], sep)
    _assert_same(scoring.word_align(hyp, hyp_len, ref, ref_len, sep), al)
    print(f'(H, R) = {(H, R)} A = {A}: word distances {al.counts[:, 0].cpu().tolist()} of '
          f'{al.counts[:, 4].cpu().tolist()} reference words')


@pytest.mark.parametrize('H,R', [(63, 64), (200, 200), (513, 300)])
def test_counts_and_maps_equal_the_label_alignment_of_interned_words(cuda, H, R):
    """An independent route: the words interned on the host (any numbering) and aligned as
    labels by scoring.edit_align give the same counts and maps."""
    from srf_amd import scoring
    batch = wr.reference(H, R, 4)
    al = scoring.word_align(*_dev(batch, cuda), wr.separator(4))
    intern = {}
    hid = [[intern.setdefault(w, len(intern)) for w in res['hyp_words']] for res in batch[4]]
    rid = [[intern.setdefault(w, len(intern)) for w in res['ref_words']] for res in batch[4]]
    lab = scoring.edit_align(hid, None, rid, None)
    assert torch.equal(lab.counts, al.counts)
    nh, nr = lab.hyp_to_ref.shape[1], lab.ref_to_hyp.shape[1]
    assert torch.equal(lab.hyp_to_ref, al.hyp_to_ref[:, :nh]) and torch.equal(lab.ref_to_hyp, al.ref_to_hyp[:, :nr])
    assert torch.all(al.hyp_to_ref[:, nh:] == -2) and torch.all(al.ref_to_hyp[:, nr:] == -2)


def _hand_rows(H, R):
    """Rows over the letters 1 .. 5, the separator 0 (which the fold would drop), the
    dropped class 6 and labels outside the fold table (-3, 7, 10^6)."""
    fold = [-1, 0, 1, 2, 3, 4, -1]
    a, b, c, sep, n = 1, 2, 3, 0, 6
    rows = []
    # one word that fills the capacity, longer than a wave and than a tile; the last label differs
    rows.append(([a, b, c, 4, 5] * (H // 5) + [a] * (H % 5), ([a, b, c, 4, 5] * (R // 5) + [a] * (R % 5))[:R - 1] + [5]))
    # label and separator in turn: the maximal word count
    rows.append((([a, sep] * H)[:H], ([b, sep, a, sep] * R)[:R]))
    # words equal but for the last label; words that are prefixes of one another
    rows.append(([a, b, c, sep, a, b, 4, sep, a, b, c, sep, a, b, 5], [a, b, c, sep, a, b, c, sep, a, b, 4, sep, a, b, 4]))
    rows.append(([a, sep, a, b, sep, a, b, c, sep, a, b, c, 4], [a, b, c, 4, sep, a, b, c, sep, a, b, sep, a, sep, a, b]))
    # the same word many times on both sides, across the wave's and the tile's edges
    rows.append(([a, b, c, sep] * (H // 4), [a, b, c, sep] * (R // 4 - 3) + [a, b, sep]))
    # dropped labels inside words and at their edges, labels outside the fold table
    rows.append(([n, a, n, b, n, sep, n, sep, -3, c, 7, sep, 10 ** 6, a, b], [a, b, sep, n, n, sep, c, n, sep, a, 7, b, n]))
    rows.append(([sep] * 9, [n] * 9))      # all separators, all dropped
    rows.append(([], [a]))
    hyp = np.full((len(rows), H), -7, dtype=np.int64)
    ref = np.full((len(rows), R), 10 ** 9, dtype=np.int64)
    for k, (h, r) in enumerate(rows):
        assert len(h) <= H and len(r) <= R
        hyp[k, :len(h)], ref[k, :len(r)] = h, r
    return hyp, [len(h) for h, _ in rows], ref, [len(r) for _, r in rows], sep, fold


def test_hand_built_rows(cuda):
    """One word that fills a capacity above 256 labels, the maximal word count (label and
    separator in turn, an odd capacity), words equal but for the last label, prefixes, one
    word many times on both sides, dropped labels inside words and at their edges, labels
    outside the fold table, and a separator that the fold would drop."""
    from srf_amd import scoring
    hyp, hyp_len, ref, ref_len, sep, fold = _hand_rows(301, 300)
    want = wr.align_batch(hyp, hyp_len, ref, ref_len, sep, fold)
    assert want[0]['counts'] == [1, 1, 0, 0, 1, 1] and want[1]['counts'][5] == 151 and want[1]['counts'][4] == 150
    assert want[4]['counts'][5] == 75 and want[5]['hyp_words'] == [(0, 1), (2,), (0, 1)]
    table = torch.tensor(fold, dtype=torch.int32, device=cuda)
    args = _dev((hyp, hyp_len, ref, ref_len), cuda)
    al = scoring.word_align(*args, sep, fold=table)
    _assert_equal(al, want)
    _assert_split(scoring.split_words(args[0], args[1], sep, fold=table), hyp, hyp_len, sep, fold)
    _assert_split(scoring.split_words(args[2], args[3], sep, fold=table), ref, ref_len, sep, fold)
    # without the fold the dropped labels are letters of their own
    _assert_equal(scoring.word_align(*args, sep), wr.align_batch(hyp, hyp_len, ref, ref_len, sep))
    print(f'hand-built rows: word distances {[w["counts"][0] for w in want]}')


@pytest.mark.parametrize('Hmax,Rmax,lens', [
    (700, 900, [(700, 900), (0, 0), (650, 640)]),       # table in LDS; srf_edit_align at KM = 8
    (2000, 1100, [(2000, 1100), (0, 1100), (30, 40)]),   # table in LDS; srf_edit_align's workgroup loop
    (6000, 1000, [(6000, 1000), (6000, 0), (900, 1000)]),   # table in more than 64 KiB of LDS
], ids=['km8', 'loop', 'lds-above-64k'])
def test_capacities_beyond_the_workload(cuda, Hmax, Rmax, lens):
    """The geometry follows the capacities (tensor widths), not the lengths.  The classes
    the implementation distinguishes are: the word table (compacted classes, per word its
    first index, length and hash) in at most 64 KiB of LDS, in more than 64 KiB of LDS
    (up to the 96 KiB budget), or in the workspace; and, by the word capacities, the
    classes of srf_edit_align (wave sweep with KM = 2, 4, 8; workgroup loop above 512
    reference words, which is also every case with the table in the workspace).
    test_shapes_exact reaches LDS with KM = 2 and 4, this test LDS with KM = 8, LDS with
    the loop and LDS above 64 KiB, test_full_capacity the workspace with the loop."""
    from srf_amd import scoring
    A = 30
    hyp = np.full((len(lens), Hmax), -7, dtype=np.int64)
    ref = np.full((len(lens), Rmax), 10 ** 9, dtype=np.int64)
    for b, (nh, nr) in enumerate(lens):
        h, r = sr.case(600 + b, nh, nr, 6 * A)
        hyp[b, :nh], ref[b, :nr] = wr.with_separators(h, A), wr.with_separators(r, A)
    hyp_len, ref_len = [n for n, _ in lens], [n for _, n in lens]
    want = wr.align_batch(hyp, hyp_len, ref, ref_len, A)
    al = scoring.word_align(*_dev((hyp, hyp_len, ref, ref_len), cuda), A)
    _assert_equal(al, want)
    print(f'capacity {(Hmax, Rmax)}: word distances {[w["counts"][0] for w in want]} of '
          f'{[w["counts"][4] for w in want]} reference words')


def test_full_capacity(cuda):
    """(8192, 8192), B = 2, the word table in the workspace: a hypothesis of label and
    separator in turn (4096 words, the most a row can hold) against a reference of 300
    such words, and one word of 8192 labels on both sides that differs in its last label
    in the hypothesis."""
    from srf_amd import scoring
    n, sep = 8192, 9
    hyp = np.full((2, n), -7, dtype=np.int64)
    ref = np.full((2, n), 10 ** 9, dtype=np.int64)
    rng = np.random.default_rng(11)
    hyp[0, 0::2], hyp[0, 1::2] = rng.integers(0, 5, n // 2), sep
    ref[0, 0:600:2], ref[0, 1:600:2] = hyp[0, 40:640:2], sep
    ref[0, 100] = 7                      # a word of the reference that no other word equals
    ref[1] = rng.integers(0, 5, n)
    hyp[1] = ref[1]
    hyp[1, n - 1] = 8
    hyp_len, ref_len = [n, n], [600, n]
    want = wr.align_batch(hyp, hyp_len, ref, ref_len, sep)
    assert want[0]['counts'][4:] == [300, 4096] and want[1]['counts'] == [1, 1, 0, 0, 1, 1]
    al = scoring.word_align(*_dev((hyp, hyp_len, ref, ref_len), cuda), sep)
    _assert_equal(al, want)
    same = hyp.copy()
    same[1, n - 1] = ref[1, n - 1]
    counts = scoring.word_align(*_dev((same, hyp_len, ref, ref_len), cuda), sep).counts.cpu().tolist()
    assert counts[1] == [0, 0, 0, 0, 1, 1] and counts[0] == want[0]['counts']
    words = scoring.split_words(*_dev((hyp, hyp_len, ref, ref_len), cuda)[:2], sep)
    assert words.count.cpu().tolist() == [4096, 1]
    assert words.start[0].cpu().tolist() == list(range(0, n, 2)) and words.end[1, 0].item() == n
    print(f'full capacity: word distances {[w["counts"][0] for w in want]}')


@pytest.mark.parametrize('H,R', [(64, 65), (200, 200), (513, 300)])
def test_padding_is_never_read(cuda, H, R):
    """The same utterances with the padding replaced by ordinary labels (the separator
    among them): nothing changes.  Lengths above the capacity and below zero are clamped."""
    from srf_amd import scoring
    batch = wr.reference(H, R, 4)
    sep = wr.separator(4)
    hyp, hyp_len, ref, ref_len = _dev(batch, cuda)
    clean_h, clean_r = hyp.clamp(0, 4), ref.clamp(0, 4)
    a, c = scoring.word_align(hyp, hyp_len, ref, ref_len, sep), scoring.word_align(clean_h, hyp_len, clean_r, ref_len, sep)
    _assert_same(a, c)
    over = scoring.word_align(clean_h, hyp_len + (hyp_len == H) * 5, clean_r, ref_len - (ref_len == 0) * 3, sep)
    _assert_same(a, over)
    ws, wc = scoring.split_words(ref, ref_len, sep), scoring.split_words(clean_r, ref_len - (ref_len == 0) * 3, sep)
    assert torch.equal(ws.start, wc.start) and torch.equal(ws.end, wc.end) and torch.equal(ws.count, wc.count)


def test_null_outputs_keep_the_rest(cuda):
    from srf_amd import ops
    for H, R in ((63, 64), (200, 200)):
        batch = wr.reference(H, R, 4)
        args = _dev(batch, cuda)
        full = ops.word_align(*args, wr.separator(4))
        counts, hw, rw, h2r, r2h = ops.word_align(*args, wr.separator(4), words=False, maps=False)
        assert hw == (None,) * 3 and rw == (None,) * 3 and h2r is None and r2h is None
        assert torch.equal(counts, full[0]) and counts.cpu().tolist() == [res['counts'] for res in batch[4]]
        counts, hw, rw, h2r, r2h = ops.word_align(*args, wr.separator(4), words=False)
        assert torch.equal(counts, full[0]) and torch.equal(h2r, full[3]) and torch.equal(r2h, full[4])
        counts, hw, rw, h2r, r2h = ops.word_align(*args, wr.separator(4), maps=False)
        assert torch.equal(counts, full[0]) and all(torch.equal(x, y) for x, y in zip(hw + rw, full[1] + full[2]))


def test_word_error_rate(cuda):
    """Two updates equal the reference's sums, a reset zeroes them, lists are taken as
    tensors are; on the reference pipeline's own self-check rows the rate per row is
    [0.111, 0.105]."""
    from srf_amd import scoring
    wer = scoring.WordErrorRate(wr.separator(30), device=cuda)
    results = []
    for H, R in ((64, 65), (200, 200)):
        batch = wr.reference(H, R, 30)
        wer.update_state(*_dev(batch, cuda))
        results += batch[4]
    t = wr.totals(results)
    assert wer.state().dtype == torch.int64 and wer.state().cpu().tolist() == t
    assert wer.result() == wr.word_error_rate(t)
    print(f'word error rate {wer.result()["word_error_rate"]:.4f}, sentences {wer.result()["sentence_error_rate"]:.4f}')
    assert t[4] > 100 and 0 < t[1] + t[2] + t[3] < t[4]
    wer.reduce()   # world size 1: nothing happens
    assert wer.state().cpu().tolist() == t
    wer.reset_states()
    assert not wer.state().any() and wer.result() == wr.word_error_rate([0] * 8)

    with open(os.path.join(GOLD, 'wer_selfcheck.json')) as fh:
        fx = json.load(fh)
    fold = [-1 if c in fx['dropped'] else c for c in range(fx['n_classes'])]
    al = scoring.word_align(fx['hyp'], None, fx['ref'], None, fx['separator'], fold=fold)
    counts = al.counts.cpu().tolist()
    wers = [round(c[0] / c[4] * 1000) / 1000 for c in counts]
    print(f'self-check rows: distances {[c[0] for c in counts]} words {[c[4] for c in counts]} WERs {wers}')
    assert wers == fx['expected_wers'] == [0.111, 0.105]
    assert [c[0] for c in counts] == fx['expected_distances'] and [c[4] for c in counts] == fx['expected_reference_words']
    check = scoring.WordErrorRate(fx['separator'], fold=fold, device=cuda)
    check.update_state(fx['hyp'], None, fx['ref'], None)
    want = [wr.align(h, r, fx['separator'], fold) for h, r in zip(fx['hyp'], fx['ref'])]
    assert check.result() == wr.word_error_rate(wr.totals(want))
    assert check.result()['word_error_rate'] == 4 / 37 and check.result()['sentence_error_rate'] == 1.0


def test_word_times(cuda):
    """ctc.forced_align on random logits (T' = 40, C = 8) with labels that hold separators:
    a word's frames are its first label's token_start and its last label's token_end, its
    log-probability is bit-equal to the float32 sequential sum of the returned token_logp
    over [start, end), and an infeasible utterance has no spans."""
    from srf_amd import ctc
    T, C, sep, blank = 40, 8, 0, 7
    g = torch.Generator().manual_seed(3)
    logits = torch.randn((4, T, C), generator=g).to(cuda)
    labels = [[1, 2, 0, 3, 3, 4, 0, 0, 5, 6, 1], [0, 2, 6, 5, 0], [1, 1, 1, 1, 0, 2, 2, 2, 2, 0, 3, 3], [4, 5, 6]]
    lens = [40, 33, 12, 40]   # utterance 2: 12 labels with repeats need 19 frames, it has 12: infeasible
    fold = [-1, 0, 1, 2, 3, 4, -1]   # drops 6 (and would drop the separator)
    al = ctc.forced_align(logits, lens, labels, blank_index=blank)
    assert torch.isinf(al.score[2]) and al.spans()[2] == [] and torch.isfinite(al.score[[0, 1, 3]]).all()
    ts, te = al.token_start.cpu().numpy(), al.token_end.cpu().numpy()
    lp = al.token_logp.cpu().numpy()
    assert lp.dtype == np.float32
    for f in (None, fold):
        words = al.words(sep, fold=f)
        ref = wr.split_batch(al.labels.cpu().tolist(), [len(l) for l in labels], sep, f)
        assert words.start.cpu().tolist() == [r[0] for r in ref] and words.count.cpu().tolist() == [r[2] for r in ref]
        fs, fe, wl = words.frame_start.cpu().numpy(), words.frame_end.cpu().numpy(), words.logp.cpu().numpy()
        spans = words.spans()
        for b, (start, end, count, tuples) in enumerate(ref):
            want = []
            for k in range(count):
                acc = np.float32(0)
                for p in range(start[k], end[k]):
                    acc = np.float32(acc + lp[b, p])
                if b == 2:
                    assert (fs[b, k], fe[b, k], wl[b, k]) == (-1, -1, 0)
                    continue
                assert fs[b, k] == ts[b, start[k]] and fe[b, k] == te[b, end[k] - 1]
                assert wl[b, k].tobytes() == acc.tobytes(), (b, k, wl[b, k], acc)
                want.append((tuples[k], int(fs[b, k]), int(fe[b, k])))
            assert np.all(fs[b, count:] == -1) and np.all(fe[b, count:] == -1) and np.all(wl[b, count:] == 0)
            assert spans[b] == want
        assert spans[2] == [] and len(spans[0]) == 3
    assert [w for w, _, _ in al.words(sep, fold=fold).spans()[1]] == [(1, 4)]


@pytest.fixture(scope='module')
def mini(cuda):
    from srf_amd.sequence_router import SequenceRouter
    kw, sh, P, z, ev = load_eval_fixture('c2_mini')
    model = SequenceRouter(config_from_shape(kw), None, sh.class_n, device=cuda)
    model.load_params(P)
    inputs = (torch.tensor(z['feats'], dtype=torch.float32, device=cuda), torch.tensor(z['labels'], device=cuda),
              torch.tensor(z['inp_len'], dtype=torch.int32, device=cuda), torch.tensor(z['tar_len'], device=cuda))
    refs = [[int(v) for v in z['labels'][b][:int(z['tar_len'][b])]] for b in range(len(z['tar_len']))]
    flat = [v for r in refs for v in r]
    # the most frequent label parts the words; among equally frequent ones (every label of this
    # fixture appears once) the one that cuts the references into the most words, then the lowest
    top = max(flat.count(v) for v in flat)
    sep = max((v for v in sorted(set(flat)) if flat.count(v) == top),
              key=lambda v: sum(len(wr.split(r, v)) for r in refs))
    assert max(len(wr.split(r, sep)) for r in refs) >= 2
    return model, sh, refs, inputs, sep


def test_valid_step_metric_list(cuda, mini):
    from srf_amd import ctc, scoring, trainer_sr
    model, sh, refs, inputs, sep = mini
    blank = sh.class_n - 1
    plain = trainer_sr.process_valid_step(4, inputs, model, None, blank)
    er, wer = scoring.ErrorRate(device=cuda), scoring.WordErrorRate(sep, device=cuda)
    both = trainer_sr.process_valid_step(4, inputs, model, trainer_sr.Mean(), blank, error_state=[er, wer])
    assert torch.equal(plain, both)
    alone = scoring.WordErrorRate(sep, device=cuda)
    assert torch.equal(plain, trainer_sr.process_valid_step(4, inputs, model, None, blank, error_state=alone))
    with torch.no_grad():
        logits = model(inputs[0], input_lengths=inputs[2], training=False)
    hyps = ctc.greedy_decode(logits, trainer_sr.ceil_div(inputs[2], 4), blank)
    want_er = sr.error_rate(sr.totals([sr.align(h, r) for h, r in zip(hyps, refs)]))
    want_wer = wr.word_error_rate(wr.totals([wr.align(h, r, sep) for h, r in zip(hyps, refs)]))
    print(f'c2_mini greedy, separator {sep}: {er.result()} {wer.result()}')
    assert er.result() == want_er and wer.result() == want_wer and alone.result() == want_wer
    assert want_wer['utterances'] == len(hyps) and want_wer['reference_words'] == sum(len(wr.split(r, sep)) for r in refs)


@pytest.mark.parametrize('kw', [dict(), dict(beam_width=4, decoder='device')], ids=['greedy', 'device-beam4'])
def test_test_step_word_spans(cuda, mini, capsys, kw):
    from srf_amd import scoring, trainer_sr
    model, sh, refs, inputs, sep = mini
    test_inputs = (*inputs, [f'utt{b}' for b in range(inputs[0].shape[0])])
    hyps, spans = trainer_sr.process_test_step(4, test_inputs, model, timestamps=True, **kw)
    out_plain = capsys.readouterr().out
    er, wer = scoring.ErrorRate(device=cuda), scoring.WordErrorRate(sep, device=cuda)
    scored = trainer_sr.process_test_step(4, test_inputs, model, timestamps=True, score=(er, wer), word_separator=sep,
                                          **kw)
    assert capsys.readouterr().out == out_plain
    assert len(scored) == 3 and scored[0] == hyps and scored[1] == spans
    assert scored[2] == [wr.group_spans(s, sep) for s in spans]
    assert sum(len(s) for s in scored[2]) == sum(len(wr.split(h, sep)) for h in hyps)
    assert trainer_sr.process_test_step(4, test_inputs, model, score=[er], **kw) == hyps
    capsys.readouterr()
    assert wer.result() == wr.word_error_rate(wr.totals([wr.align(h, r, sep) for h, r in zip(hyps, refs)]))
    fold = [c if c != hyps[0][0] else -1 for c in range(sh.class_n)] if hyps[0] else None
    folded = trainer_sr.process_test_step(4, test_inputs, model, timestamps=True, word_separator=sep, word_fold=fold, **kw)
    capsys.readouterr()
    assert folded[:2] == (hyps, spans) and folded[2] == [wr.group_spans(s, sep, fold) for s in spans]
