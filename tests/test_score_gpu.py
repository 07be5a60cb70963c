"""Device scoring (srf_edit_align, scoring.edit_align, scoring.ErrorRate and the trainer's
error_state / score arguments) against the plain-Python restatement of tests/score_ref.py.
Everything is an integer, so everything is compared for exact equality."""
import json
import os

import numpy as np
import pytest
import torch

from tests import score_ref as sr
from tests.helpers import config_from_shape, load_eval_fixture

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _dev(batch, cuda):
    hyp, hyp_len, ref, ref_len = batch[:4]
    # the poison 10^9 fits int32; -7 and 10^9 are never labels of the cases
    return (torch.tensor(hyp, dtype=torch.int32, device=cuda), torch.tensor(hyp_len, dtype=torch.int32, device=cuda),
            torch.tensor(ref, dtype=torch.int32, device=cuda), torch.tensor(ref_len, dtype=torch.int32, device=cuda))


def _assert_equal(al, results):
    counts, h2r, r2h = al.counts.cpu().tolist(), al.hyp_to_ref.cpu().tolist(), al.ref_to_hyp.cpu().tolist()
    for b, res in enumerate(results):
        assert counts[b] == res['counts'], (b, counts[b], res['counts'])
        assert h2r[b] == res['hyp_to_ref'], b
        assert r2h[b] == res['ref_to_hyp'], b


@pytest.mark.parametrize('A', sr.ALPHABETS)
@pytest.mark.parametrize('H,R', sr.SHAPES)
def test_shapes_exact(cuda, H, R, A):
    """Ragged batches of 8 with poisoned padding (-7 / 10^9 past the lengths): counts and
    both maps equal the reference, the map entries past a length are -2, the host view
    equals the reference's operations, and a second call returns the same bits."""
    from srf_amd import scoring
    batch = sr.reference(H, R, A)
    hyp, hyp_len, ref, ref_len = _dev(batch, cuda)
    al = scoring.edit_align(hyp, hyp_len, ref, ref_len)
    _assert_equal(al, batch[4])
    h2r, r2h = al.hyp_to_ref.cpu().numpy(), al.ref_to_hyp.cpu().numpy()
    for b in range(len(batch[4])):
        assert np.all(h2r[b, batch[1][b]:] == -2) and np.all(r2h[b, batch[3][b]:] == -2)
    assert al.ops() == [res['ops'] for res in batch[4]]
    again = scoring.edit_align(hyp, hyp_len, ref, ref_len)
    assert torch.equal(again.counts, al.counts) and torch.equal(again.hyp_to_ref, al.hyp_to_ref)
    assert torch.equal(again.ref_to_hyp, al.ref_to_hyp)
    print(f'(H, R) = {(H, R)} A = {A}: distances {al.counts[:, 0].cpu().tolist()}')


@pytest.mark.parametrize('H,R', [(7, 9), (200, 200), (300, 512), (600, 700)])
def test_padding_is_never_read(cuda, H, R):
    """The same utterances with the padding replaced by ordinary labels: nothing changes."""
    from srf_amd import scoring
    batch = sr.reference(H, R, 4)
    hyp, hyp_len, ref, ref_len = _dev(batch, cuda)
    clean_h, clean_r = hyp.clamp(0, 3), ref.clamp(0, 3)
    a, c = scoring.edit_align(hyp, hyp_len, ref, ref_len), scoring.edit_align(clean_h, hyp_len, clean_r, ref_len)
    assert torch.equal(a.counts, c.counts) and torch.equal(a.hyp_to_ref, c.hyp_to_ref)
    assert torch.equal(a.ref_to_hyp, c.ref_to_hyp)
    # lengths beyond the capacity and below zero are clamped
    over = scoring.edit_align(clean_h, hyp_len + (hyp_len == H) * 5, clean_r, ref_len - (ref_len == 0) * 3)
    assert torch.equal(over.counts, a.counts) and torch.equal(over.hyp_to_ref, a.hyp_to_ref)


@pytest.mark.parametrize('Hmax,Rmax,lens', [
    (2000, 128, [(2000, 128), (0, 0), (150, 128)]),      # wave sweep with more than 64 KiB of LDS
    (8192, 64, [(8192, 64), (8192, 0), (40, 64)]),       # wave sweep, the head in the workspace
    (7400, 513, [(7400, 20), (30, 513), (0, 0)]),        # workgroup loop, the head in the workspace
    (64, 8192, [(64, 8192), (0, 8192), (3, 100)]),       # workgroup loop at the widest row
], ids=['lds-above-64k', 'wave-head-in-workspace', 'loop-head-in-workspace', 'loop-widest'])
def test_capacities_beyond_the_workload(cuda, Hmax, Rmax, lens):
    """The geometry follows the capacities (tensor widths), not the lengths: the paths
    that the shapes above do not reach, with utterances at the capacity's edge."""
    from srf_amd import scoring
    hyp = np.full((len(lens), Hmax), -7, dtype=np.int64)
    ref = np.full((len(lens), Rmax), 10 ** 9, dtype=np.int64)
    for b, (nh, nr) in enumerate(lens):
        h, r = sr.case(500 + b, nh, nr, 4)
        hyp[b, :nh], ref[b, :nr] = h, r
    hyp_len, ref_len = [n for n, _ in lens], [n for _, n in lens]
    want = sr.align_batch(hyp, hyp_len, ref, ref_len)
    al = scoring.edit_align(*_dev((hyp, hyp_len, ref, ref_len), cuda))
    _assert_equal(al, want)
    print(f'capacity {(Hmax, Rmax)}: distances {[w["counts"][0] for w in want]}')


def test_null_maps_keep_the_counts(cuda):
    from srf_amd import ops
    for H, R in ((17, 15), (200, 200), (600, 700)):
        batch = sr.reference(H, R, 4)
        args = _dev(batch, cuda)
        counts, h2r, r2h = ops.edit_align(*args, maps=False)
        assert h2r is None and r2h is None
        assert counts.cpu().tolist() == [res['counts'] for res in batch[4]]


def test_list_input_and_worked_examples(cuda):
    from srf_amd import scoring
    hyps = [[1, 2, 3], [1, 2], [1, 1, 2], [1, 2], []]
    refs = [[1, 3], [2, 1], [1, 2], [1, 1, 2], [4, 5]]
    al = scoring.edit_align(hyps, None, refs, None)
    _assert_equal(al, [sr.align(h, r, hmax=3, rmax=3) for h, r in zip(hyps, refs)])
    assert al.counts.cpu().tolist() == [[1, 0, 0, 1, 2, 3], [2, 2, 0, 0, 2, 2], [1, 0, 0, 1, 2, 3], [1, 0, 1, 0, 3, 2],
                                        [2, 0, 2, 0, 2, 0]]
    assert al.ops()[2] == [('ins', 0, -1), ('cor', 1, 0), ('cor', 2, 1)]
    assert al.ops()[3] == [('del', -1, 0), ('cor', 0, 1), ('cor', 1, 2)]


def _timit(cuda):
    from srf_amd import scoring
    with open(os.path.join(GOLD, 'timit_fold.json')) as fh:
        fx = json.load(fh)
    table, names = scoring.fold_table(fx['vocab'], fx['fold'], cuda)
    return fx, table, names


def _fold_cases(seed, B, H, R, n_vocab):
    """Labels over the whole vocabulary (dropped classes among them) with some values
    outside [0, n_fold) mixed in."""
    rng = np.random.default_rng(seed)
    hyps, refs = [], []
    for b in range(B):
        h, r = sr.case(seed * 100 + b, int(rng.integers(0, H + 1)), int(rng.integers(0, R + 1)), n_vocab)
        for seq in (h, r):
            for k in range(len(seq)):
                if rng.random() < 0.05:
                    seq[k] = int(rng.choice([-1, -5, n_vocab, n_vocab + 7, 10 ** 6]))
        hyps.append(h)
        refs.append(r)
    return hyps, refs


def test_timit_fold(cuda):
    from srf_amd import scoring
    fx, table, names = _timit(cuda)
    fold = table.cpu().tolist()
    assert len(names) == 39
    hyps, refs = _fold_cases(3, 8, 70, 75, len(fold))
    hyps[0] += [fx['vocab'].index('q'), 0, 62, -1]   # dropped class, padding symbol, outside the table
    al = scoring.edit_align(hyps, None, refs, None, fold=table)
    Hmax, Rmax = al.hyp.shape[1], al.ref.shape[1]
    want = [sr.align(h, r, fold, Hmax, Rmax) for h, r in zip(hyps, refs)]
    _assert_equal(al, want)
    h2r = al.hyp_to_ref.cpu().tolist()
    assert h2r[0][len(hyps[0]) - 4:len(hyps[0])] == [-2] * 4
    n_dropped = sum(1 for h in hyps for x in h if not 0 <= x < len(fold) or fold[x] < 0)
    assert n_dropped > 8 and sum(row.count(-2) for row in h2r) == sum(Hmax - len(h) for h in hyps) + n_dropped
    assert al.ops() == [w['ops'] for w in want]
    # ao / aa fold to one class: the pair is correct, not a substitution
    v = fx['vocab']
    pair = scoring.edit_align([[v.index('ao'), v.index('ix')]], None, [[v.index('aa'), v.index('ih')]], None, fold=table)
    assert pair.counts.cpu().tolist() == [[0, 0, 0, 0, 2, 2]]
    # a fold that drops everything: nothing to align
    none = scoring.edit_align(hyps, None, refs, None, fold=torch.full((62,), -1, dtype=torch.int32))
    assert none.counts.cpu().tolist() == [[0] * 6] * len(hyps)
    assert torch.all(none.hyp_to_ref == -2) and torch.all(none.ref_to_hyp == -2)


def test_accumulators(cuda):
    """Two updates equal the reference's sum; the confusion matrix equals the reference's
    tally with its insertion row, deletion column and skipped out-of-range pairs; a reset
    zeroes everything."""
    from srf_amd import scoring
    K = 40
    er = scoring.ErrorRate(n_classes=K, device=cuda)
    results = []
    for H, R in ((65, 63), (200, 200)):
        batch = sr.reference(H, R, 62)   # classes 40 .. 61 are outside [0, K)
        er.update_state(*_dev(batch, cuda))
        results += batch[4]
    t = sr.totals(results)
    totals, conf = er.state()
    assert totals.dtype == torch.int64 and conf.dtype == torch.int64
    assert totals.cpu().tolist() == t
    assert er.result() == sr.error_rate(t)
    want = sr.confusion(results, K)
    got = er.confusion().cpu().numpy()
    assert np.array_equal(got, want)
    n_pairs = sum(len(res['pairs']) for res in results)
    print(f'error rate {er.result()["error_rate"]:.4f}; {int(want.sum())} of {n_pairs} pairs inside [0, {K}), '
          f'{int(want[K].sum())} insertions, {int(want[:, K].sum())} deletions')
    assert got[K, K] == 0 and want[K].sum() > 0 and want[:, K].sum() > 0 and 0 < want.sum() < n_pairs
    er.reduce()   # world size 1: nothing happens
    assert er.state()[0].cpu().tolist() == t
    er.reset_states()
    assert not er.state()[0].any() and not er.state()[1].any()
    assert er.result() == sr.error_rate([0] * 8)


def test_error_rate_with_fold_and_lists(cuda):
    from srf_amd import scoring
    _, table, names = _timit(cuda)
    fold = table.cpu().tolist()
    er = scoring.ErrorRate(n_classes=len(names), fold=table, device=cuda)
    hyps, refs = _fold_cases(5, 6, 50, 50, len(fold))
    er.update_state(hyps, None, refs, None)
    results = [sr.align(h, r, fold) for h, r in zip(hyps, refs)]
    assert er.state()[0].cpu().tolist() == sr.totals(results)
    assert np.array_equal(er.confusion().cpu().numpy(), sr.confusion(results, len(names)))


@pytest.fixture(scope='module')
def mini(cuda):
    from srf_amd.sequence_router import SequenceRouter
    kw, sh, P, z, ev = load_eval_fixture('c2_mini')
    model = SequenceRouter(config_from_shape(kw), None, sh.class_n, device=cuda)
    model.load_params(P)
    inputs = (torch.tensor(z['feats'], dtype=torch.float32, device=cuda), torch.tensor(z['labels'], device=cuda),
              torch.tensor(z['inp_len'], dtype=torch.int32, device=cuda), torch.tensor(z['tar_len'], device=cuda))
    return model, sh, z, inputs


def test_valid_step_error_state(cuda, mini):
    from srf_amd import ctc, scoring, trainer_sr
    model, sh, z, inputs = mini
    blank = sh.class_n - 1
    plain = trainer_sr.process_valid_step(4, inputs, model, None, blank)
    er = scoring.ErrorRate(device=cuda)
    state = trainer_sr.Mean()
    scored = trainer_sr.process_valid_step(4, inputs, model, state, blank, error_state=er)
    assert torch.equal(plain, scored)
    with torch.no_grad():
        logits = model(inputs[0], input_lengths=inputs[2], training=False)
    hyps = ctc.greedy_decode(logits, trainer_sr.ceil_div(inputs[2], 4), blank)
    refs = [[int(v) for v in z['labels'][b][:int(z['tar_len'][b])]] for b in range(len(hyps))]
    want = sr.error_rate(sr.totals([sr.align(h, r) for h, r in zip(hyps, refs)]))
    print(f'c2_mini greedy: {er.result()}')
    assert er.result() == want
    assert want['utterances'] == len(hyps) and want['reference_labels'] == int(sum(z['tar_len']))


@pytest.mark.parametrize('kw', [dict(), dict(beam_width=4, decoder='device')], ids=['greedy', 'device-beam4'])
def test_test_step_score(cuda, mini, capsys, kw):
    from srf_amd import scoring, trainer_sr
    model, sh, z, inputs = mini
    test_inputs = (*inputs, [f'utt{b}' for b in range(inputs[0].shape[0])])
    plain = trainer_sr.process_test_step(4, test_inputs, model, **kw)
    out_plain = capsys.readouterr().out
    er = scoring.ErrorRate(device=cuda)
    scored = trainer_sr.process_test_step(4, test_inputs, model, score=er, **kw)
    assert capsys.readouterr().out == out_plain
    assert scored == plain
    refs = [[int(v) for v in z['labels'][b][:int(z['tar_len'][b])]] for b in range(len(plain))]
    assert er.result() == sr.error_rate(sr.totals([sr.align(h, r) for h, r in zip(plain, refs)]))
