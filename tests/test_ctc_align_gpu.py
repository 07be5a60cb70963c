"""CTC forced alignment (srf_ctc_align, ctc.forced_align) and greedy label frames
(srf_ctc_greedy_frames_n, StreamOut.label_frames) on the GPU against the float64
restatement of tests/align_ref.py.

fp32 bound: align_ref.bound(T, v) = 4 T 2^-23 max(1, |v|).  The short cases have a best
path that leads every other by more than that (tests/test_ctc_align_cpu.py), so their
states must equal the reference's; the long cases' gaps lie below it, so the device path
must be a valid alignment whose float64 score is within the bound of the optimum.
Each test prints its figures before it asserts.

Observed on an MI355X: short cases, states equal on all 40, none
excused, scores within 0.015 bounds; long cases, 8 of 8 paths equal the reference's in
every case, rescoring 0.0000 bounds below the optimum, scores within 0.009 bounds."""
import math

import numpy as np
import pytest
import torch

from tests import align_ref as ar
from tests import beam_ref
from tests.helpers import config_from_shape, load_eval_fixture

pytestmark = pytest.mark.gpu


def _batch(T, C, L, dev):
    cases = [ar.case(seed, T, C, L) for seed in ar.SEEDS]
    logits = torch.tensor(np.stack([c[0] for c in cases]), device=dev)
    labels = torch.tensor(np.array([c[1] for c in cases], dtype=np.int32).reshape(len(cases), L), device=dev)
    return cases, logits, labels


def _align(logits, labels, L, T, blank):
    from srf_amd import ctc
    B = logits.shape[0]
    al = ctc.forced_align(logits, torch.full((B,), T, dtype=torch.int32), labels,
                          torch.full((B,), L, dtype=torch.int32), blank_index=blank)
    torch.cuda.synchronize()
    return (al, al.states.cpu().numpy(), al.token_start.cpu().numpy(), al.token_end.cpu().numpy(),
            al.token_logp.cpu().double().numpy(), al.score.cpu().double().numpy())


@pytest.mark.parametrize('T,C,L', ar.SHORT_CASES)
def test_short_cases_exact(cuda, T, C, L):
    cases, logits, labels = _batch(T, C, L, cuda)
    _, states, tst, ten, tlp, score = _align(logits, labels, L, T, C - 1)
    excused, worst_s, worst_l = 0, 0.0, 0.0
    for b, (x, lab, blank) in enumerate(cases):
        lp = ar.log_softmax(x)
        ref, ref_score = ar.viterbi(lp, lab, blank)
        bd = ar.bound(T, ref_score)
        if ref_score - ar.second_best(lp, lab, blank, ref) <= bd:
            excused += 1
        else:
            assert states[b].tolist() == ref, (b, states[b].tolist(), ref)
        worst_s = max(worst_s, abs(score[b] - ref_score) / bd)
        assert abs(score[b] - ref_score) <= bd, (b, score[b], ref_score)
        starts, ends = ar.spans(ref, L)
        assert tst[b].tolist() == starts and ten[b].tolist() == ends, b
        ext = ar.extended(lab, blank)
        for k in range(L):
            want = float(lp[starts[k]:ends[k], ext[2 * k + 1]].sum())
            worst_l = max(worst_l, abs(tlp[b, k] - want) / bd)
            assert abs(tlp[b, k] - want) <= bd, (b, k, tlp[b, k], want)
    print(f'(T, C, L) = {(T, C, L)}: {excused} excused, score err {worst_s:.4f} bounds, '
          f'token logp err {worst_l:.4f} bounds')
    assert excused == 0


@pytest.mark.parametrize('T,C,L', ar.LONG_CASES)
def test_long_cases_valid_and_optimal(cuda, T, C, L):
    cases, logits, labels = _batch(T, C, L, cuda)
    al, states, tst, ten, tlp, score = _align(logits, labels, L, T, C - 1)
    classes = al.classes.cpu().numpy()
    same, worst_p, worst_s = 0, 0.0, 0.0
    for b, (x, lab, blank) in enumerate(cases):
        lp = ar.log_softmax(x)
        ref, ref_score = ar.viterbi(lp, lab, blank)
        bd = ar.bound(T, ref_score)
        got = states[b].tolist()
        assert ar.is_valid_path(got, lab, blank), b
        ext = ar.extended(lab, blank)
        assert classes[b].tolist() == [int(ext[s]) for s in got]
        assert ar.collapse(classes[b].tolist(), blank) == lab
        rescored = ar.path_score(lp, lab, blank, got)
        worst_p = max(worst_p, (ref_score - rescored) / bd)
        worst_s = max(worst_s, abs(score[b] - rescored) / bd)
        assert ref_score - rescored <= bd, (b, ref_score, rescored)
        assert abs(score[b] - rescored) <= bd, (b, score[b], rescored)
        starts, ends = ar.spans(got, L)
        assert tst[b].tolist() == starts and ten[b].tolist() == ends, b
        for k in range(L):
            want = float(lp[starts[k]:ends[k], ext[2 * k + 1]].sum())
            assert abs(tlp[b, k] - want) <= bd, (b, k, tlp[b, k], want)
        same += got == ref
    print(f'(T, C, L) = {(T, C, L)}: {same} of {len(cases)} paths equal the reference; path below the optimum by '
          f'{worst_p:.4f} bounds, score off its rescoring by {worst_s:.4f} bounds')


def test_zero_logits_tie_rule(cuda):
    """The five tie cases of the CPU test as one ragged batch; sums of equal fp32 terms
    tie exactly on the device too."""
    from srf_amd import ctc
    Tmax, C = 7, 4   # the states of all-equal logits do not depend on the class count
    x = torch.zeros((len(ar.TIE_CASES), Tmax, C), device=cuda)
    lens = torch.tensor([c[0] for c in ar.TIE_CASES], dtype=torch.int32)
    al = ctc.forced_align(x, lens, [c[2] for c in ar.TIE_CASES], blank_index=C - 1)
    states, score = al.states.cpu().numpy(), al.score.cpu().numpy()
    for j, (T, _, lab, want) in enumerate(ar.TIE_CASES):
        print(f'T={T} labels={lab}: {states[j].tolist()} score {score[j]}')
        assert ar.viterbi(ar.log_softmax(np.zeros((T, C))), lab, C - 1)[0] == want
        if want is None:
            assert states[j].tolist() == [-1] * Tmax and score[j] == -math.inf
            assert al.spans()[j] == []
        else:
            assert states[j].tolist() == want + [-1] * (Tmax - T)
            assert abs(score[j] - T * -math.log(C)) <= ar.bound(T, score[j])


def test_ragged_edges_and_guards(cuda):
    """Ragged lengths down to 0, an infeasible utterance, and poisoned outputs with guard
    rows: rows beyond T_b are -1 and nothing outside [B][Tmax] / [B][Lmax] is written."""
    from srf_amd import _lib, ops
    T, C, blank, Lmax = 30, 8, 7, 10
    logit_len = [30, 17, 1, 0, 3]
    lab_len = [10, 5, 1, 0, 3]
    B = len(logit_len)
    rng = np.random.default_rng(77)
    x = (rng.standard_normal((B, T, C)) * 3).astype(np.float32)
    labs = [[int(v) for v in rng.integers(0, C - 1, n)] for n in lab_len]
    labs[4] = [1, 1, 1]   # three frames cannot hold two repeats
    dense = np.zeros((B, Lmax), dtype=np.int32)
    for b, l in enumerate(labs):
        dense[b, :len(l)] = l
    dev = dict(device=cuda)
    G = 2   # guard rows before and after
    states = torch.full((B + 2 * G, T), 12345, dtype=torch.int32, **dev)
    tst = torch.full((B + 2 * G, Lmax), 12345, dtype=torch.int32, **dev)
    ten = torch.full((B + 2 * G, Lmax), 12345, dtype=torch.int32, **dev)
    tlp = torch.full((B + 2 * G, Lmax), 12345.0, dtype=torch.float32, **dev)
    score = torch.full((B + 2 * G,), 12345.0, dtype=torch.float32, **dev)
    L = _lib.lib()
    wb = L.srf_ctc_align_workspace(B, T, C, Lmax)
    ws = torch.empty(wb, dtype=torch.uint8, **dev)
    args = [torch.tensor(x, **dev), torch.tensor(dense, **dev), torch.tensor(lab_len, dtype=torch.int32, **dev),
            torch.tensor(logit_len, dtype=torch.int32, **dev)]
    _lib.check(L.srf_ctc_align(*[ops._ptr(a) for a in args], B, T, C, Lmax, blank, ops._ptr(states[G:]),
                               ops._ptr(tst[G:]), ops._ptr(ten[G:]), ops._ptr(tlp[G:]), ops._ptr(score[G:]),
                               ops._ptr(ws), wb, ops._stream()), 'srf_ctc_align')
    torch.cuda.synchronize()
    for t in (states, tst, ten, tlp, score):
        t = t.cpu()
        assert torch.all(t[:G] == 12345) and torch.all(t[G + B:] == 12345), 'a guard row was written'
    states, tst, ten = states[G:G + B].cpu().numpy(), tst[G:G + B].cpu().numpy(), ten[G:G + B].cpu().numpy()
    tlp, score = tlp[G:G + B].cpu().double().numpy(), score[G:G + B].cpu().double().numpy()
    for b in range(B):
        Tb, Lb = logit_len[b], lab_len[b]
        lp = ar.log_softmax(x[b, :Tb])
        ref, ref_score = ar.viterbi(lp, labs[b], blank)
        print(f'utt {b}: T_b={Tb} L_b={Lb} score {score[b]} reference {ref_score}')
        if ref is None:
            assert b == 4 and score[b] == -math.inf
            assert np.all(states[b] == -1) and np.all(tst[b] == -1) and np.all(ten[b] == -1) and np.all(tlp[b] == 0)
            continue
        bd = ar.bound(max(Tb, 1), ref_score)
        if Tb > 1:   # the demand for the reference's very path rests on its lead over every other
            gap = ref_score - ar.second_best(lp, labs[b], blank, ref)
            print(f'utt {b}: gap / bound {gap / bd:.1f}')
            assert gap > bd
        assert states[b].tolist() == ref + [-1] * (T - Tb)
        assert abs(score[b] - ref_score) <= bd
        starts, ends = ar.spans(ref, Lb)
        assert tst[b].tolist() == starts + [-1] * (Lmax - Lb) and ten[b].tolist() == ends + [-1] * (Lmax - Lb)
        assert np.all(tlp[b, Lb:] == 0)
    assert score[3] == 0.0


def test_refusals(cuda):
    from srf_amd import ctc
    x = torch.zeros((1, 4, 3), device=cuda)
    with pytest.raises(ValueError, match='device tensor'):
        ctc.forced_align(x.cpu(), [4], [[0]], blank_index=2)
    with pytest.raises(ValueError, match='device tensor'):
        ctc.forced_align(x[0], [4], [[0]], blank_index=2)
    with pytest.raises(ValueError, match='blank index'):
        ctc.forced_align(x, [4], [[0]], blank_index=3)
    with pytest.raises(ValueError, match='label_lengths'):
        ctc.forced_align(x, [4], torch.zeros((1, 1), dtype=torch.int32), blank_index=2)
    assert ctc.forced_align(x, [4], [[0]], blank_index=2).spans() == [[(0, 3, 4)]]
    assert ctc.forced_align(x, [4], [[]], blank_index=2).spans() == [[]]


@pytest.mark.parametrize('T,C', [(40, 8), (60, 32), (64, 33), (50, 63)])
def test_greedy_frames_against_alignment(cuda, T, C):
    """The two halves against each other: greedy labels and frames in chunks of 7, then
    forced_align on the greedy labelling.  The arg-max path is the unique best path with
    that labelling (the gap is the smallest top-1 / top-2 margin of a frame whose change
    keeps the labelling, far above the bound), so classes are the per-frame arg-max and
    token_start the greedy frames.  srf_ctc_greedy_n returns the same labels bit for bit."""
    from srf_amd import ctc
    blank = C - 1
    x = np.stack([beam_ref.case_logits(seed, T, C) for seed in ar.SEEDS])
    B = len(x)
    logits = torch.tensor(x, device=cuda)
    prev = torch.full((B,), -1, dtype=torch.int32, device=cuda)
    prev_old = prev.clone()
    labs, frames = [[] for _ in range(B)], [[] for _ in range(B)]
    lens = torch.full((B,), T, dtype=torch.int32, device=cuda)
    for pos in range(0, T, 7):
        chunk = logits[:, pos:pos + 7].contiguous()
        n_valid = (lens - pos).clamp(0, chunk.shape[1])
        l_new, f_new, c_new = ctc.greedy_decode_frames_device(chunk, n_valid, blank, prev, pos)
        l_old, c_old = ctc.greedy_decode_device(chunk, n_valid, blank, prev_old)
        assert torch.equal(c_new, c_old) and torch.equal(prev, prev_old)
        cnt = c_new.cpu().tolist()
        l_new, f_new, l_old = l_new.cpu().tolist(), f_new.cpu().tolist(), l_old.cpu().tolist()
        for b in range(B):
            assert l_new[b][:cnt[b]] == l_old[b][:cnt[b]]
            labs[b] += l_new[b][:cnt[b]]
            frames[b] += f_new[b][:cnt[b]]
    for b in range(B):
        assert (labs[b], frames[b]) == ar.greedy_frames(x[b], T, blank), b
    al = ctc.forced_align(logits, lens, labs, blank_index=blank)
    classes, tst = al.classes.cpu().numpy(), al.token_start.cpu().numpy()
    ratios = []
    for b in range(B):
        lp = ar.log_softmax(x[b])
        ref, ref_score = ar.viterbi(lp, labs[b], blank)
        ratios.append((ref_score - ar.second_best(lp, labs[b], blank, ref)) / ar.bound(T, ref_score))
        assert classes[b].tolist() == np.argmax(x[b], axis=-1).tolist(), b
        assert tst[b, :len(labs[b])].tolist() == frames[b], b
        assert [(l, s) for l, s, _ in al.spans()[b]] == list(zip(labs[b], frames[b]))
    print(f'(T, C) = {(T, C)}: gap / bound {min(ratios):.1f} .. {max(ratios):.1f}')
    assert min(ratios) > 1.0


@pytest.fixture(scope='module')
def built(cuda):
    from srf_amd.sequence_router import SequenceRouter
    cache = {}

    def get(name):
        if name not in cache:
            kw, sh, P, z, ev = load_eval_fixture(name)
            model = SequenceRouter(config_from_shape(kw), None, sh.class_n, device=cuda)
            model.load_params(P)
            cache[name] = (model, sh, z, ev)
        return cache[name]
    yield get
    cache.clear()


def _inputs(z, dev):
    return (torch.tensor(z['feats'], dtype=torch.float32, device=dev), torch.tensor(z['labels'], device=dev),
            torch.tensor(z['inp_len'], dtype=torch.int32, device=dev), torch.tensor(z['tar_len'], device=dev))


@pytest.mark.parametrize('name', ['c4_mini', 'c3_mini_sdr'])
def test_model_end_to_end(cuda, built, name):
    """Eval-mode logits aligned with the fixture's transcript at ceil(len / 4) against
    the reference on the oracle's float64 logits.  Tolerance: the project's per-logit
    1e-4 (1 + |logit|), on the logit and on the log-sum-exp of each of T' frames; and the
    best path cannot beat the sum over all paths, -nll."""
    from srf_amd import ctc
    model, sh, z, ev = built(name)
    feats, labels, inp_len, tar_len = _inputs(z, cuda)
    blank = sh.class_n - 1
    with torch.no_grad():
        logits = model(feats, input_lengths=inp_len, training=False)
    lens = (inp_len + 3) // 4
    al = ctc.forced_align(logits, lens, labels, tar_len, blank_index=blank)
    score = al.score.cpu().double().numpy()
    ref_logits = ev['logits'].astype(np.float64)
    for b in range(feats.shape[0]):
        Tb, Lb = int(lens[b]), int(z['tar_len'][b])
        lab = [int(v) for v in z['labels'][b][:Lb]]
        ref, ref_score = ar.viterbi(ar.log_softmax(ref_logits[b, :Tb]), lab, blank)
        tol = 2 * Tb * 1e-4 * (1 + np.abs(ref_logits[b, :Tb]).max())
        print(f'{name} utt {b}: score {score[b]:.5f} reference {ref_score:.5f} -nll {-ev["nll"][b]:.5f} tol {tol:.4f}')
        assert abs(score[b] - ref_score) <= tol
        assert score[b] <= -float(ev['nll'][b]) + tol
        got = al.states[b, :Tb].cpu().tolist()
        assert ar.is_valid_path(got, lab, blank)
        assert [l for l, _, _ in al.spans()[b]] == lab


def test_process_test_step_timestamps(cuda, built, capsys):
    from srf_amd import trainer_sr
    model, sh, z, ev = built('c4_mini')
    inputs = _inputs(z, cuda)
    utts = [f'utt{b}' for b in range(inputs[0].shape[0])]
    test_inputs = (inputs[0], inputs[1], inputs[2], inputs[3], utts)
    plain = trainer_sr.process_test_step(4, test_inputs, model, beam_width=16)
    out_plain = capsys.readouterr().out
    hyps, spans = trainer_sr.process_test_step(4, test_inputs, model, beam_width=16, timestamps=True)
    assert capsys.readouterr().out == out_plain
    assert hyps == plain
    for b, (h, sp) in enumerate(zip(hyps, spans)):
        n = int(z['inp_len'][b]) // 4
        print(f'utt {b}: {sp}')
        assert [l for l, _, _ in sp] == h
        assert all(0 <= s < e <= n for _, s, e in sp)
        assert all(a[2] <= c[1] for a, c in zip(sp[:-1], sp[1:]))
    greedy, gspans = trainer_sr.process_test_step(4, test_inputs, model, timestamps=True)
    assert greedy == ev['greedy_floor'] and [[l for l, _, _ in sp] for sp in gspans] == greedy


@pytest.mark.parametrize('pattern', [[12] * 8, [32] * 3], ids=['12*8', '32*3'])
def test_streaming_label_frames(cuda, built, pattern):
    """The c4_mini session of tests/test_streaming_gpu.py (B = 2, T = 96, lengths [96,
    70]): hypothesis_frames are the frames of the host restatement over the concatenated
    streamed logits, whatever the chunking."""
    from srf_amd.streaming import StreamingRouter
    model, sh, _, _ = built('c4_mini')
    T, lens = 96, [96, 70]
    feats = torch.tensor(np.random.default_rng(20).standard_normal((2, T, sh.feat_dim)).astype(np.float32), device=cuda)
    s = StreamingRouter(model, 2, max_chunk=32)
    outs, pos, declared = [], 0, False
    for n in pattern:
        ended = [-1, -1]
        if not declared and pos <= lens[1] <= pos + n:
            ended[1], declared = lens[1], True
        outs.append(s.push(feats[:, pos:pos + n], ended))
        pos += n
    outs.append(s.finish())
    logits = torch.cat([o.logits for o in outs], dim=1).cpu().numpy()
    hyp, hyp_frames = s.hypotheses, s.hypothesis_frames
    for o in outs:
        for b in range(2):
            assert len(o.label_frames[b]) == len(o.labels[b])
            assert all(o.t0 <= f < o.t0 + o.logits.shape[1] for f in o.label_frames[b])
    for b in range(2):
        want_l, want_f = ar.greedy_frames(logits[b], (lens[b] + 3) // 4, sh.class_n - 1)
        print(f'stream {b}: {len(hyp[b])} labels at frames {hyp_frames[b]}')
        assert hyp[b] == want_l and hyp_frames[b] == want_f
        assert hyp[b] == sum((o.labels[b] for o in outs), [])
        assert hyp_frames[b] == sum((o.label_frames[b] for o in outs), [])
