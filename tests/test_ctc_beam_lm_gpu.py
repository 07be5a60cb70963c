"""CTC prefix beam search with a fused language model on the device (srf_ctc_beam_lm_*,
csrc/ctc_beam.hip) through ctc.BeamState(lm=...), ctc.beam_search_decode_device(lm=...),
StreamingRouter(lm=...) and trainer_sr.process_test_step(lm=...).

Definition of correct: the host decoder's fused result (ctc.beam_search_decode(lm=...),
pinned by tests/test_ctc_beam_lm_cpu.py against the float64 restatement and by exhaustive
search).  Labellings equal on tests/beam_ref.py's case lists with the automaton of
beam_lm_ref.case_automaton, the fused score and the accumulated bonus within
1e-4 * (1 + |value|) (both sides fp32, the bound of the unfused decoders); any chunking of
the same frames gives the same bits; a zero bonus gives the bits of the unfused search.
Each test prints its figures before it asserts."""
import numpy as np
import pytest
import torch

from srf_amd import ctc
from srf_amd.lm import FusedLM
from tests import beam_lm_ref, beam_ref
from tests.helpers import config_from_shape, load_eval_fixture

pytestmark = pytest.mark.gpu


def _tol(v):
    return 1e-4 * (1 + np.abs(v))


@pytest.fixture(scope='module')
def lms(cuda):
    cache = {}

    def get(C):
        if C not in cache:
            cache[C] = FusedLM.from_tables(*beam_lm_ref.case_automaton(C), blank=C - 1, device=cuda)
        return cache[C]
    yield get
    cache.clear()


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize('T,C,W', beam_ref.CASES)
def test_against_host_decoder(cuda, lms, T, C, W):
    """The eight seeds of a case as one batched call."""
    lm = lms(C)
    logits = torch.tensor(np.stack([beam_ref.case_logits(s, T, C) for s in beam_ref.SEEDS]), device=cuda)
    B = logits.shape[0]
    want, want_v, want_lm = ctc.beam_search_decode(logits, [T] * B, C - 1, W, lm=lm, with_lm_score=True)
    state = ctc.BeamState(B, C, C - 1, W, T, cuda, lm=lm)
    state.push(logits, [T] * B)
    hyps, v = state.best()
    lm_score = state.best_device()[3].cpu().double().numpy()
    plain, _ = ctc.beam_search_decode_device(logits, [T] * B, C - 1, W)
    print(f'T={T} C={C} W={W}: labellings equal {[h == w for h, w in zip(hyps, want)]}, differ from the unfused '
          f'{[h != p for h, p in zip(hyps, plain)]}, max score err {np.abs(v - want_v).max():.3e} '
          f'({(np.abs(v - want_v) / _tol(want_v)).max():.4f} tolerances), max lm_score err '
          f'{np.abs(lm_score - want_lm).max():.3e} ({(np.abs(lm_score - want_lm) / _tol(want_lm)).max():.4f})')
    assert hyps == want
    assert np.all(np.abs(v - want_v) <= _tol(want_v)), (v, want_v)
    assert np.all(np.abs(lm_score - want_lm) <= _tol(want_lm)), (lm_score, want_lm)
    assert hyps != plain
    again, again_v = ctc.beam_search_decode_device(logits, [T] * B, C - 1, W, lm=lm)
    assert again == hyps and np.array_equal(again_v, v)


def test_prefix_made_again_adopts_its_children(cuda, lms):
    """The 40 flat narrow-beam cases as one batch: labellings equal to the host's; one push
    and frame-by-frame pushes give the same bits."""
    T, C, W = beam_ref.READOPT_CASE
    lm = lms(C)
    logits = torch.tensor(np.stack([beam_ref.readopt_logits(s) for s in beam_ref.READOPT_SEEDS]), device=cuda)
    B = logits.shape[0]
    want, want_v, want_lm = ctc.beam_search_decode(logits, [T] * B, C - 1, W, lm=lm, with_lm_score=True)
    one = ctc.BeamState(B, C, C - 1, W, T, cuda, lm=lm)
    one.push(logits, [T] * B)
    hyps, v = one.best()
    print(f'readopt: {sum(h == w for h, w in zip(hyps, want))} of {B} labellings equal, max score err '
          f'{np.abs(v - want_v).max():.3e} ({(np.abs(v - want_v) / _tol(want_v)).max():.4f} tolerances)')
    assert hyps == want
    assert np.all(np.abs(v - want_v) <= _tol(want_v)), (v, want_v)
    s = ctc.BeamState(B, C, C - 1, W, T, cuda, lm=lm)
    for f in range(T):
        s.push(logits[:, f:f + 1], [1] * B)
    a, b = one.best_device(), s.best_device()
    assert s.best()[0] == hyps
    assert np.array_equal(_bits(a[1]), _bits(b[1])) and np.array_equal(_bits(a[2]), _bits(b[2]))
    assert np.array_equal(_bits(a[3]), _bits(b[3]))
    assert np.all(np.abs(a[3].cpu().double().numpy() - want_lm) <= _tol(want_lm))


@pytest.mark.parametrize('T,C,W', [(64, 33, 100), (50, 63, 128)])
def test_chunking_changes_nothing(cuda, lms, T, C, W):
    """Chunks of 1, 7, 0, 13 frames and the rest; utterance 1 ends at frame 20.  Labels,
    counts, fused scores and lm_score are the bits of the one-push decode."""
    lm = lms(C)
    logits = torch.tensor(np.stack([beam_ref.case_logits(s, T, C) for s in beam_ref.SEEDS]), device=cuda)
    B = logits.shape[0]
    lens = [T] * B
    lens[1] = 20
    one = ctc.BeamState(B, C, C - 1, W, T, cuda, lm=lm)
    one.push(logits, lens)
    want = [t.cpu().numpy() for t in one.best_device()]
    s = ctc.BeamState(B, C, C - 1, W, T, cuda, lm=lm)
    pos = 0
    for n in (1, 7, 0, 13, T - 21):
        s.push(logits[:, pos:pos + n], [max(0, min(ln - pos, n)) for ln in lens])
        pos += n
    assert pos == T and s.frames_pushed == T
    got = [t.cpu().numpy() for t in s.best_device()]
    assert np.array_equal(got[1], want[1]), (got[1], want[1])
    for b in range(B):
        assert np.array_equal(got[0][b, :got[1][b]], want[0][b, :want[1][b]]), b
    assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32)), (got[2], want[2])
    assert np.array_equal(got[3].view(np.uint32), want[3].view(np.uint32)), (got[3], want[3])
    host, _ = ctc.beam_search_decode(logits, lens, C - 1, W, lm=lm)
    assert host == [got[0][b, :got[1][b]].tolist() for b in range(B)]
    # a reset state decodes again from the start
    s.reset()
    assert s.frames_pushed == 0 and s.best()[0] == [[] for _ in range(B)]
    s.push(logits, lens)
    assert np.array_equal(_bits(s.best_device()[2]), want[2].view(np.uint32))


def test_zero_bonus_is_the_unfused_search_bit_for_bit(cuda):
    """All bonuses zero, any next: labels, counts and scores are the bits of the unfused
    BeamState, on the case list (two seeds) and on all-zero logits, where the key passes
    decide."""
    cases = [(T, C, W, torch.tensor(np.stack([beam_ref.case_logits(s, T, C) for s in (0, 1)]), device=cuda))
             for T, C, W in beam_ref.CASES]
    cases += [(T, C, W, torch.zeros((2, T, C), device=cuda)) for T, C, W in beam_ref.TIE_CASES]
    for T, C, W, x in cases:
        lm = FusedLM.from_tables(np.zeros((9, C), np.float32), beam_lm_ref.random_automaton(T, 9, C)[1], C - 1, cuda)
        out = []
        for model in (None, lm):
            s = ctc.BeamState(2, C, C - 1, W, T, cuda, lm=model)
            s.push(x, [T, T - 1])
            out.append(s.best_device())
        (labels, count, logp), (f_labels, f_count, f_score, f_lm) = out
        assert np.array_equal(count.cpu().numpy(), f_count.cpu().numpy()), (T, C, W)
        for b in range(2):
            n = int(count[b])
            assert torch.equal(labels[b, :n], f_labels[b, :n]), (T, C, W, b)
        assert np.array_equal(_bits(logp), _bits(f_score)), (T, C, W)
        assert np.all(f_lm.cpu().numpy() == 0)


@pytest.mark.parametrize('seed,T,C', [(0, 4, 4), (1, 5, 3), (3, 3, 5), (4, 6, 3)])
def test_full_beam_is_exact(cuda, seed, T, C):
    """Beam 128 keeps all of the at most 127 prefixes: the argmax over all labellings of
    torch's float64 CTC log probability + the bonuses of a random automaton."""
    logits = np.random.default_rng(seed).standard_normal((1, T, C)).astype(np.float32) * 2.0
    assert sum((C - 1) ** n for n in range(T + 1)) <= 127
    bonus, nxt = beam_lm_ref.random_automaton(100 + seed, 6, C)
    lm = FusedLM.from_tables(bonus, nxt, C - 1, cuda)
    x = logits[0].astype(np.float64)
    x = x - x.max(axis=-1, keepdims=True)
    best, best_v = beam_lm_ref.exhaustive(x - np.log(np.exp(x).sum(axis=-1, keepdims=True)), C - 1, bonus, nxt)
    hyps, v = ctc.beam_search_decode_device(torch.tensor(logits, device=cuda), [T], C - 1, beam_width=128, lm=lm)
    print(f'seed {seed} T={T} C={C}: {hyps[0]} score {v[0]:.6f}, exhaustive {best} {best_v:.6f}')
    assert hyps[0] == best
    assert abs(v[0] - best_v) < 1e-4


def test_ragged_lengths(cuda, lms):
    B, T, C, W = 4, 30, 8, 16
    lm = lms(C)
    logits = torch.tensor(np.random.default_rng(7).standard_normal((B, T, C)).astype(np.float32) * 3.0, device=cuda)
    lens = torch.tensor([30, 17, 1, 0])
    want, want_v, want_lm = ctc.beam_search_decode(logits, lens, C - 1, W, lm=lm, with_lm_score=True)
    s = ctc.BeamState(B, C, C - 1, W, T, cuda, lm=lm)
    s.push(logits, lens)
    hyps, v = s.best()
    lm_score = s.best_device()[3].cpu().double().numpy()
    print(f'ragged: {hyps} {v} {lm_score} against {want} {want_v} {want_lm}')
    assert hyps == want
    assert np.all(np.abs(v - want_v) <= _tol(want_v)) and np.all(np.abs(lm_score - want_lm) <= _tol(want_lm))
    assert hyps[3] == [] and v[3] == 0.0 and lm_score[3] == 0.0


def test_nbest_with_a_model(cuda, lms):
    T, C, W, N = 40, 8, 16, 10
    lm = lms(C)
    logits = torch.tensor(np.stack([beam_ref.case_logits(s, T, C) for s in range(3)]), device=cuda)
    s = ctc.BeamState(3, C, C - 1, W, T, cuda, lm=lm)
    s.push(logits, [T, T, 5])
    nb = s.nbest(N)
    labels, count, score, lm_best = s.best_device()
    assert nb.lm_score is not None and tuple(nb.lm_score.shape) == (3, N)
    lists, lm_score, logp = nb.lists(), nb.lm_score.cpu().double().numpy(), nb.log_prob.cpu().numpy()
    worst = 0.0
    for b in range(3):
        assert lists[b][0][0] == labels[b, :int(count[b])].tolist()
        assert np.array_equal(_bits(nb.log_prob[b, :1]), _bits(score[b:b + 1]))
        assert np.array_equal(_bits(nb.lm_score[b, :1]), _bits(lm_best[b:b + 1]))
        n = int(nb.count[b])
        assert n == N and np.all(np.diff(logp[b, :n]) <= 0)   # the beam holds W = 16 >= N entries
        for i, (hyp, _) in enumerate(lists[b]):
            want = beam_lm_ref.sequence_bonus(hyp, lm.bonus_host, lm.next_host)
            worst = max(worst, abs(lm_score[b, i] - want) / _tol(want))
            assert abs(lm_score[b, i] - want) <= _tol(want), (b, i, lm_score[b, i], want)
    print(f'nbest: largest lm_score error {worst:.4f} tolerances')
    assert ctc.beam_search_nbest_device(logits, [T, T, 5], C - 1, W, N, lm=lm).lists() == lists
    assert s.nbest(N).lm_score is not None and ctc.BeamState(1, C, C - 1, W, T, cuda).nbest(2).lm_score is None


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


def test_streaming_beam_with_a_model(cuda, built):
    """StreamingRouter(beam_width=8, lm=...), B = 2, lengths [96, 70], chunks of 12: the beam
    hypotheses and scores after finish() are the bits of the fused device decode of the
    offline logits; the greedy output is that of a router without a beam."""
    from srf_amd.streaming import StreamingRouter
    model, sh = built('c4_mini')[:2]
    T, lens, W, blank = 96, [96, 70], 8, sh.class_n - 1
    lm = FusedLM.from_tables(*beam_lm_ref.case_automaton(sh.class_n), blank=blank, device=cuda)
    feats = torch.tensor(np.random.default_rng(20).standard_normal((2, T, sh.feat_dim)).astype(np.float32),
                         device=cuda)
    with torch.no_grad():
        off = model(feats, input_lengths=torch.tensor(lens, device=cuda), training=False)
    routers = [StreamingRouter(model, 2, max_chunk=12, beam_width=W, lm=lm), StreamingRouter(model, 2, max_chunk=12)]
    for s in routers:
        for pos in range(0, T, 12):
            ended = [ln if pos <= ln <= pos + 12 and ln < T else -1 for ln in lens]
            s.push(feats[:, pos:pos + 12], ended)
        s.finish()
    s = routers[0]
    ceil = [(ln + 3) // 4 for ln in lens]
    want, want_v = ctc.beam_search_decode_device(off, ceil, blank, beam_width=W, lm=lm)
    plain, _ = ctc.beam_search_decode_device(off, ceil, blank, beam_width=W)
    print(f'streamed {s.beam_hypotheses} {s.beam_scores}, offline {want} {want_v}, without the model {plain}')
    assert s.beam_hypotheses == want
    assert np.array_equal(s.beam_scores, want_v)
    assert s.hypotheses == routers[1].hypotheses
    with pytest.raises(ValueError, match='beam_width'):
        StreamingRouter(model, 2, max_chunk=12, lm=lm)


def test_process_test_step_with_a_model(cuda, built, capsys):
    from srf_amd import trainer_sr
    model, sh, z, _ = built('c2_mini')
    feats = torch.tensor(z['feats'], dtype=torch.float32, device=cuda)
    inp_len = torch.tensor(z['inp_len'], dtype=torch.int32, device=cuda)
    utts = [f'utt{b}' for b in range(feats.shape[0])]
    inputs = (feats, torch.tensor(z['labels'], device=cuda), inp_len, torch.tensor(z['tar_len'], device=cuda), utts)
    blank = sh.class_n - 1
    lm = FusedLM.from_tables(*beam_lm_ref.case_automaton(sh.class_n), blank=blank, device=cuda)
    with torch.no_grad():
        y_pred = model(feats, input_lengths=inp_len, training=False)
    floor = inp_len.to(torch.int64) // 4
    dev = trainer_sr.process_test_step(4, inputs, model, beam_width=8, lm=lm, decoder='device')
    host = trainer_sr.process_test_step(4, inputs, model, beam_width=8, lm=lm, decoder='host')
    capsys.readouterr()
    print(f'device {dev}, host {host}')
    assert dev == host
    assert dev == ctc.beam_search_decode_device(y_pred, floor, blank, beam_width=8, lm=lm)[0]
    with pytest.raises(ValueError, match='beam_width'):
        trainer_sr.process_test_step(4, inputs, model, lm=lm)
    with pytest.raises(ValueError, match='beam_width'):
        trainer_sr.process_test_step(4, inputs, model, lm=lm, decoder='device')


def test_model_for_other_classes_is_refused_before_any_launch(cuda, lms):
    lm = lms(8)
    with pytest.raises(ValueError, match='classes'):
        ctc.BeamState(1, 32, 31, 4, 10, cuda, lm=lm)
    with pytest.raises(ValueError, match='classes'):
        ctc.beam_search_decode_device(torch.zeros(1, 3, 32, device=cuda), [3], 31, beam_width=4, lm=lm)
    with pytest.raises(ValueError, match='blank'):
        ctc.BeamState(1, 8, 3, 4, 10, cuda, lm=lm)
    host = FusedLM.from_tables(*beam_lm_ref.case_automaton(8), blank=7, device='cpu')
    s = ctc.BeamState(1, 8, 7, 4, 10, cuda, lm=host)
    with pytest.raises(ValueError, match='device'):   # its tables are not on the device
        s.push(torch.zeros(1, 3, 8, device=cuda), [3])
    assert s.frames_pushed == 0
