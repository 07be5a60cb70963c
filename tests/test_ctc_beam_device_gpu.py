"""CTC prefix beam search on the device (srf_ctc_beam_*, csrc/ctc_beam.hip) through
ctc.beam_search_decode_device, ctc.BeamState, StreamingRouter(beam_width=...) and
trainer_sr.process_test_step(decoder='device').

Definition of correct: the host decoder's result (ctc.beam_search_decode), which is in
turn pinned by exhaustive search.  The labelling must be the host's on every case of
tests/beam_ref.py's list, on which rounding does not decide the answer
(tests/test_ctc_beam_device_cpu.py), log probabilities within 1e-4 * (1 + |logp|) (both
sides fp32, sums of at most 64 frames); any chunking of the same frames must give the
same bits.  Each test prints its figures before it asserts."""
import itertools

import numpy as np
import pytest
import torch

from srf_amd import ctc
from tests import beam_ref
from tests.helpers import config_from_shape, load_eval_fixture

pytestmark = pytest.mark.gpu


def _log_softmax(x):
    x = x - x.max(axis=-1, keepdims=True)
    return x - np.log(np.exp(x).sum(axis=-1, keepdims=True))


def _ctc_logp(logp, labels, blank):
    """log p(labels | x) by torch's float64 CTC forward (independent of the decoders)."""
    T = logp.shape[0]
    lp = torch.tensor(logp, dtype=torch.float64).unsqueeze(1)
    tgt = torch.tensor([labels if labels else [0]], dtype=torch.long)
    nll = torch.nn.functional.ctc_loss(lp, tgt, torch.tensor([T]), torch.tensor([len(labels)]), blank=blank,
                                       reduction='none', zero_infinity=False)
    return -float(nll[0])


def _batch(T, C, dev):
    x = np.stack([beam_ref.case_logits(seed, T, C) for seed in beam_ref.SEEDS])
    return torch.tensor(x, device=dev)


@pytest.mark.parametrize('seed,T,C', [(0, 4, 4), (1, 5, 3), (3, 3, 5), (4, 6, 3)])
def test_full_beam_is_exact_map_labelling(cuda, seed, T, C):
    """At most 127 prefixes exist, so a beam of 128 keeps them all and the search is
    exact: the result is the labelling of maximum CTC probability among all labellings,
    each scored by torch's float64 CTC forward."""
    logits = np.random.default_rng(seed).standard_normal((1, T, C)).astype(np.float32) * 2.0
    blank = C - 1
    assert sum((C - 1) ** n for n in range(T + 1)) <= 127
    lp = _log_softmax(logits[0].astype(np.float64))
    best, best_lp = None, -np.inf
    for n in range(T + 1):
        for lab in itertools.product(range(C - 1), repeat=n):
            v = _ctc_logp(lp, list(lab), blank)
            if v > best_lp:
                best, best_lp = list(lab), v
    hyps, logp = ctc.beam_search_decode_device(torch.tensor(logits, device=cuda), [T], blank, beam_width=128)
    print(f'seed {seed} T={T} C={C}: {hyps[0]} logp {logp[0]:.6f}, exhaustive {best} {best_lp:.6f}')
    assert hyps[0] == best
    assert abs(logp[0] - best_lp) < 1e-4


@pytest.mark.parametrize('T,C,W', beam_ref.CASES)
def test_against_host_decoder(cuda, T, C, W):
    """The eight seeds of a case as one batched call."""
    logits = _batch(T, C, cuda)
    lens = [T] * logits.shape[0]
    want, want_lp = ctc.beam_search_decode(logits, lens, C - 1, beam_width=W)
    hyps, logp = ctc.beam_search_decode_device(logits, lens, C - 1, beam_width=W)
    err = np.abs(logp - want_lp) / (1e-4 * (1 + np.abs(want_lp)))
    print(f'T={T} C={C} W={W}: labellings equal {[h == w for h, w in zip(hyps, want)]}, '
          f'max logp err {np.abs(logp - want_lp).max():.3e} ({err.max():.4f} tolerances)')
    assert hyps == want
    assert np.all(err <= 1.0), (logp, want_lp)


def test_prefix_made_again_adopts_its_children(cuda):
    """tests/beam_ref.py's flat narrow-beam cases, all seeds as one batch: a prefix that
    left the beam while a child stayed is made again and must merge with that child as
    in the host decoder (which gives the re-made prefix its old node back).  Labellings
    equal the host's; log probabilities within 1e-4 * (1 + |logp|).  One push and
    frame-by-frame pushes give the same bits."""
    T, C, W = beam_ref.READOPT_CASE
    logits = torch.tensor(np.stack([beam_ref.readopt_logits(s) for s in beam_ref.READOPT_SEEDS]), device=cuda)
    B = logits.shape[0]
    want, want_lp = ctc.beam_search_decode(logits, [T] * B, C - 1, beam_width=W)
    hyps, logp = ctc.beam_search_decode_device(logits, [T] * B, C - 1, beam_width=W)
    err = np.abs(logp - want_lp) / (1e-4 * (1 + np.abs(want_lp)))
    print(f'readopt: {sum(h == w for h, w in zip(hyps, want))} of {B} labellings equal, '
          f'max logp err {np.abs(logp - want_lp).max():.3e} ({err.max():.4f} tolerances)')
    assert hyps == want
    assert np.all(err <= 1.0), (logp, want_lp)
    s = ctc.BeamState(B, C, C - 1, W, T, cuda)
    for f in range(T):
        s.push(logits[:, f:f + 1], [1] * B)
    step, step_lp = s.best()
    assert step == hyps and np.array_equal(step_lp, logp)


def test_ragged_lengths(cuda):
    B, T, C, W = 4, 30, 8, 16
    logits = torch.tensor(np.random.default_rng(7).standard_normal((B, T, C)).astype(np.float32) * 3.0, device=cuda)
    lens = torch.tensor([30, 17, 1, 0])
    want, want_lp = ctc.beam_search_decode(logits, lens, C - 1, beam_width=W)
    hyps, logp = ctc.beam_search_decode_device(logits, lens, C - 1, beam_width=W)
    print(f'ragged: {hyps} {logp} against {want} {want_lp}')
    assert hyps == want
    assert np.all(np.abs(logp - want_lp) <= 1e-4 * (1 + np.abs(want_lp)))
    assert hyps[3] == [] and logp[3] == 0.0


def test_ties_go_to_the_earlier_created(cuda):
    """All-zero logits: the totals of sibling extensions are equal bit for bit and
    straddle the edge of the beam, so the key decides (the select's two passes over it).
    The host decoder's labelling on every case (tests/test_ctc_beam_device_cpu.py shows
    that its float64 restatement agrees)."""
    for T, C, W in beam_ref.TIE_CASES:
        x = torch.zeros((2, T, C), device=cuda)
        want, want_lp = ctc.beam_search_decode(x, [T, T - 1], C - 1, beam_width=W)
        hyps, logp = ctc.beam_search_decode_device(x, [T, T - 1], C - 1, beam_width=W)
        print(f'ties T={T} C={C} W={W}: {hyps} {logp} against {want} {want_lp}')
        assert hyps == want
        assert np.all(np.abs(logp - want_lp) <= 1e-4 * (1 + np.abs(want_lp)))


@pytest.mark.parametrize('T,C,W', [(64, 33, 100), (50, 63, 128)])
def test_chunking_changes_nothing(cuda, T, C, W):
    """Chunks of 1, 7, 0, 13 frames and the rest, best() after each; utterance 1 ends at
    frame 20 (n_valid 0 from there on).  Labels, counts and scores are the bits of the
    one-push decode of the same frames."""
    logits = _batch(T, C, cuda)
    B = logits.shape[0]
    lens = [T] * B
    lens[1] = 20
    one = ctc.BeamState(B, C, C - 1, W, T, cuda)
    one.push(logits, lens)
    want = [t.cpu().numpy() for t in one.best_device()]
    s = ctc.BeamState(B, C, C - 1, W, T, cuda)
    pos = 0
    for n in (1, 7, 0, 13, T - 21):
        s.push(logits[:, pos:pos + n], [max(0, min(ln - pos, n)) for ln in lens])
        pos += n
        mid = s.best()
        assert all(len(h) <= min(pos, ln) for h, ln in zip(mid[0], lens))
    assert pos == T and s.frames_pushed == T
    got = [t.cpu().numpy() for t in s.best_device()]
    assert np.array_equal(got[1], want[1]), (got[1], want[1])
    for b in range(B):
        assert np.array_equal(got[0][b, :got[1][b]], want[0][b, :want[1][b]]), b
    assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32)), (got[2], want[2])
    # and the one-push decode is the decoder's: the same call as beam_search_decode_device
    hyps, logp = ctc.beam_search_decode_device(logits, lens, C - 1, beam_width=W)
    assert hyps == [got[0][b, :got[1][b]].tolist() for b in range(B)]
    assert np.array_equal(logp, got[2].astype(np.float64))
    # a reset state decodes again from the start
    s.reset()
    assert s.frames_pushed == 0 and s.best()[0] == [[] for _ in range(B)]
    s.push(logits, lens)
    assert np.array_equal(s.best_device()[2].cpu().numpy().view(np.uint32), want[2].view(np.uint32))


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


@pytest.mark.parametrize('name', ['c3_mini_sdr', 'c4_mini'])
def test_streaming_beam(cuda, built, name):
    """StreamingRouter(beam_width=8), B = 2, T = 96, lengths [96, 70], chunks of 12: the
    beam hypotheses after finish() are the bits of the device decode of the offline
    logits at ceil(len / 4); each is at least as likely (float64 CTC) as the host
    decoder's hypothesis, less 1e-4; the greedy output is that of a router without a beam."""
    from srf_amd.streaming import StreamingRouter
    model, sh = built(name)[:2]
    T, lens, W, blank = 96, [96, 70], 8, sh.class_n - 1
    feats = torch.tensor(np.random.default_rng(20).standard_normal((2, T, sh.feat_dim)).astype(np.float32),
                         device=cuda)
    with torch.no_grad():
        off = model(feats, input_lengths=torch.tensor(lens, device=cuda), training=False)
    routers = [StreamingRouter(model, 2, max_chunk=12, beam_width=W), StreamingRouter(model, 2, max_chunk=12)]
    for s in routers:
        for pos in range(0, T, 12):
            ended = [ln if pos <= ln <= pos + 12 and ln < T else -1 for ln in lens]
            s.push(feats[:, pos:pos + 12], ended)
        s.finish()
    s = routers[0]
    ceil = [(ln + 3) // 4 for ln in lens]
    want, want_lp = ctc.beam_search_decode_device(off, ceil, blank, beam_width=W)
    print(f'{name}: streamed {s.beam_hypotheses} {s.beam_scores}, offline {want} {want_lp}')
    assert s.beam_hypotheses == want
    assert np.array_equal(s.beam_scores, want_lp)
    host, _ = ctc.beam_search_decode(off, ceil, blank, beam_width=W)
    for b in range(2):
        lp = _log_softmax(off[b, :ceil[b]].cpu().double().numpy())
        dev_lp, host_lp = _ctc_logp(lp, want[b], blank), _ctc_logp(lp, host[b], blank)
        print(f'{name} stream {b}: log p(device hypothesis) {dev_lp:.6f}, log p(host hypothesis) {host_lp:.6f}')
        assert dev_lp >= host_lp - 1e-4
    assert s.hypotheses == routers[1].hypotheses
    with pytest.raises(ValueError, match='beam_width'):
        routers[1].beam_hypotheses
    s.reset()
    assert s.beam_hypotheses == [[], []] and list(s.beam_scores) == [0.0, 0.0]


def test_streaming_beam_refuses_beyond_max_frames_before_advancing(cuda, built):
    """max_frames = 4 output frames, chunks of 12 input frames (lookahead 2 + L * rpad):
    the step that would emit a fifth frame raises before anything advances, so the router's
    frame count and both hypotheses are what they were."""
    from srf_amd.streaming import StreamingRouter, frames_final
    model, sh = built('c4_mini')[:2]
    feats = torch.tensor(np.random.default_rng(20).standard_normal((2, 96, sh.feat_dim)).astype(np.float32),
                         device=cuda)
    s = StreamingRouter(model, 2, max_chunk=12, beam_width=8, max_frames=4)
    pos = 0
    while frames_final(pos + 12, s.L, s.rpad)[-1] <= 4 and pos + 12 < 96:
        s.push(feats[:, pos:pos + 12])
        pos += 12
    assert 0 < pos < 96
    greedy, beam, scores = s.hypotheses, s.beam_hypotheses, s.beam_scores
    with pytest.raises(ValueError, match='max_frames'):
        s.push(feats[:, pos:pos + 12], [pos + 4, -1])
    with pytest.raises(ValueError, match='max_frames'):
        s.finish()
    assert s._pushed == pos and s._lengths == [None, None] and not s._finished
    assert s.hypotheses == greedy and s.beam_hypotheses == beam and np.array_equal(s.beam_scores, scores)
    assert s._beam.frames_pushed == frames_final(pos, s.L, s.rpad)[-1]


def test_process_test_step_device_decoder(cuda, built, capsys):
    from srf_amd import trainer_sr
    model, sh, z, _ = built('c2_mini')
    feats = torch.tensor(z['feats'], dtype=torch.float32, device=cuda)
    inp_len = torch.tensor(z['inp_len'], dtype=torch.int32, device=cuda)
    utts = [f'utt{b}' for b in range(feats.shape[0])]
    inputs = (feats, torch.tensor(z['labels'], device=cuda), inp_len, torch.tensor(z['tar_len'], device=cuda), utts)
    with torch.no_grad():
        y_pred = model(feats, input_lengths=inp_len, training=False)
    floor, blank = inp_len.to(torch.int64) // 4, sh.class_n - 1
    got = trainer_sr.process_test_step(4, inputs, model, beam_width=16, decoder='device')
    assert got == ctc.beam_search_decode_device(y_pred, floor, blank, beam_width=16)[0]
    assert trainer_sr.process_test_step(4, inputs, model, beam_width=16) == \
        ctc.beam_search_decode(y_pred, floor, blank, beam_width=16)[0]
    capsys.readouterr()
    with pytest.raises(ValueError, match='decoder'):
        trainer_sr.process_test_step(4, inputs, model, beam_width=16, decoder='gpu')


def test_refusals(cuda):
    """Outside the supported range every entry raises with a message before anything is
    launched; a refused push leaves the state and its frame count as they were."""
    from srf_amd import _lib, ops
    with pytest.raises(ValueError, match='beam width'):
        ctc.beam_search_decode_device(torch.zeros(1, 3, 8, device=cuda), [3], 7, beam_width=129)
    with pytest.raises(ValueError, match='classes'):
        ctc.beam_search_decode_device(torch.zeros(1, 3, 129, device=cuda), [3], 128, beam_width=100)
    with pytest.raises(ValueError, match='blank'):
        ctc.beam_search_decode_device(torch.zeros(1, 3, 8, device=cuda), [3], 8, beam_width=4)
    with pytest.raises(ValueError, match='blank'):
        ctc.BeamState(1, 8, -1, 4, 10, cuda)
    with pytest.raises(_lib.SrfError, match='beam_width'):
        ops.ctc_beam_state_bytes(1, 8, 129, 10)
    s = ctc.BeamState(2, 8, 7, 4, 10, cuda)
    x = torch.tensor(np.random.default_rng(0).standard_normal((2, 8, 8)).astype(np.float32), device=cuda)
    n_valid = torch.full((2,), 8, device=cuda, dtype=torch.int32)
    s.push(x, n_valid)
    before = s.best()
    with pytest.raises(_lib.SrfError, match='max_frames'):   # 8 + 8 > 10
        s.push(x, n_valid)
    assert s.frames_pushed == 8
    with pytest.raises(_lib.SrfError, match='state block'):
        ops.ctc_beam_push(s._state[:-4], s.shape, s._pushed, x[:, :1].contiguous(), n_valid, 7)
    with pytest.raises(_lib.SrfError, match='state block'):
        ops.ctc_beam_best(s._state[:-4], s.shape)
    with pytest.raises(_lib.SrfError, match='blank'):
        ops.ctc_beam_push(s._state, s.shape, s._pushed, x[:, :1].contiguous(), n_valid, 8)
    assert s.frames_pushed == 8
    after = s.best()
    assert after[0] == before[0] and np.array_equal(after[1], before[1])
    s.push(x[:, :2].contiguous(), n_valid)   # 8 + 2 = max_frames is still legal
    assert s.frames_pushed == 10
