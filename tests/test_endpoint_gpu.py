"""Endpointing on the GPU (csrc/endpoint.hip, srf_ctc_beam_cut in csrc/ctc_beam.hip) through
endpoint.endpoints / Endpointer, ctc.BeamState(segmented=True).push_cut and
StreamingRouter(endpoint=...).

Definition of correct: the cuts are those of the float64 restatement tests/endpoint_ref.py,
exactly -- everything after the two flags per frame is integer, and tests/test_endpoint_cpu.py
asserts that no flag of these inputs lies within 1e-4 of its threshold, a hundred times an
fp32 log-softmax's error.  A closed segment's beam hypothesis, count, score and lm_score are
the bits of the device beam search run on the segment's frames alone.  Chunking changes
nothing.  Each test prints its figures before it asserts."""
import numpy as np
import pytest
import torch

from srf_amd import _lib, ctc, endpoint
from srf_amd.lm import FusedLM
from tests import beam_lm_ref
from tests import endpoint_ref as R
from tests.helpers import config_from_shape, load_eval_fixture, load_model_fixture

pytestmark = pytest.mark.gpu

RULES = endpoint.EndpointRules(*R.RULES)
LENGTHS = [[R.T] * 4, [R.T, 97, 1, 0]]


@pytest.fixture(scope='module')
def inputs(cuda):
    """inputs[C] -> (host [4, T, C] float32, the same on the device); left unchanged."""
    host = {C: R.batch(C) for C in R.WIDTHS}
    return {C: (x, torch.tensor(x, device=cuda)) for C, x in host.items()}


def _oracle(x, lens, rules=R.RULES):
    return [R.cuts(x[b, :ln], x.shape[2] - 1, rules) for b, ln in enumerate(lens)]


@pytest.mark.parametrize('lens', LENGTHS, ids=['full', 'ragged'])
@pytest.mark.parametrize('C', R.WIDTHS)
def test_kernel_against_oracle(inputs, C, lens):
    x, xd = inputs[C]
    want = _oracle(x, lens)
    cuts = endpoint.endpoints(xd, torch.tensor(lens), C - 1, RULES)
    start, end, reason, n_cuts = cuts
    got = cuts.lists()
    print(f'C={C} lens={lens}: {[len(w) for w in want]} cuts, reasons '
          f'{sorted({r for w in want for _, _, r in w})}, equal {[g == w for g, w in zip(got, want)]}')
    assert tuple(start.shape) == (4, R.T // 5 + 1) and start.dtype == torch.int32
    assert got == want
    assert n_cuts.tolist() == [len(w) for w in want]
    for b, w in enumerate(want):   # -1 past the count
        for t in (start, end, reason):
            assert (t[b, len(w):] == -1).all()


@pytest.mark.parametrize('C', R.WIDTHS)
def test_chunking_changes_nothing(cuda, inputs, C):
    """Chunks of 1, 3, 5, 4 and then 5 frames, none longer than the smallest count, so one
    cut per call suffices; ragged lengths."""
    x, xd = inputs[C]
    lens = LENGTHS[1]
    one = endpoint.endpoints(xd, torch.tensor(lens), C - 1, RULES).lists()
    ep = endpoint.Endpointer(RULES, 4, C, C - 1, cuda)
    got, pos = [[] for _ in range(4)], 0
    chunks = [1, 3, 5, 4] + [5] * ((R.T - 13 + 4) // 5)
    for n in chunks:
        cuts = ep.push(xd[:, pos:pos + n], [max(0, min(ln - pos, n)) for ln in lens], max_cuts=1)
        assert cuts.n_cuts.max().item() <= 1
        for b, c in enumerate(cuts.lists()):
            got[b] += c
        pos += n
    assert pos >= R.T
    assert got == one == _oracle(x, lens)
    # reset() starts over
    ep.reset()
    again = ep.push(xd, lens, max_cuts=R.T // 5 + 1).lists()
    assert again == one


def test_more_cuts_than_room(cuda, inputs):
    """30 frames of silence hold two cuts under silence_only = 12: with max_cuts = 1 the
    first is stored, n_cuts says 2, and the state has run to the end of the chunk."""
    x, xd = inputs[8]
    want = R.ANCHORS[(8, 2)]
    ep = endpoint.Endpointer(RULES, 1, 8, 7, cuda)
    cuts = ep.push(xd[2:3, :30], [30], max_cuts=1)
    assert cuts.n_cuts.tolist() == [2] and cuts.lists() == [want[:1]]
    assert tuple(cuts.start.shape) == (1, 1)
    rest = ep.push(xd[2:3, 30:], [R.T - 30], max_cuts=16)
    assert rest.lists() == [want[2:]]
    empty = ep.push(xd[2:3, :0], [0])   # n = 0 launches nothing
    assert empty.n_cuts.tolist() == [0] and empty.end.tolist() == [[-1]]


def test_many_tiles_and_wide_rows(cuda):
    """More frames than the kernel keeps flags for at once (512) and more classes than two
    per lane: T = 1100, C = 200, three streams of different lengths."""
    T, C = 1100, 200
    g = np.random.default_rng(5)
    x = g.standard_normal((3, T, C))
    blank = C - 1
    x[:, :, blank] += 9.0 * (g.random((3, T)) < np.array([0.7, 0.3, 0.7])[:, None])
    spoken = g.integers(0, blank, (3, T))
    x[np.arange(3)[:, None], np.arange(T)[None, :], spoken] += 11.0 * (g.random((3, T)) < 0.3)
    x = x.astype(np.float32)
    rules = (7, 3, 25, 0.5)
    lens = [T, 513, 512]
    worst = min(R.margin(x[b, :ln], blank, rules[3]) for b, ln in enumerate(lens))
    want = _oracle(x, lens, rules)
    got = endpoint.endpoints(torch.tensor(x, device=cuda), lens, blank, endpoint.EndpointRules(*rules)).lists()
    print(f'T={T} C={C}: margin {worst:.3g}, {[len(w) for w in want]} cuts, reasons '
          f'{sorted({r for w in want for _, _, r in w})}')
    assert worst > 1e-4
    assert {r for w in want for _, _, r in w} == {1, 2, 3}
    assert got == want


# ---------------------------------------------------------------------------
# the beam, segmented

def _decode_slices(xd, slices, blank, W, lm):
    """The device beam search on every slice (b, start, end) of xd alone, as one batch:
    (label lists, count, score bits, lm_score bits or None)."""
    n = len(slices)
    Tm = max(e - s + 1 for _, s, e in slices)
    batch = xd.new_zeros((n, Tm, xd.shape[2]))
    for i, (b, s, e) in enumerate(slices):
        batch[i, :e - s + 1] = xd[b, s:e + 1]
    lens = [e - s + 1 for _, s, e in slices]
    state = ctc.BeamState(n, xd.shape[2], blank, W, Tm, xd.device, lm=lm)
    state.push(batch, lens)
    out = state.best_device()
    count = out[1].cpu().tolist()
    labels = [out[0][i, :count[i]].cpu().tolist() for i in range(n)]
    hyps, v = ctc.beam_search_decode_device(batch, lens, blank, W, lm=lm)   # the public call gives the same
    assert hyps == labels and np.array_equal(v, out[2].cpu().double().numpy())
    return labels, count, _bits(out[2]), (_bits(out[3]) if lm is not None else None)


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _drive(state, xd, lens, cuts_of, chunk, max_len=None):
    """push_cut in chunks of ``chunk`` frames with the cuts of cuts_of(pos, n) -> [B] chunk
    frames or -1.  Returns per utterance the closed segments' (labels, count, score bits,
    lm_score bits or None) in order."""
    B, T = xd.shape[0], xd.shape[1]
    closed = [[] for _ in range(B)]
    for pos in range(0, T, chunk):
        n = min(chunk, T - pos)
        cut = cuts_of(pos, n)
        out = state.push_cut(xd[:, pos:pos + n], [max(0, min(ln - pos, n)) for ln in lens], cut, max_len=max_len)
        count = out[1].cpu().tolist()
        for b in range(B):
            assert (count[b] >= 0) == (cut[b] >= 0), (pos, b, count[b], cut[b])
            if cut[b] >= 0:
                closed[b].append((out[0][b, :count[b]].cpu().tolist(), count[b], _bits(out[2])[b],
                                  None if out[3] is None else _bits(out[3])[b]))
    return closed


def _cuts_from(want):
    def cuts_of(pos, n):
        cut = [-1] * len(want)
        for b, w in enumerate(want):
            hit = [e - pos for _, e, _ in w if pos <= e < pos + n]
            assert len(hit) <= 1
            if hit:
                cut[b] = hit[0]
        return cut
    return cuts_of


@pytest.mark.parametrize('lens', [[R.T, 97, R.T, R.T], LENGTHS[1]], ids=['long', 'ragged'])
@pytest.mark.parametrize('fused', [False, True], ids=['plain', 'lm'])
@pytest.mark.parametrize('C,W', [(8, 4), (33, 100)])
def test_beam_segments_equal_decodes_of_their_slices(cuda, inputs, C, W, fused, lens):
    """push_cut driven by the oracle's cuts in chunks of 5: every closed segment is, bit for
    bit, the decode of its frames alone; best() afterwards is the decode of the open
    remainder."""
    x, xd = inputs[C]
    blank = C - 1
    lm = FusedLM.from_tables(*beam_lm_ref.case_automaton(C), blank=blank, device=cuda) if fused else None
    want = _oracle(x, lens)
    state = ctc.BeamState(4, C, blank, W, 64, cuda, lm=lm, segmented=True)
    closed = _drive(state, xd, lens, _cuts_from(want), 5)
    slices = [(b, s, e) for b, w in enumerate(want) for s, e, _ in w]
    tails = [(b, (want[b][-1][1] + 1 if want[b] else 0), lens[b] - 1) for b in range(4)]
    tails = [t for t in tails if t[2] >= t[1]]   # (utterance 3 is empty; a cut on a last frame leaves nothing open)
    assert {1, 2} <= {t[0] for t in tails}
    labels, count, score, lm_score = _decode_slices(xd, slices + tails, blank, W, lm)
    got = [seg for b in range(4) for seg in closed[b]]
    assert len(got) == len(slices) and state.frames_pushed == 0
    print(f'C={C} W={W} fused={fused}: {len(slices)} segments, lengths {[c for c in count[:len(slices)]]}, '
          f'{sum(g[0] == l for g, l in zip(got, labels))} labellings equal')
    assert any(c > 0 for c in count)
    for i, g in enumerate(got):
        assert g[0] == labels[i] and g[1] == count[i], (slices[i], g[0], labels[i])
        assert g[2] == score[i], (slices[i], g[2], score[i])
        assert (g[3] == lm_score[i]) if fused else g[3] is None
    out = state.best_device()
    open_count = out[1].cpu().tolist()
    for i, (b, s, e) in enumerate(tails, start=len(slices)):
        assert out[0][b, :open_count[b]].cpu().tolist() == labels[i] and open_count[b] == count[i], (b, s, e)
        assert _bits(out[2])[b] == score[i]
        if fused:
            assert _bits(out[3])[b] == lm_score[i]
    for b in set(range(4)) - {t[0] for t in tails}:   # nothing open: the reset state
        assert open_count[b] == 0 and out[2][b].item() == 0.0


def test_cut_puts_one_utterance_back_to_the_reset_state(cuda, inputs):
    """After a cut the utterance's header and beam entry 0 are the words a reset leaves;
    its neighbour's block is untouched."""
    x, xd = inputs[8]
    for lm in (None, FusedLM.from_tables(*beam_lm_ref.case_automaton(8), blank=7, device=cuda)):
        s = ctc.BeamState(2, 8, 7, 4, 20, cuda, lm=lm, segmented=True)
        fresh = s._state.clone().view(2, -1)
        s.push(xd[:2, :9], [9, 9])
        before = s._state.clone().view(2, -1)
        out = s.push_cut(xd[:2, 9:12], [3, 3], [2, -1], max_len=3)
        after = s._state.view(2, -1)
        W, fields = 4, 9 if lm is None else 11
        words = after[0].view(torch.int32)
        want = fresh[0].view(torch.int32)
        head = list(range(4)) + [4 + f * W for f in range(fields)]   # the header and entry 0 of every beam array
        assert words[head].tolist() == want[head].tolist()
        base = 4 + fields * W
        cap = 1 + 20 * W
        assert words[base].item() == -1 and words[base + cap].item() == -1   # the root's parent and label
        assert out[1].tolist()[1] == -1 and out[1].tolist()[0] >= 0
        # the neighbour took 3 more frames: the header and the result of a state that pushed 12 at once
        ref = ctc.BeamState(2, 8, 7, 4, 20, cuda, lm=lm)
        ref.push(xd[:2, :12], [12, 12])
        assert after[1].view(torch.int32)[:3].tolist() == ref._state.view(2, -1)[1].view(torch.int32)[:3].tolist()
        assert after[1].view(torch.int32)[2].item() == 12 and not torch.equal(after[1], before[1])
        a, r = s.best_device(), ref.best_device()
        n = int(r[1][1])
        assert n > 0 and int(a[1][1]) == n and torch.equal(a[0][1, :n], r[0][1, :n])
        assert _bits(a[2])[1] == _bits(r[2])[1]
        # labels beyond max_len are dropped, count stays the true length
        long = ctc.BeamState(1, 8, 7, 4, 40, cuda, lm=lm, segmented=True)
        full = long.push_cut(xd[:1, :30], [30], [29])
        long.push(xd[:1, :30], [30])
        short = long.push_cut(xd[:1, :0], [0], [0], max_len=2)   # closes what was pushed, stores two labels
        n = full[1].item()
        assert n > 2 and short[1].item() == n and short[0][0].tolist() == full[0][0, :2].tolist()


def test_forced_cut_bounds_the_trie(cuda, inputs):
    """max_frames = 45 and 320 frames, seven times that: plan 1 twice.  The device
    endpointer's forced cut every 40 frames keeps push_cut within the trie; every segment
    is the decode of its slice.  A plain state of the same size still refuses frame 46."""
    x, xd = inputs[8]
    x2, xd2 = np.concatenate([x[1:2], x[1:2]], axis=1), torch.cat([xd[1:2], xd[1:2]], dim=1)
    want = _oracle(x2, [2 * R.T])
    assert want == [[(40 * k, 40 * k + 39, 3) for k in range(8)]]
    W = 4
    ep = endpoint.Endpointer(RULES, 1, 8, 7, cuda)
    state = ctc.BeamState(1, 8, 7, W, 45, cuda, segmented=True)
    closed, bounds = [], []
    for pos in range(0, 2 * R.T, 5):
        cuts = ep.push(xd2[:, pos:pos + 5], [5], max_cuts=1)
        out = state.push_cut(xd2[:, pos:pos + 5], [5], (cuts.end[:, 0] - pos).clamp(min=-1))   # no host read
        closed.append(out)
        bounds.append(cuts)
    got_bounds = [c for cuts in bounds for c in cuts.lists()[0]]
    assert got_bounds == want[0]
    labels, count, score, _ = _decode_slices(xd2, [(0, s, e) for s, e, _ in want[0]], 7, W, None)
    got = [(o[0][0, :o[1].item()].tolist(), o[1].item(), _bits(o[2])[0]) for o in closed if o[1].item() >= 0]
    print(f'{len(got)} segments of 40 frames through a trie of 45: lengths {[g[1] for g in got]}')
    assert len(got) == 8
    for i, g in enumerate(got):
        assert g[0] == labels[i] and g[1] == count[i] and g[2] == score[i], i
    assert state.best()[0] == [[]]   # the last frame closed the last segment
    plain = ctc.BeamState(1, 8, 7, W, 45, cuda)
    plain.push(xd2[:, :45], [45])
    with pytest.raises(_lib.SrfError, match='max_frames'):
        plain.push(xd2[:, 45:46], [1])
    assert plain.frames_pushed == 45


# ---------------------------------------------------------------------------
# the router

@pytest.fixture(scope='module')
def built(cuda):
    from srf_amd.sequence_router import SequenceRouter
    cache = {}

    def get(name, evaluation=True):
        if name not in cache:
            if evaluation:
                kw, sh, P = load_eval_fixture(name)[:3]
            else:
                kw, sh, P = load_model_fixture(name)[:3]
            model = SequenceRouter(config_from_shape(kw), None, sh.class_n, device=cuda)
            model.load_params(P)
            cache[name] = (model, sh)
        return cache[name]
    yield get
    cache.clear()


ROUTER_LENS = [400, 330]
ROUTER_COUNTS = (16, 6, 30)


def _choose_threshold(off, out_lens, blank):
    """The first blank threshold of 0.005, 0.010, ... under which the float64 oracle closes, on
    these logits, a segment for reason 2 and one for reason 3, with every flag decided
    beyond rounding.  None if there is none."""
    for thr in np.arange(1, 200) * 0.005:
        rules = ROUTER_COUNTS + (float(thr),)
        cuts = [R.cuts(off[b, :ln], blank, rules) for b, ln in enumerate(out_lens)]
        reasons = {r for c in cuts for _, _, r in c}
        if {2, 3} <= reasons and min(R.margin(off[b, :ln], blank, thr) for b, ln in enumerate(out_lens)) > 1e-4:
            return float(thr), cuts
    return None


@pytest.mark.parametrize('name', ['c3_mini_sdr', 'c4_mini'])
def test_router_segments(cuda, built, name):
    """B = 2, 400 and 330 input frames in chunks of 12, beam 8, counts (16, 6, 30): the
    segments are the oracle's on the offline logits, their beam results the decodes of the
    offline slices, and everything else what a router without an endpointer gives."""
    from srf_amd.streaming import StreamingRouter
    model, sh = built(name)
    T, lens, W, blank = ROUTER_LENS[0], ROUTER_LENS, 8, sh.class_n - 1
    out_lens = [(ln + 3) // 4 for ln in lens]
    feats = torch.tensor(np.random.default_rng(30).standard_normal((2, T, sh.feat_dim)).astype(np.float32),
                         device=cuda)
    with torch.no_grad():
        off = model(feats, input_lengths=torch.tensor(lens, device=cuda), training=False)
    chosen = _choose_threshold(off.cpu().double().numpy(), out_lens, blank)
    print(f'{name}: threshold and oracle cuts {chosen}')
    assert chosen is not None, 'no threshold gives a reason-2 and a reason-3 cut with decided flags'
    thr, want = chosen
    rules = endpoint.EndpointRules(*ROUTER_COUNTS, blank_threshold=thr)
    s = StreamingRouter(model, 2, max_chunk=12, beam_width=W, endpoint=rules)
    plain = StreamingRouter(model, 2, max_chunk=12, beam_width=W)
    assert s.lookahead == 6
    logits = []
    for r in (s, plain):
        outs = []
        for pos in range(0, T, 12):
            n = min(12, T - pos)
            ended = [ln if pos <= ln <= pos + n and ln < T else -1 for ln in lens]
            outs.append(r.push(feats[:, pos:pos + n], ended))
        outs.append(r.finish())
        logits.append(torch.cat([o.logits for o in outs], dim=1))
        if r is s:
            per_step = [sum((o.segments[b] for o in outs), []) for b in range(2)]
    segs = s.segments
    assert per_step == segs
    for b in range(2):
        assert want[b][-1][1] < out_lens[b] - 1   # the oracle leaves a remainder open (else no reason-0 segment)
    full = [w + [(w[-1][1] + 1, out_lens[b] - 1, 0)] for b, w in enumerate(want)]
    print(f'{name}: segments {[[(g.start, g.end, g.reason) for g in sb] for sb in segs]}')
    assert [[(g.start, g.end, g.reason) for g in sb] for sb in segs] == full
    assert all(sb[-1].reason == 0 and sb[-1].end == out_lens[b] - 1 for b, sb in enumerate(segs))
    # the beam: every segment against the device decode of the offline logits' slice
    slices = [(b, g.start, g.end) for b, sb in enumerate(segs) for g in sb]
    labels, count, score, _ = _decode_slices(off, slices, blank, W, None)
    flat = [g for sb in segs for g in sb]
    for i, g in enumerate(flat):
        assert g.beam_labels == labels[i], (slices[i], g.beam_labels, labels[i])
        assert np.float32(g.beam_score).view(np.uint32) == score[i], (slices[i], g.beam_score)
        assert g.lm_score is None
    assert any(g.beam_labels for g in flat)
    # beam_hypotheses is the open segment's, here the last one's
    assert s.beam_hypotheses == [sb[-1].beam_labels for sb in segs]
    # the greedy side and the logits are untouched
    assert torch.equal(logits[0], logits[1]) and torch.equal(logits[0], off)
    assert s.hypotheses == plain.hypotheses and s.hypothesis_frames == plain.hypothesis_frames
    for b in range(2):
        assert sum((g.labels for g in segs[b]), []) == s.hypotheses[b]
        frames = iter(s.hypothesis_frames[b])
        for g in segs[b]:
            assert all(g.start <= next(frames) <= g.end for _ in g.labels)
    with pytest.raises(ValueError, match='endpoint'):
        plain.segments
    # pop_segments() hands the closed segments over with their labels
    assert s.pop_segments() == segs and s.segments == [[], []]
    assert s.hypotheses == [[], []] and s.hypothesis_frames == [[], []]
    # reset() starts the endpointer over too
    s.reset()
    s.push(feats[:, :12])
    for pos in range(12, 96, 12):
        s.push(feats[:, pos:pos + 12])
    first = [[(g.start, g.end, g.reason) for g in sb] for sb in s.segments]
    assert first == [[c for c in full[b] if c[2] and c[1] < 96 // 4 - s.lookahead] for b in range(2)]
    # popped mid-stream, the rest of the session gives the remaining segments, labels included
    popped = s.pop_segments()
    assert sum(len(p) for p in popped) > 0
    for pos in range(96, T, 12):
        n = min(12, T - pos)
        s.push(feats[:, pos:pos + n], [ln if pos <= ln <= pos + n and ln < T else -1 for ln in lens])
    s.finish()
    assert [popped[b] + s.segments[b] for b in range(2)] == segs
    assert [sum((g.labels for g in s.segments[b]), []) for b in range(2)] == s.hypotheses


def test_front_end_segments(cuda, built):
    """push_audio on c1_mini with a sliding CMVN and an endpointer: the segments of the same
    router fed the offline features fe(samples, n) through push in the same groups of 4."""
    from srf_amd import fbank
    from srf_amd.streaming import StreamingRouter, audio_chunk_bound
    from tests import fbank_ref
    model, sh = built('c1_mini', evaluation=False)
    fe = fbank.Fbank(cmvn=fbank.SlidingCmvn(window=16, device=cuda), device=cuda)
    lens = [400 + 160 * 199 + 77, 400 + 160 * 150]   # 200 and 151 feature frames: 50 and 38 output frames
    N = max(lens)
    sig = fbank_ref.signal_noise(N + 97)
    x = torch.tensor(np.stack([sig[:N], sig[97:97 + N]]), device=cuda)
    assert audio_chunk_bound(16) == 1280
    probe = StreamingRouter(model, 2, max_chunk=16)
    nmax = max(4, probe.lookahead)
    rules = endpoint.EndpointRules(nmax + 1, nmax, nmax + 7, 0.5)   # 50 and 38 frames leave a remainder open
    s = StreamingRouter(model, 2, max_chunk=16, frontend=fe, beam_width=4, endpoint=rules)
    calls, push = [], s.push

    def recording_push(feats, ended=None):
        calls.append((feats.clone(), ended))
        return push(feats, ended)
    s.push = recording_push
    for pos in range(0, N, 1280):
        n = min(1280, N - pos)
        s.push_audio(x[:, pos:pos + n], [-1, lens[1]] if pos <= lens[1] < pos + n else None)
    last = s.finish()
    ref = StreamingRouter(model, 2, max_chunk=16, beam_width=4, endpoint=rules)
    for feats, ended in calls:
        ref.push(feats, ended)
    ref.finish()
    got, want = s.segments, ref.segments
    print(f'segments from audio: {[[(g.start, g.end, g.reason) for g in sb] for sb in got]}')
    assert got == want
    assert [sb[-1].end for sb in got] == [49, 37] and all(len(sb) >= 3 for sb in got)
    assert all(sb[-1].reason == 0 for sb in got) and all(g.reason == 0 for sb in last.segments for g in sb[-1:])
    assert s.hypotheses == ref.hypotheses
