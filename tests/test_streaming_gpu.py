"""Chunked streaming inference on the GPU (srf_amd/streaming.py, csrc/stream.hip).

Definition of correct: after finish() the concatenated logits are those of
``model(all pushed feats, input_lengths=lens, training=False)`` -- every stream, every
output frame, padding frames included -- however the frames were cut into chunks.

References: the evaluation fixtures of the CPU oracle (c3_real / c4_real), the float64
oracle run in the test on seeded inputs (B = 2, T = 96, lengths [96, 70]: stream 1 ends
mid-session and is padding from there on), and the offline GPU forward.  Tolerances:
the project's |err| <= 1e-4 (1 + |ref|) against the oracle (tests/test_eval_gpu.py);
streamed against offline twice that, both being within one tolerance of the exact value.

The B = 1 cases stream utterance 1 of the same inputs alone (length 70 of 96 pushed
frames): the evaluation path has no coupling across the batch, so the reference is row 1
of the B = 2 oracle result.

Observed on an MI355X: max |err| against the oracle 1.2e-6 .. 1.1e-5, at most 0.062
tolerances (c3_real); max |streamed - offline| 0 in every case.
Each test prints its figures before it asserts."""
import numpy as np
import pytest
import torch

from oracle import srf_oracle as so
from tests.helpers import config_from_shape, load_eval_fixture

pytestmark = pytest.mark.gpu

MOVING = ['bn0_moving_mean', 'bn0_moving_var', 'bn1_moving_mean', 'bn1_moving_var']
MINI = ['c1_mini', 'c2_mini', 'c2_mini_lowmemory', 'c3_mini_sdr', 'c3_mini_sdr_lowmemory', 'c4_mini']
PATTERNS = [[96], [12] * 8, [4] * 24, [4, 20, 8, 4, 36, 24]]
CASES = [(name, 2) for name in MINI] + [('c3_mini_sdr', 1), ('c4_mini', 1)]
T, LENS = 96, [96, 70]


def _pid(p):
    return 'x'.join(map(str, p)) if len(set(p)) > 1 else f'{p[0]}*{len(p)}'


@pytest.fixture(scope='module')
def built(cuda):
    """built(name, **config overrides) -> (model, shape, oracle params, eval arrays); one
    model per fixture for the module (evaluation writes nothing to it)."""
    from srf_amd.sequence_router import SequenceRouter
    cache = {}

    def get(name, **over):
        key = (name, tuple(sorted(over.items())))
        if key not in cache:
            kw, sh, P, z, ev = load_eval_fixture(name)
            model = SequenceRouter(config_from_shape(kw, **over), None, sh.class_n, device=cuda)
            model.load_params(P)
            cache[key] = (model, sh, P, z, ev)
        return cache[key]
    yield get
    cache.clear()


@pytest.fixture(scope='module')
def reference(cuda, built):
    """reference(name, B) -> (feats [B, T, F] device, lens, oracle logits, offline GPU
    logits), computed once per case and left unchanged."""
    cache = {}

    def get(name, B):
        if name not in cache:
            model, sh, P, _, _ = built(name)
            feats = np.random.default_rng(20).standard_normal((2, T, sh.feat_dim)).astype(np.float32)
            ref = so.srf_forward(P, sh, feats.astype(np.float64), np.array(LENS), bn_training=False)
            ft = torch.tensor(feats, device=cuda)
            with torch.no_grad():
                off = model(ft, input_lengths=torch.tensor(LENS, device=cuda), training=False)
            cache[name] = (ft, ref, off)
        ft, ref, off = cache[name]
        rows = slice(0, 2) if B == 2 else slice(1, 2)
        return ft[rows].contiguous(), LENS[rows], ref[rows], off[rows]
    yield get
    cache.clear()


def _stream(s, feats, lens, pattern):
    """Push ``feats`` in chunks of ``pattern``, declaring each stream's length with the
    chunk its end lies in (a stream as long as everything pushed declares nothing), and
    finish.  Checks the emission bound after every push.  Returns (logits, labels)."""
    total = feats.shape[1]
    declared = [False] * len(lens)
    outs, pos = [], 0
    for n in pattern:
        ended = [-1] * len(lens)
        for b, ln in enumerate(lens):
            if ln < total and not declared[b] and pos <= ln <= pos + n:
                ended[b], declared[b] = ln, True
        outs.append(s.push(feats[:, pos:pos + n], ended))
        pos += n
        assert outs[-1].t0 + outs[-1].logits.shape[1] >= pos // 4 - s.lookahead, (pos, outs[-1].t0)
    assert pos == total
    outs.append(s.finish())
    t = 0
    for o in outs:
        assert o.t0 == t and o.logits.shape[0] == len(lens)
        t += o.logits.shape[1]
    assert t == total // 4
    labels = [sum((o.labels[b] for o in outs), []) for b in range(len(lens))]
    return torch.cat([o.logits for o in outs], dim=1), labels


def _logit_check(got, ref, what, tol=1e-4):
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = np.abs(got - ref)
    print(f'{what}: max err {err.max():.3e}, in tolerances {(err / (tol * (1 + np.abs(ref)))).max():.3f}')
    assert np.all(err <= tol * (1 + np.abs(ref))), err.max()


@pytest.mark.parametrize('name', ['c3_real', 'c4_real'])
def test_stream_oracle_fixture(cuda, built, name):
    """The evaluation fixtures (T = 60, lengths [60, 47]) pushed in chunks of 12: stream
    1 ends in the fourth chunk and is padding after it, stream 0 never declares a length.
    Logits and greedy hypotheses against the oracle; the moving statistics unchanged."""
    from srf_amd.streaming import StreamingRouter
    model, sh, _, z, ev = built(name)
    feats = torch.tensor(z['feats'], dtype=torch.float32, device=cuda)
    lens = [int(x) for x in z['inp_len']]
    assert feats.shape[1] == 60 and lens == [60, 47]
    before = [getattr(model, n).clone() for n in MOVING]
    s = StreamingRouter(model, 2, max_chunk=12)
    assert s.lookahead == 2 + sh.enc_num * sh.rpad
    logits, labels = _stream(s, feats, lens, [12] * 5)
    torch.cuda.synchronize()
    for n, b in zip(MOVING, before):
        assert torch.equal(getattr(model, n), b), n
    _logit_check(logits.cpu().double().numpy(), ev['logits'].astype(np.float64), name)
    assert s.hypotheses == ev['greedy_ceil']
    assert labels == ev['greedy_ceil']


@pytest.fixture(scope='module')
def streamed(cuda, built, reference):
    """streamed(name, B, pattern) -> (logits, labels), each case streamed once."""
    from srf_amd.streaming import StreamingRouter
    cache = {}

    def get(name, B, pattern):
        key = (name, B, tuple(pattern))
        if key not in cache:
            model = built(name)[0]
            feats, lens, _, _ = reference(name, B)
            s = StreamingRouter(model, B, max_chunk=96)
            logits, labels = _stream(s, feats, lens, pattern)
            assert s.hypotheses == labels
            cache[key] = (logits, labels)
        return cache[key]
    yield get
    cache.clear()


@pytest.mark.parametrize('pattern', PATTERNS, ids=_pid)
@pytest.mark.parametrize('name,B', CASES)
def test_stream_against_oracle(cuda, built, reference, streamed, name, B, pattern):
    """Streamed logits against the float64 oracle of the whole utterances (the emission
    bound is checked after every push, in _stream); the labels the chunks added are the
    greedy decode of the streamed logits at ceil(len / 4)."""
    from srf_amd import ctc
    model, sh = built(name)[:2]
    before = [getattr(model, n).clone() for n in MOVING]
    _, lens, ref, _ = reference(name, B)
    logits, labels = streamed(name, B, pattern)
    _logit_check(logits.cpu().double().numpy(), ref, f'{name} B={B} {_pid(pattern)}')
    assert labels == ctc.greedy_decode(logits, (torch.tensor(lens) + 3) // 4, sh.class_n - 1)
    for n, b in zip(MOVING, before):
        assert torch.equal(getattr(model, n), b), n


@pytest.mark.parametrize('pattern', PATTERNS, ids=_pid)
@pytest.mark.parametrize('name,B', CASES)
def test_stream_against_offline(cuda, reference, streamed, name, B, pattern):
    """Streamed against the offline GPU forward of the same audio: each is within 1e-4
    (1 + |exact|) of the exact value, so they differ by at most twice that."""
    off = reference(name, B)[3]
    logits = streamed(name, B, pattern)[0]
    d = (logits - off).abs()
    print(f'{name} B={B} {_pid(pattern)}: max |streamed - offline| {d.max().item():.3e}')
    assert torch.all(d <= 2e-4 * (1 + off.abs())), d.max().item()


@pytest.mark.parametrize('name', ['c3_mini_sdr', 'c2_mini'])
def test_reset_equals_a_fresh_session(cuda, built, reference, name):
    """Half an utterance, reset(), then another utterance: bit for bit what a fresh
    session gives (a stale SDR carry or stale halo frames would show)."""
    from srf_amd.streaming import StreamingRouter
    model = built(name)[0]
    feats, lens, _, _ = reference(name, 2)
    other = torch.flip(feats, dims=[0, 1]).contiguous() * 0.5
    pattern = [12, 20, 4, 28, 32]
    fresh = StreamingRouter(model, 2, max_chunk=32)
    want, want_labels = _stream(fresh, other, [70, 96], pattern)
    s = StreamingRouter(model, 2, max_chunk=32)
    s.push(feats[:, :32], [-1, -1])
    s.push(feats[:, 32:48], [-1, -1])
    assert s.hypotheses is not None
    s.reset()
    got, got_labels = _stream(s, other, [70, 96], pattern)
    assert torch.equal(got, want)
    assert got_labels == want_labels == s.hypotheses
    s.reset()   # after finish() too
    again, _ = _stream(s, other, [70, 96], pattern)
    assert torch.equal(again, want)


def test_refusals(cuda, built):
    from srf_amd.streaming import StreamingRouter
    with pytest.raises(ValueError, match='einsum'):
        StreamingRouter(built('c2_mini_einsum')[0], 2)
    with pytest.raises(ValueError, match='fp8'):
        StreamingRouter(built('c3_mini_sdr', model_pose_fp8=True)[0], 2)
    model, sh = built('c2_mini')[:2]
    with pytest.raises(ValueError, match='max_chunk'):
        StreamingRouter(model, 2, max_chunk=30)
    s = StreamingRouter(model, 2, max_chunk=16)
    x = torch.zeros((2, 16, sh.feat_dim), device=cuda)
    with pytest.raises(ValueError, match='multiple of 4'):
        s.push(x[:, :10])
    with pytest.raises(ValueError, match='max_chunk'):
        s.push(torch.zeros((2, 20, sh.feat_dim), device=cuda))
    with pytest.raises(ValueError, match=r'feats must be \[2'):
        s.push(x[:1])
    with pytest.raises(ValueError, match='feats must be'):
        s.push(x[:, :, :-1])
    s.push(x, [-1, 9])
    with pytest.raises(ValueError, match='already declared'):
        s.push(x, [-1, 20])
    with pytest.raises(ValueError, match='before this chunk'):
        s.push(x, [15, -1])
    out = s.push(x, [16, -1])   # a refused push left the session where it was
    assert out.t0 == max(0, 16 // 4 - s.lookahead)
    assert out.t0 + out.logits.shape[1] == max(0, 32 // 4 - s.lookahead)
    s.finish()
    with pytest.raises(ValueError, match='after finish'):
        s.push(x)
    with pytest.raises(ValueError, match='already called'):
        s.finish()
    s.reset()
    s.push(x)


# ---------------------------------------------------------------------------
# srf_ctc_greedy_n

def _greedy_chunks(logits, lens, blank, split):
    """The kernel over ``logits`` [B, T, C] cut into chunks of ``split`` frames."""
    from srf_amd import ctc
    B = logits.shape[0]
    prev = torch.full((B,), -1, device=logits.device, dtype=torch.int32)
    lens_t = torch.tensor(lens, device=logits.device, dtype=torch.int32)
    got, pos = [[] for _ in range(B)], 0
    for n in split:
        n_valid = (lens_t - pos).clamp(0, n)
        labels, count = ctc.greedy_decode_device(logits[:, pos:pos + n], n_valid, blank, prev)
        assert labels.shape == (B, n) and count.shape == (B,)
        labels, count = labels.cpu().tolist(), count.cpu().tolist()
        for b in range(B):
            assert 0 <= count[b] <= max(0, min(n, lens[b] - pos))
            got[b] += labels[b][:count[b]]
        pos += n
    assert pos == logits.shape[1]
    return got


@pytest.mark.parametrize('C', [2, 32, 63, 130])
def test_ctc_greedy_random(cuda, C):
    """Random logits, chunks of 0, 1, 5 and 64 frames in several orders, lengths that
    end inside a chunk (n_valid < n), at a chunk edge and before a chunk (n_valid = 0),
    against ctc.greedy_decode of the whole.  Few classes make repeats and blanks across
    the chunk edges frequent; C = 130 takes the per-lane class loop past one round."""
    from srf_amd import ctc
    g = torch.Generator().manual_seed(C)
    logits = torch.randn((5, 140, C), generator=g).to(cuda)
    logits[:, :, :max(1, C // 8)] += 1.0   # a few favoured classes: repeats at every C
    lens = [140, 70, 64, 3, 0]
    for blank in (C - 1, 0):
        want = ctc.greedy_decode(logits, torch.tensor(lens), blank)
        for split in ([140], [64, 5, 1, 0, 64, 5, 1], [1, 0, 5, 64, 64, 1, 5], [5] * 28, [1] * 140):
            assert _greedy_chunks(logits, lens, blank, split) == want, (blank, split)


def _path_logits(path, C, dev):
    x = torch.full((1, len(path), C), -1.0, device=dev)
    for t, k in enumerate(path):
        x[0, t, k] = 2.0
    return x


@pytest.mark.parametrize('C', [2, 32, 63])
def test_ctc_greedy_crafted(cuda, C):
    """A label repeated across a chunk edge with and without a blank between, an
    all-blank chunk, and exact ties (the lowest class index wins, as torch.argmax)."""
    from srf_amd import ctc
    blank, a = C - 1, 0
    b = 1 if C > 2 else 0
    # [a a | a blank a | blank blank blank | b blank | blank a]
    path = [a, a, a, blank, a, blank, blank, blank, b, blank, blank, a]
    logits = _path_logits(path, C, cuda)
    want = ctc.greedy_decode(logits, torch.tensor([len(path)]), blank)
    assert want == ([[a, a, b, a]] if C > 2 else [[a, a, a, a]])
    for split in ([2, 3, 3, 2, 2], [12], [1] * 12, [3, 1, 4, 4]):
        assert _greedy_chunks(logits, [len(path)], blank, split) == want, split
    # an all-blank chunk adds nothing and keeps the blank as prev
    prev = torch.tensor([a], device=cuda, dtype=torch.int32)
    labels, count = ctc.greedy_decode_device(_path_logits([blank] * 3, C, cuda),
                                             torch.tensor([3], device=cuda, dtype=torch.int32), blank, prev)
    assert count.tolist() == [0] and prev.tolist() == [blank]
    # exact ties: between two classes, between a class and the blank, between all classes
    ties = torch.full((1, 4, C), -3.0, device=cuda)
    hi = min(C - 1, 40)
    ties[0, 0, [b, hi]] = 1.5
    ties[0, 1, [C // 2, blank]] = 0.25
    ties[0, 2, :] = 0.0
    ties[0, 3, [blank]] = 7.0
    want = ctc.greedy_decode(ties, torch.tensor([4]), blank)
    assert torch.argmax(ties, dim=-1).tolist() == [[b, C // 2, 0, blank]]
    for split in ([4], [1, 1, 1, 1], [2, 0, 2]):
        assert _greedy_chunks(ties, [4], blank, split) == want, split


# ---------------------------------------------------------------------------
# srf_stream_advance_n

def _advance_check(specs, dev):
    """specs: [(B-shaped tensor size tuple, dtype, shift, keep)]; one launch."""
    from srf_amd import ops
    g = torch.Generator().manual_seed(len(specs))
    bufs, wants = [], []
    for shape, dtype, shift, keep in specs:
        t = torch.randint(0, 250, shape, generator=g).to(dtype).to(dev)
        wants.append(t[:, shift:shift + keep].clone())
        bufs.append((t, shape[1], shift, keep))
    ops.stream_advance(bufs)
    torch.cuda.synchronize()
    for (t, rows, shift, keep), want in zip(bufs, wants):
        assert torch.equal(t[:, :keep], want), (tuple(t.shape), t.dtype, shift, keep)


@pytest.mark.parametrize('shift,keep', [(3, 9), (6, 6), (9, 3), (12, 0), (0, 12), (1, 11)])
def test_stream_advance_overlap_cases(cuda, shift, keep):
    """keep > shift (source and destination overlap), keep == shift, keep < shift,
    keep = 0 and shift = 0, with rows of 16-byte multiples, of 4-byte multiples (12 and
    1028 bytes) and of odd byte counts (7), one buffer per launch."""
    for row, dtype in (((8, 4), torch.float32), ((3,), torch.float32), ((257,), torch.float32),
                       ((7,), torch.uint8)):
        _advance_check([((3, 12) + row, dtype, shift, keep)], cuda)


def test_stream_advance_32_buffers(cuda):
    """32 buffers of different shapes, shifts and element sizes in one launch."""
    specs = []
    for i in range(32):
        rows = 5 + i % 7
        shift = i % rows
        keep = (rows - shift) if i % 3 else (rows - shift) // 2
        specs.append(((2, rows, 1 + i % 5, 3 + i % 4), torch.float32 if i % 2 else torch.int16, shift, keep))
    _advance_check(specs, cuda)


def test_stream_advance_overlap_within_a_tile(cuda):
    """Blocks larger than one tile (1024 elements per workgroup pass: 16 KiB of 16-byte
    elements, 4 KiB of 4-byte ones, 1 KiB of bytes) moved by less than a tile: a tile's
    stores land inside the region the same tile reads.  Also a single row larger than a
    tile (20000 bytes), where a tile's stores land in what the tile before it read."""
    _advance_check([((2, 48, 1024), torch.float32, 1, 47)], cuda)     # 4 KiB shift, 188 KiB kept, 16-byte path
    _advance_check([((2, 60, 257), torch.float32, 1, 59)], cuda)      # 1028 B shift, 4-byte path
    _advance_check([((3, 500, 7), torch.uint8, 2, 498)], cuda)        # 14 B shift, byte path
    _advance_check([((2, 6, 5000), torch.float32, 1, 5)], cuda)       # rows of 20000 B
    _advance_check([((2, 6, 5000), torch.float32, 2, 4), ((2, 48, 1024), torch.float32, 3, 40)], cuda)
