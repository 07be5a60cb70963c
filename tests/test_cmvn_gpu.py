"""Sliding-window CMVN on the GPU (srf_amd/fbank.py SlidingCmvn, csrc/cmvn.hip, DESIGN.md
section 20).

Reference: the float64 numpy oracle of tests/cmvn_ref.py (direct sums per frame), pinned by
the anchors of tests/test_cmvn_cpu.py.  Tolerance: |kernel - oracle| <= 4 u elementwise,
u = 2^-24 max(1, |y|).  A correctly rounded fp64 result is within 1 u; the factor 4 covers an
fp64 division and square root that are not correctly rounded and the order of the fp64 sums
(tests/test_cmvn_cpu.py bounds that at 0.5 u, measured 7e-7 u).  It does not admit forming
x - m in fp32.

Inputs (cmvn_ref.features): every dimension Gaussian, static-like (means 8 .. 16,
deviations 2 .. 5) or delta-like (means +-0.2, deviations 0.4 .. 1.5), float32, fixed seeds.
Shapes (cmvn_ref.SHAPES): B = 3, D = 123, lengths [50, 7, 0], W = 16 (a filling and a
sliding window, a row shorter than W, a zero-frame row, two tiles of 32 frames) without a
prior, with a shared and with a per-row one worth 5 frames; B = 1, T = 700, W = 600;
B = 1, T = 2000, W = 8; W = 1; D = 5 and D = 128.  The chunked runs use the chunks
[1, 3, 31, 32, 33, rest]; the 50-frame batch takes only the first three of them, so they also
run on the same batch with its long row drawn out to 130 frames.

Observed on an MI355X, max |err| in u (limit 4): 0.985 with and 0.999 without norm_vars on
the B = 3 batch without a prior, 0.985 / 0.995 with either prior; 0.997 at W = 600; 0.998 at
T = 2000 (first 100 frames 0.994, last 100 frames 0.991: no growth); 0 at W = 1; 0.913 / 0.916
at D = 5, 0.973 / 0.995 at D = 128; the 130-frame batch 0.985 / 0.999; after a carry 0.959,
after reset() 0.978; the carried mean and count equal the oracle's, the carried deviation
within 2.3e-15.  Streamed against offline, from features and from samples, and push_audio
against push: equal bits in every case.  The tuple CMVN against the formula on the plain
output: 2.2e-7, against its oracle 3.7e-6, limit 1.70e-5.  Each test prints its figures
before it asserts."""
import numpy as np
import pytest
import torch

from tests import cmvn_ref as R
from tests import fbank_ref
from tests.helpers import config_from_shape, load_model_fixture

pytestmark = pytest.mark.gpu

LIMIT_U = 4.0
CHUNKS = [1, 3, 31, 32, 33]
NORM_VARS = {'w600': (True,), 'long': (True,)}          # the other shapes run both ways


@pytest.fixture(scope='module')
def reference():
    """name -> the case of cmvn_ref.case plus y[norm_vars] (oracle float64 [B, T, D]);
    computed once and left unchanged."""
    out = {}
    for name in R.SHAPES:
        c = R.case(name)
        prior = None if c['prior'] is None else c['prior'] + (c['prior_frames'],)
        c['y'] = {nv: R.batch(c['x'], c['lens'], c['window'], nv, prior)[0] for nv in NORM_VARS.get(name, (True, False))}
        out[name] = c
    return out


def _sc(c, nv, cuda, **kw):
    from srf_amd import fbank
    return fbank.SlidingCmvn(window=c['window'], norm_vars=nv, prior=c['prior'], prior_frames=c['prior_frames'],
                             dim=c['x'].shape[2], device=cuda, **kw)


def _err_u(got, want):
    got = got.cpu().double().numpy()
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all()
    return np.abs(got - want) / R.unit(want)


def _check(got, want, lens, what):
    err = _err_u(got, want)
    print(f'{what}: max err {err.max():.3f} u, limit {LIMIT_U} u')
    assert err.max() <= LIMIT_U, (what, float(err.max()))
    got = got.cpu().numpy()
    for b, T in enumerate(lens):
        assert not got[b, T:].any(), f'{what}: padding rows of stream {b} are not zero'
    return err


@pytest.mark.parametrize('norm_vars', [True, False])
@pytest.mark.parametrize('name', ['acc', 'acc_shared', 'acc_rows'])
def test_accuracy_against_oracle(cuda, reference, name, norm_vars):
    c = reference[name]
    x = torch.tensor(c['x'], device=cuda)
    sc = _sc(c, norm_vars, cuda)
    got = sc(x, torch.tensor(c['lens'], device=cuda))
    got_host = sc(x, c['lens'])
    assert got.dtype == torch.float32 and got.is_cuda and torch.equal(got, got_host)
    _check(got, c['y'][norm_vars], c['lens'], f'{name} norm_vars={norm_vars}')


@pytest.mark.parametrize('name', ['w600', 'long', 'w1', 'd5', 'd128'])
def test_other_shapes(cuda, reference, name):
    c = reference[name]
    x = torch.tensor(c['x'], device=cuda)
    for nv, want in c['y'].items():
        got = _sc(c, nv, cuda)(x, c['lens'])
        err = _check(got, want, c['lens'], f'{name} norm_vars={nv}')
        if name == 'long':     # the error must not grow with the stream's length
            print(f'long: first 100 frames {err[0, :100].max():.3f} u, last 100 frames {err[0, -100:].max():.3f} u')
            assert err[0, -100:].max() <= LIMIT_U
        if name == 'w1':
            assert not got.cpu().numpy().any(), 'W = 1 without a prior normalises every frame with itself'


@pytest.mark.parametrize('norm_vars', [True, False])
def test_exact_zeros(cuda, reference, norm_vars):
    """No prior: frame 0 of every column and a column that is constant (-15.9424) come out
    as exactly 0; the fp64 sums of such a column are exact."""
    c = reference['acc']
    x = c['x'].copy()
    x[:, :, 3] = np.float32(-15.9424)
    got = _sc(c, norm_vars, cuda)(torch.tensor(x, device=cuda), c['lens']).cpu().numpy()
    assert not got[:, 0].any(), 'frame 0 must be exactly 0'
    assert not got[:, :, 3].any(), 'a constant column must be exactly 0'
    assert got[0, 1:, :3].all() and got[1, 1:7, 4:].all()


def _stream_cmvn(s, x, lens, chunks):
    """Push x [B, T, D] through the SlidingCmvnStream in ``chunks``, declaring each
    stream's end with the chunk it lies in."""
    B, T, _ = x.shape
    assert sum(chunks) == T
    outs, pos, declared = [], 0, [False] * B
    for m in chunks:
        total = [-1] * B
        for b, ln in enumerate(lens):
            if not declared[b] and pos <= ln <= pos + m:
                total[b], declared[b] = ln, True
        outs.append(s.push(x[:, pos:pos + m].contiguous(), total))
        pos += m
        assert s.pushed == pos and outs[-1].shape == (B, m, x.shape[2])
    assert all(declared)
    return torch.cat(outs, dim=1)


@pytest.mark.parametrize('norm_vars', [True, False])
@pytest.mark.parametrize('name', ['acc', 'acc_rows', 'chunk', 'chunk_rows'])
def test_chunk_invariance_of_the_cmvn_stream(cuda, reference, name, norm_vars):
    """SlidingCmvnStream on its own: the concatenated output is the offline call bit for
    bit; the short streams end inside a chunk."""
    from srf_amd import fbank
    c = reference[name]
    x, lens, T = torch.tensor(c['x'], device=cuda), c['lens'], c['x'].shape[1]
    chunks = [m for i, m in enumerate(CHUNKS) if sum(CHUNKS[:i + 1]) < T]
    chunks.append(T - sum(chunks))
    assert chunks == ([1, 3, 31, 15] if T == 50 else [1, 3, 31, 32, 33, 30])
    sc = _sc(c, norm_vars, cuda)
    want = sc(x, lens)
    s = fbank.SlidingCmvnStream(sc, len(lens), max(chunks))
    got = _stream_cmvn(s, x, lens, chunks)
    assert torch.equal(got, want), (chunks, float((got - want).abs().max()))
    s.reset()
    big = max(chunks)
    again = _stream_cmvn(s, x, lens, [big] * (T // big) + [T % big])
    assert torch.equal(again, want)
    if name.startswith('chunk'):
        _check(want, c['y'][norm_vars], lens, f'{name} norm_vars={norm_vars}')


LENS_AUDIO = [400 + 160 * 36 + 77, 4000, 399]     # 37, 23 and 0 frames
AUDIO_CHUNKS = [400, 1, 159, 1600]


def _audio(lens, cuda):
    N = max(lens)
    sig = fbank_ref.signal_noise(N + 97 * len(lens))
    return torch.tensor(np.stack([sig[97 * b:97 * b + N] for b in range(len(lens))]), device=cuda)


def _audio_prior():
    return (np.concatenate([np.full(41, 12.0), np.zeros(82)]), np.concatenate([np.full(41, 4.0), np.ones(82)]))


@pytest.mark.parametrize('prior', [False, True])
@pytest.mark.parametrize('norm_vars', [True, False])
def test_chunk_invariance_from_samples(cuda, norm_vars, prior):
    """FbankStream on a front end with a sliding CMVN: its output, and the offline front
    end's, equal sc(*plain_fe(samples, n)) bit for bit."""
    from srf_amd import fbank
    sc = fbank.SlidingCmvn(window=16, norm_vars=norm_vars, prior=_audio_prior() if prior else None, prior_frames=5,
                           device=cuda)
    fe, plain = fbank.Fbank(cmvn=sc, device=cuda), fbank.Fbank(device=cuda)
    x, n = _audio(LENS_AUDIO, cuda), torch.tensor(LENS_AUDIO, device=cuda)
    raw, T = plain(x, n)
    want = sc(raw, T)
    assert T.tolist() == [37, 23, 0] and want.shape == (3, 37, 123)
    offline, T2 = fe(x, n)
    assert torch.equal(offline, want) and torch.equal(T, T2)
    assert torch.equal(fe.static(x, n)[0], plain.static(x, n)[0])
    chunks = AUDIO_CHUNKS + [x.shape[1] - sum(AUDIO_CHUNKS)]
    s = fbank.FbankStream(fe, 3, max(chunks))
    outs, pos, declared = [], 0, [False] * 3
    for m in chunks:
        ended = [-1] * 3
        for b, ln in enumerate(LENS_AUDIO):
            if not declared[b] and pos <= ln <= pos + m:
                ended[b], declared[b] = ln, True
        outs.append(s.push(x[:, pos:pos + m], ended))
        pos += m
    outs.append(s.finish())
    got = torch.cat(outs, dim=1)
    assert got.shape == want.shape and torch.equal(got, want), float((got - want).abs().max())
    assert want[0].abs().max() > 0 and not want[2].any()


def test_speaker_carry(cuda, reference):
    """Two utterances per stream with reset(carry=True) between them; stream 2's first one
    is empty, so it keeps the constructor's prior.  The second utterance matches the oracle
    run with the oracle's carried prior; after reset() it is the constructor's prior again."""
    from srf_amd import fbank
    c = reference['acc_rows']
    frames, speaker = c['prior_frames'], 14          # n + c is 16 and 12 after utterance 1: one capped, one not
    sc = _sc(c, True, cuda, speaker_frames=speaker)
    x1, lens1 = torch.tensor(c['x'], device=cuda), c['lens']
    x2_host, lens2 = R.features(3, 30, 123, seed=21), [20, 30, 9]
    x2 = torch.tensor(x2_host, device=cuda)
    s = fbank.SlidingCmvnStream(sc, 3, 32)
    first = _stream_cmvn(s, x1, lens1, [20, 30])
    assert torch.equal(first, sc(x1, lens1))
    s.reset(carry=True)
    got = _stream_cmvn(s, x2, lens2, [7, 23])
    torch.cuda.synchronize()

    prior = c['prior'] + (float(frames),)
    _, lasts = R.batch(c['x'], lens1, c['window'], True, prior)
    carried = R.carry(lasts, (prior[0], prior[1], np.full(3, float(frames))), speaker, 3, 123)
    assert carried[2].tolist() == [14.0, 12.0, 5.0]
    for name, dev, host in zip(('mean', 'std', 'count'), (s.prior_mean, s.prior_std, s.prior_count), carried):
        rel = np.abs(dev.cpu().numpy() - host) / np.maximum(1.0, np.abs(host))
        print(f'carried {name}: max relative difference {rel.max():.2e}')
        # the kernel's sums take at most W + 2 tiles = 80 fp64 additions of partial sums below
        # 16 * 31^2: |error of q| <= 80 * 1.1e-16 * 15376 / 16 = 8.5e-12, and a static-like
        # deviation is at least 2, so sqrt(q - m^2) moves by at most 8.5e-12 / 4
        assert rel.max() <= 1e-11
    want, _ = R.batch(x2_host, lens2, c['window'], True, carried)
    _check(got, want, lens2, 'second utterance, carried prior')
    fresh, _ = R.batch(x2_host, lens2, c['window'], True, prior)
    assert (np.abs(want - fresh) / R.unit(want)).max() > 100, 'the carried prior must matter'

    s.reset()
    again = _stream_cmvn(s, x2, lens2, [30])
    assert torch.equal(again, sc(x2, lens2))
    _check(again, fresh, lens2, 'second utterance, constructor prior')


def test_push_audio_end_to_end(cuda):
    """c1_mini with a front end whose CMVN slides: push_audio's logits are, bit for bit,
    those of a router fed the offline features fe(samples, n) through push in the same
    groups of 4 frames; the audio lookahead is what it was."""
    from srf_amd import fbank
    from srf_amd.sequence_router import SequenceRouter
    from srf_amd.streaming import StreamingRouter, audio_chunk_bound
    kw, sh, P, _ = load_model_fixture('c1_mini')
    model = SequenceRouter(config_from_shape(kw), None, sh.class_n, device=cuda)
    model.load_params(P)
    fe = fbank.Fbank(cmvn=fbank.SlidingCmvn(window=16, prior=_audio_prior(), device=cuda), device=cuda)
    lens = LENS_AUDIO[:2]
    x = _audio(lens, cuda)
    chunks = [1280, 1, 399, 1000, 1280, 1280, 997]
    assert sum(chunks) == lens[0] and audio_chunk_bound(16) == 1280

    s = StreamingRouter(model, 2, max_chunk=16, frontend=fe)
    assert s.lookahead_audio_ms == 65
    calls, push = [], s.push

    def recording_push(feats, ended=None):
        calls.append((feats.clone(), ended))
        return push(feats, ended)
    s.push = recording_push

    def run():
        outs, pos = [], 0
        for n in chunks:
            ended = [-1, 4000] if pos <= 4000 < pos + n else None
            outs.append(s.push_audio(x[:, pos:pos + n], ended))
            pos += n
        outs.append(s.finish())
        return torch.cat([o.logits for o in outs], dim=1)
    logits = run()

    offline, T = fe(x, torch.tensor(lens, device=cuda))
    assert T.tolist() == [37, 23]
    offline = torch.cat([offline, offline.new_zeros((2, 3, 123))], dim=1)
    ref = StreamingRouter(model, 2, max_chunk=16)
    ref_outs, pos = [], 0
    for feats, ended in calls:
        n = feats.shape[1]
        assert n % 4 == 0 and torch.equal(feats, offline[:, pos:pos + n]), pos
        ref_outs.append(ref.push(offline[:, pos:pos + n].contiguous(), ended))
        pos += n
    assert pos == 40
    ref_outs.append(ref.finish())
    ref_logits = torch.cat([o.logits for o in ref_outs], dim=1)
    torch.cuda.synchronize()
    assert logits.shape == ref_logits.shape and logits.shape[1] > 0
    assert torch.equal(logits, ref_logits), float((logits - ref_logits).abs().max())
    assert s.hypotheses == ref.hypotheses

    # reset() starts over with the same bits; reset(carry_cmvn=True) takes the speakers along
    s.reset()
    assert torch.equal(run(), logits)
    s.reset(carry_cmvn=True)
    assert s._fe._cmvn.prior_count.tolist() == [16.0, 16.0]
    carried = run()
    assert carried.shape == logits.shape and not torch.equal(carried, logits)
    with pytest.raises(ValueError, match='carry_cmvn'):
        ref.reset(carry_cmvn=True)


def test_tuple_and_plain_paths_are_unchanged(cuda):
    """Fbank(cmvn=(mean, std)) against (plain - mean + 1e-14) / (std + 1e-14) formed in fp64
    from Fbank()'s own output, on the noise batch of tests/test_fbank_gpu.py and within that
    test's limit (8 x the error of the oracle's float32 restatement); neither front end has a
    sliding stage."""
    from srf_amd import fbank
    lens = [2237, 560, 399]
    x = _audio(lens, cuda)
    rng = np.random.default_rng(11)
    mean = np.concatenate([rng.uniform(8, 16, (3, 41)), rng.uniform(-0.2, 0.2, (3, 82))], axis=1).astype(np.float32)
    std = np.concatenate([rng.uniform(2, 5, (3, 41)), rng.uniform(0.4, 1.5, (3, 82))], axis=1).astype(np.float32)
    o64, T = fbank_ref.batch(x.cpu().numpy(), lens, dtype=np.float64, mean=mean, std=std)
    o32, _ = fbank_ref.batch(x.cpu().numpy(), lens, dtype=np.float32, mean=mean, std=std)
    limit = min(8.0 * float(np.abs(o32.astype(np.float64) - o64).max()), 1e-3)
    plain_fe, tuple_fe = fbank.Fbank(device=cuda), fbank.Fbank(cmvn=(mean, std), device=cuda)
    assert plain_fe.sliding is None and tuple_fe.sliding is None and tuple_fe.cmvn_rows(3) == 3
    n = torch.tensor(lens, device=cuda)
    plain, T1 = plain_fe(x, n)
    normed, T2 = tuple_fe(x, n)
    assert T1.tolist() == T2.tolist() == list(T) == [12, 2, 0]
    want = (plain.cpu().double().numpy() - mean[:, None] + 1e-14) / (std[:, None].astype(np.float64) + 1e-14)
    for b, t in enumerate(T):
        want[b, t:] = 0.0
    err = np.abs(normed.cpu().double().numpy() - want).max()
    err_oracle = np.abs(normed.cpu().double().numpy() - o64).max()
    print(f'tuple CMVN against the formula on the plain output: {err:.3e}, against the oracle: {err_oracle:.3e}, '
          f'limit {limit:.3e}')
    assert err <= limit and err_oracle <= limit
    s = fbank.FbankStream(tuple_fe, 3, 2237)
    assert s._cmvn is None
    got = torch.cat([s.push(x, lens), s.finish()], dim=1)
    assert torch.equal(got, normed)
