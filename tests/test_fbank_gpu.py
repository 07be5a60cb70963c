"""Waveform front end on the GPU (srf_amd/fbank.py, csrc/fbank.hip).

Reference: the float64 numpy oracle of tests/fbank_ref.py, pinned by the anchors of
tests/test_fbank_cpu.py.  Tolerance: max |kernel - oracle| <= 8 x the max error of the
oracle's own float32 restatement on the same input and quantity, computed here, and never
more than 1e-3 (the logit tolerance of smoke()).  The factor 8: a radix-2 fp32 FFT has nine
rounding stages and in-order sums where numpy uses blocked products.

Shapes: B = 3 with 2237, 560 and 399 samples (12, 2 and 0 frames: a zero-frame row, a row
where every delta tap clamps, a ragged batch, a partial last workgroup), and B = 1 with
400 + 160 * 36 + 77 samples (37 frames).  Signals: integer noise and a wide-dynamic-range
mix of tones (fbank_ref.signal_noise / signal_wide), each as int16 and as float32.

Observed on an MI355X (max |err| / limit): statics 1.31e-5 / 5.38e-5 (noise, B = 3),
2.42e-5 / 2.97e-4 (wide, B = 3), 3.01e-5 / 4.04e-4 (wide, B = 1); the 123-d features the
same figures (the largest error sits in a static); with the per-stream CMVN 3.7e-6 /
1.70e-5, 6.3e-6 / 1.06e-4 and 1.6e-5 / 2.31e-4; CmvnStats mean 4.0e-7 and deviation 8.1e-7
against 4.04e-4 (relative); mean frame energy of unit dither 401.8 for 399.  Streamed
against offline and push_audio against push: equal bits in every case.  Each test prints
its figures before it asserts."""
import numpy as np
import pytest
import torch

from tests import fbank_ref as R
from tests.helpers import config_from_shape, load_model_fixture

pytestmark = pytest.mark.gpu

LENS3 = [2237, 560, 399]
N1 = 400 + 160 * 36 + 77
CASES = ['noise3', 'wide3', 'wide1']


def _cmvn(B):
    rng = np.random.default_rng(11)
    mean = np.concatenate([rng.uniform(8, 16, (B, 41)), rng.uniform(-0.2, 0.2, (B, 82))], axis=1)
    std = np.concatenate([rng.uniform(2, 5, (B, 41)), rng.uniform(0.4, 1.5, (B, 82))], axis=1)
    return mean.astype(np.float32), std.astype(np.float32)


def _batch(sig, lens):
    """Row b: the signal from sample 97 b on, so that the rows differ; what lies past a
    row's length is signal too, which the kernels must not read into the result."""
    N = max(lens)
    x = sig(N + 97 * len(lens))
    return np.stack([x[97 * b:97 * b + N] for b in range(len(lens))])


@pytest.fixture(scope='module')
def reference():
    """case -> dict(samples int16 [B, N], lens, cmvn, and per quantity (oracle float64,
    limit)); computed once and left unchanged."""
    out = {}
    for case, sig, lens in [('noise3', R.signal_noise, LENS3), ('wide3', R.signal_wide, LENS3),
                            ('wide1', R.signal_wide, [N1])]:
        x = _batch(sig, lens)
        mean, std = _cmvn(len(lens))
        ref = {'samples': x, 'lens': lens, 'cmvn': (mean, std)}
        for q, kw in [('static', dict(statics_only=True)), ('feats', {}), ('cmvn_feats', dict(mean=mean, std=std))]:
            o64, T = R.batch(x, lens, dtype=np.float64, **kw)
            o32, _ = R.batch(x, lens, dtype=np.float32, **kw)
            ref[q] = (o64, min(8.0 * float(np.abs(o32.astype(np.float64) - o64).max()), 1e-3))
        ref['n_frames'] = T
        out[case] = ref
    return out


def _run(fe, x, lens, cuda, dtype):
    xs = torch.tensor(x.astype(np.float32) if dtype == 'float32' else x, device=cuda)
    assert xs.dtype == (torch.float32 if dtype == 'float32' else torch.int16)
    n = torch.tensor(lens, device=cuda)
    st, T1 = fe.static(xs, n)
    f, T2 = fe(xs, n)
    return st, f, T1, T2


@pytest.mark.parametrize('case', CASES)
def test_accuracy_against_oracle(cuda, reference, case):
    from srf_amd import fbank
    ref = reference[case]
    x, lens = ref['samples'], ref['lens']
    plain, normed = fbank.Fbank(device=cuda), fbank.Fbank(cmvn=ref['cmvn'], device=cuda)
    st, f, T1, T2 = _run(plain, x, lens, cuda, 'int16')
    st_f, f_f, _, _ = _run(plain, x, lens, cuda, 'float32')
    fc, _ = normed(torch.tensor(x, device=cuda), torch.tensor(lens, device=cuda))
    torch.cuda.synchronize()
    assert T1.tolist() == T2.tolist() == ref['n_frames'].tolist() == fbank.n_frames(lens)
    assert T1.dtype == torch.int32 and T1.is_cuda
    assert torch.equal(st, st_f) and torch.equal(f, f_f), 'int16 and float32 samples must give the same bits'
    assert torch.equal(f[:, :, :41], st)
    for q, got in [('static', st), ('feats', f), ('cmvn_feats', fc)]:
        o64, lim = ref[q]
        got = got.cpu().double().numpy()
        assert got.shape == o64.shape, (got.shape, o64.shape)
        err = np.abs(got - o64).max()
        print(f'{case} {q}: max err {err:.3e}, limit {lim:.3e}')
        assert np.isfinite(got).all() and err <= lim, (q, err, lim)
        for b, T in enumerate(ref['n_frames']):
            assert not got[b, T:].any(), f'{q}: padding rows of utterance {b} are not zero'


def test_cmvn_stats(cuda, reference):
    """Two update_state calls (the noise batch, the 37-frame utterance) against the float64
    mean and deviation of the oracle's valid rows.  The limit is the features' own, the
    larger of the two inputs': a mean or a deviation moves by no more than the largest
    error among its rows."""
    from srf_amd import fbank
    fe, stats = fbank.Fbank(device=cuda), fbank.CmvnStats(device=cuda)
    rows, lim = [], 0.0
    for case in ('noise3', 'wide1'):
        ref = reference[case]
        f, T = fe(torch.tensor(ref['samples'], device=cuda), torch.tensor(ref['lens'], device=cuda))
        stats.update_state(f, T)
        o64, lim_case = ref['feats']
        rows += [o64[b, :t] for b, t in enumerate(ref['n_frames'])]
        lim = max(lim, lim_case)
    rows = np.concatenate(rows)
    assert rows.shape == (12 + 2 + 37, 123)
    mean, std = stats.result()
    assert float(stats.sums[-1]) == rows.shape[0]
    for name, got, want in [('mean', mean, rows.mean(axis=0)), ('std', std, rows.std(axis=0))]:
        err = (np.abs(got - want) / np.maximum(1.0, np.abs(want))).max()
        print(f'CmvnStats {name}: max relative err {err:.3e}, limit {lim:.3e}')
        assert err <= lim, (name, err, lim)


def test_dither(cuda):
    from srf_amd import fbank
    n = 400 + 160 * 63
    zeros = torch.zeros((1, n), dtype=torch.int16, device=cuda)
    ln = torch.tensor([n], device=cuda)
    a, _ = fbank.Fbank(dither=1.0, seed=5, device=cuda).static(zeros, ln)
    b, _ = fbank.Fbank(dither=1.0, seed=5, device=cuda).static(zeros, ln)
    c, _ = fbank.Fbank(dither=1.0, seed=6, device=cuda).static(zeros, ln)
    # mean-removed unit Gaussian noise: sum x^2 over 400 samples is chi^2 with 399 degrees
    # of freedom; 64 overlapping frames estimate its mean to better than 2 %
    energy = float(torch.exp(a[0, :, 0].double()).mean())
    print(f'dither: mean frame energy {energy:.2f} (399 expected)')
    assert a.shape == (1, 64, 41) and abs(energy - 399.0) <= 39.9
    assert torch.equal(a, b), 'the same seed must give the same bits'
    assert not torch.equal(a, c), 'another seed must differ'
    x = torch.tensor(R.signal_noise(2237)[None], device=cuda)
    ln = torch.tensor([2237], device=cuda)
    off, _ = fbank.Fbank(device=cuda)(x, ln)
    zero, _ = fbank.Fbank(dither=0.0, seed=9, device=cuda)(x, ln)
    on, _ = fbank.Fbank(dither=1.0, seed=9, device=cuda)(x, ln)
    assert torch.equal(off, zero), 'dither = 0 must be the undithered call'
    assert not torch.equal(off, on)


def _stream(fe, x, lens, chunks, cuda, declare_last=True):
    """Push x [B, N] in ``chunks``, declaring each stream's end with the chunk it lies in
    (declare_last=False: a stream as long as everything pushed is left to finish())."""
    from srf_amd import fbank
    B, N = x.shape
    assert sum(chunks) == N
    s = fbank.FbankStream(fe, B, max(chunks))
    outs, pos, declared = [], 0, [False] * B
    for n in chunks:
        ended = [-1] * B
        for b, ln in enumerate(lens):
            if not declared[b] and pos <= ln <= pos + n and (ln < N or declare_last):
                ended[b], declared[b] = ln, True
        outs.append(s.push(x[:, pos:pos + n], ended))
        pos += n
        assert s.frames_out == sum(o.shape[1] for o in outs)
    outs.append(s.finish())
    return torch.cat(outs, dim=1)


CHUNKINGS = [[2237], [160] * 13 + [157], [1, 399, 161, 640, 1036], [300, 300, 1000, 637]]


@pytest.mark.parametrize('dither', [0.0, 0.5])
def test_chunk_invariance(cuda, reference, dither):
    """The concatenated FbankStream output is the offline output bit for bit, for every
    chunking; the short streams end inside a chunk, the long one at the last chunk's end
    or (last chunking) at finish().  With the per-stream CMVN."""
    from srf_amd import fbank
    ref = reference['noise3']
    fe = fbank.Fbank(dither=dither, seed=3, cmvn=ref['cmvn'], device=cuda)
    x = torch.tensor(ref['samples'], device=cuda)
    want, T = fe(x, torch.tensor(LENS3, device=cuda))
    assert want.shape == (3, 12, 123) and T.tolist() == [12, 2, 0]
    for i, chunks in enumerate(CHUNKINGS):
        got = _stream(fe, x, LENS3, chunks, cuda, declare_last=i < len(CHUNKINGS) - 1)
        assert got.shape == want.shape, (chunks, got.shape)
        assert torch.equal(got, want), (chunks, float((got - want).abs().max()))
    if dither == 0.0:
        err = np.abs(want.cpu().double().numpy() - ref['cmvn_feats'][0]).max()
        assert err <= ref['cmvn_feats'][1]


def test_push_audio_end_to_end(cuda):
    """c2_mini with a front end: push_audio's logits are, bit for bit, those of a second
    router fed the offline features through push in the same groups of 4 frames; the greedy
    hypotheses are equal.  Stream 1 (4000 samples, 23 frames) ends inside a chunk, stream 0
    (37 frames) at finish()."""
    from srf_amd import fbank
    from srf_amd.sequence_router import SequenceRouter
    from srf_amd.streaming import StreamingRouter, audio_chunk_bound
    kw, sh, P, _ = load_model_fixture('c2_mini')
    model = SequenceRouter(config_from_shape(kw), None, sh.class_n, device=cuda)
    model.load_params(P)
    mean = np.concatenate([np.full(41, 12.0), np.zeros(82)])
    std = np.concatenate([np.full(41, 4.0), np.ones(82)])
    fe = fbank.Fbank(cmvn=(mean, std), device=cuda)
    lens = [N1, 4000]
    x = torch.tensor(_batch(R.signal_wide, lens), device=cuda)
    chunks = [1280, 1, 399, 1000, 1280, 1280, 997]
    assert sum(chunks) == N1 and audio_chunk_bound(16) == 1280

    s = StreamingRouter(model, 2, max_chunk=16, frontend=fe)
    assert s.lookahead_audio_ms == 65
    with pytest.raises(ValueError, match='1280'):
        s.push_audio(x[:, :1281])
    calls, push = [], s.push

    def recording_push(feats, ended=None):
        calls.append((feats.clone(), ended))
        return push(feats, ended)
    s.push = recording_push
    outs, pos = [], 0
    for n in chunks:
        ended = [-1, 4000] if pos <= 4000 < pos + n else None
        outs.append(s.push_audio(x[:, pos:pos + n], ended))
        pos += n
    assert outs[0].logits.shape[1] == 0 and outs[0].labels == [[], []]
    outs.append(s.finish())
    logits = torch.cat([o.logits for o in outs], dim=1)
    labels = [sum((o.labels[b] for o in outs), []) for b in range(2)]

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
    assert pos == 40 and [e for _, e in calls if e is not None] == [[-1, 23], [37, -1]]
    ref_outs.append(ref.finish())
    ref_logits = torch.cat([o.logits for o in ref_outs], dim=1)
    torch.cuda.synchronize()
    assert logits.shape == ref_logits.shape == (2, 10, sh.class_n)
    assert torch.equal(logits, ref_logits), float((logits - ref_logits).abs().max())
    assert s.hypotheses == ref.hypotheses == labels
    with pytest.raises(ValueError):
        s.push_audio(x[:, :160])
    s.reset()
    assert s.push_audio(x[:, :1280]).logits.shape[1] == 0
