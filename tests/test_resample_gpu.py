"""Resampler on the GPU (srf_amd/resample.py, csrc/resample.hip).

Reference: the float64 numpy oracle of tests/resample_ref.py, pinned by the anchors of
tests/test_resample_cpu.py.  Limit, per output sample: (taps + 2) 2^-24 sum_j |w64 x_j|, the
first-order rounding bound of an fp32 dot product of ``taps`` terms whose weights were
rounded once (one rounding per weight, one per accumulation, and room for the conversion);
it is derived, not measured, and an output whose taps see only zeros must be exactly zero.
The float32 restatement on the CPU stays within 0.30 of it on the signal every case uses
(fbank_ref.signal_wide: 0.131, 0.138, 0.271, 0.214 and 0.261 for the five cases).  That
figure belongs to the signal, not to the filter: on fbank_ref.signal_noise the 15999 case's
restatement reaches 0.348 at one output, still a third of the limit.

Cases (input lengths -> output counts) and the kernel path each takes -- the weight table in
LDS when ou * (taps | 1) <= 8192 floats, read from global memory otherwise:
  48k      48000 -> 16000  [1501, 37, 0] -> [501, 13, 0]           LDS (37 floats)
  44k      44100 -> 16000  [1403, 441, 5] -> [510, 160, 2]         LDS (160 x 35 floats)
  8k        8000 -> 16000  [333, 1] -> [666, 2]                    LDS
  speed    14400 / 16000 / 17600 -> 16000, choice [0, 1, 2, 0],
           [700, 700, 700, 9] -> [778, 700, 637, 10]               LDS, the 1.0 row a bit copy
  15999    15999 -> 16000  [300] -> [301]                          global (16000 x 13 floats)
A zero-length row, a row shorter than the filter, a row of exactly one unit, ragged
batches, every phase of the 160-phase table.  Rows are cut from one signal, so what lies
past a row's length is signal that must not reach the result.

Observed on an MI355X, max |err| (int16 units) and the largest |err| / limit over a case's
outputs: 48k 1.20e-3, 0.099; 44k 1.92e-3, 0.138; 8k 9.7e-4, 0.232; speed 1.03e-3, 0.232; 15999
9.4e-4, 0.256 -- below the float32 restatement's ratio in four cases and 0.018 above it in
the speed bank (the kernel uses one fma per tap where numpy rounds the product and the
sum).  Streamed against offline and the
resampling router against the 16 kHz one: equal bits in every case.  Each test prints its
figures before it asserts."""
import numpy as np
import pytest
import torch

from tests import resample_ref as R
from tests.helpers import config_from_shape, load_model_fixture

pytestmark = pytest.mark.gpu

CASES = {
    '48k': ([48000], None, [1501, 37, 0], [501, 13, 0]),
    '44k': ([44100], None, [1403, 441, 5], [510, 160, 2]),
    '8k': ([8000], None, [333, 1], [666, 2]),
    'speed': ([14400, 16000, 17600], [0, 1, 2, 0], [700, 700, 700, 9], [778, 700, 637, 10]),
    '15999': ([15999], None, [300], [301]),
}


def _batch(sig, lens):
    """Row b: the signal from sample 97 b on, so that the rows differ; what lies past a
    row's length is signal too, which the kernel must not read into the result."""
    N = max(lens)
    x = sig(N + 97 * len(lens))
    return np.stack([x[97 * b:97 * b + N] for b in range(len(lens))])


@pytest.fixture(scope='module')
def reference():
    """case -> dict(rates, choice, samples int16 [B, N], lens, n_out, oracle float64 [B, Mmax],
    limit [B, Mmax]); computed once and left unchanged."""
    out = {}
    for case, (rates, choice, lens, n_out) in CASES.items():
        filters = [R.Filter(r, 16000) for r in rates]
        ch = choice or [0] * len(lens)
        x = _batch(R.signal_wide, lens)
        o64, M = R.batch(filters, ch, x, lens)
        o32, _ = R.batch(filters, ch, x, lens, dtype=np.float32)
        bd, _ = R.batch(filters, ch, x, lens, what=R.bound)
        taps = np.array([filters[c].taps for c in ch], dtype=np.float64)[:, None]
        lim = (taps + 2.0) * 2.0 ** -24 * bd
        assert M.tolist() == n_out, (case, M)
        ratio32 = float((np.abs(o32.astype(np.float64) - o64) / np.maximum(lim, 1e-300)).max())
        out[case] = dict(rates=rates, choice=choice, samples=x, lens=lens, n_out=n_out, oracle=o64, limit=lim,
                         ratio32=ratio32)
    return out


@pytest.mark.parametrize('case', list(CASES))
def test_accuracy_against_oracle(cuda, reference, case):
    from srf_amd import resample
    ref = reference[case]
    rs = resample.Resampler(ref['rates'] if len(ref['rates']) > 1 else ref['rates'][0], device=cuda)
    x, lens = ref['samples'], torch.tensor(ref['lens'], device=cuda)
    y, n = rs(torch.tensor(x, device=cuda), lens, ref['choice'])
    y_f, n_f = rs(torch.tensor(x.astype(np.float32), device=cuda), lens,
                  None if ref['choice'] is None else torch.tensor(ref['choice']))
    torch.cuda.synchronize()
    assert n.dtype == torch.int32 and n.is_cuda and y.dtype == torch.float32
    assert n.tolist() == n_f.tolist() == ref['n_out']
    assert [rs.n_out(ln, c) for ln, c in zip(ref['lens'], ref['choice'] or [0] * len(ref['lens']))] == ref['n_out']
    assert torch.equal(y, y_f), 'int16 and float32 samples must give the same bits'
    got = y.cpu().double().numpy()
    assert got.shape == ref['oracle'].shape, (got.shape, ref['oracle'].shape)
    err = np.abs(got - ref['oracle'])
    ratio = float((err / np.maximum(ref['limit'], 1e-300)).max())
    print(f'{case}: max |err| {err.max():.3e}, at {ratio:.3f} of the limit (float32 restatement {ref["ratio32"]:.3f})')
    assert ref['ratio32'] <= 0.30
    assert np.isfinite(got).all() and (err <= ref['limit']).all(), (case, ratio)
    for b, m in enumerate(ref['n_out']):
        assert not got[b, m:].any(), f'padding of row {b} is not zero'
    if case == 'speed':
        assert torch.equal(y[1, :700], torch.tensor(x[1].astype(np.float32), device=cuda)), 'factor 1.0 is a bit copy'


def test_speed_perturb(cuda, reference):
    from srf_amd import resample
    ref = reference['speed']
    sp = resample.SpeedPerturb(seed=7, device=cuda)
    assert sp.resampler.rates_in == [14400, 16000, 17600]
    x, lens = torch.tensor(ref['samples'], device=cuda), torch.tensor(ref['lens'], device=cuda)
    y, n, choice = sp(x, lens, step=3)
    y2, n2, choice2 = sp(x, lens, step=3)
    want, want_n = sp.resampler(x, lens, choice)
    assert choice.tolist() == choice2.tolist() == sp.draw(4, 3).tolist()
    assert torch.equal(y, y2) and torch.equal(y, want) and n.tolist() == n2.tolist() == want_n.tolist()
    assert any(sp.draw(4, s).tolist() != choice.tolist() for s in range(4, 8)), 'the draw must depend on the step'
    for b, c in enumerate(choice.tolist()):
        assert int(n[b]) == sp.resampler.n_out(ref['lens'][b], c)
        if c == 1:
            assert torch.equal(y[b, :ref['lens'][b]], x[b, :ref['lens'][b]].float())


def _stream(rs, x, lens, chunks, declare_last=True):
    """Push x [B, N] in ``chunks``, declaring each stream's end with the chunk it lies in
    (declare_last=False: a stream as long as everything pushed is left to finish())."""
    from srf_amd import resample
    B, N = x.shape
    assert sum(chunks) == N
    s = resample.ResampleStream(rs, B, max(chunks))
    outs, pos, declared = [], 0, [False] * B
    for n in chunks:
        ended = [-1] * B
        for b, ln in enumerate(lens):
            if not declared[b] and pos <= ln <= pos + n and (ln < N or declare_last):
                ended[b], declared[b] = ln, True
        outs.append(s.push(x[:, pos:pos + n], ended))
        pos += n
        assert s.out_done == sum(o.shape[1] for o in outs)
        assert s._tail <= s._taps - 1 or all(declared)
    outs.append(s.finish())
    return torch.cat(outs, dim=1)


CHUNKINGS = {
    '44k': [[1403], [441, 441, 441, 80], [1, 33, 34, 500, 835], [5, 436, 962]],
    '8k': [[333], [1] * 14 + [319], [1, 5, 6, 300, 21], [100, 233]],
}


@pytest.mark.parametrize('case', list(CHUNKINGS))
def test_chunk_invariance(cuda, reference, case):
    """The concatenated ResampleStream output is the offline output bit for bit for every
    chunking: a single chunk, 1-sample chunks, chunks shorter than the filter, chunks that
    complete no output.  The short streams end inside a chunk or at a chunk's end, the long
    one at the last chunk's end or (last chunking) at finish()."""
    from srf_amd import resample
    ref = reference[case]
    rs = resample.Resampler(ref['rates'][0], device=cuda)
    for dtype in (torch.int16, torch.float32):
        x = torch.tensor(ref['samples'], device=cuda).to(dtype)
        want, n = rs(x, torch.tensor(ref['lens'], device=cuda))
        assert n.tolist() == ref['n_out']
        for i, chunks in enumerate(CHUNKINGS[case]):
            got = _stream(rs, x, ref['lens'], chunks, declare_last=i < len(CHUNKINGS[case]) - 1)
            assert got.shape == want.shape, (chunks, got.shape, want.shape)
            assert torch.equal(got, want), (chunks, float((got - want).abs().max()))
    err = np.abs(want.cpu().double().numpy() - ref['oracle'])
    assert (err <= ref['limit']).all()


def test_push_audio_resampled_end_to_end(cuda):
    """c2_mini behind a 48 kHz resampler and the front end: the logits are, bit for bit, those
    of a second router without a resampler fed the offline-resampled audio in the chunks the
    first one handed to its FbankStream; the greedy hypotheses are equal.  Stream 1 (12 000
    samples, 4000 at 16 kHz, 23 frames) ends inside a chunk, stream 0 (18 711, 6237, 37
    frames) at finish()."""
    from srf_amd import fbank, resample
    from srf_amd.sequence_router import SequenceRouter
    from srf_amd.streaming import StreamingRouter
    kw, sh, P, _ = load_model_fixture('c2_mini')
    model = SequenceRouter(config_from_shape(kw), None, sh.class_n, device=cuda)
    model.load_params(P)
    mean = np.concatenate([np.full(41, 12.0), np.zeros(82)])
    std = np.concatenate([np.full(41, 4.0), np.ones(82)])
    fe = fbank.Fbank(cmvn=(mean, std), device=cuda)
    rs = resample.Resampler(48000, device=cuda)
    lens = [18711, 12000]
    x = torch.tensor(_batch(R.signal_wide, lens), device=cuda)

    plain = StreamingRouter(model, 2, max_chunk=16, frontend=fe)
    assert plain.lookahead_audio_ms == 65 and isinstance(plain.lookahead_audio_ms, int) and plain._rs is None
    s = StreamingRouter(model, 2, max_chunk=16, frontend=fe, resampler=rs)
    bound = s.audio_bound
    assert bound == (1280 - 6) * 3 and abs(s.lookahead_audio_ms - (65 + 6000 / (0.99 * 16000))) < 1e-9
    chunks = [bound, 1, 1199, 3000, bound, bound, 3045]
    assert sum(chunks) == lens[0]
    with pytest.raises(ValueError, match=str(bound)):
        s.push_audio(x[:, :bound + 1])
    calls, fe_push = [], s._fe.push

    def recording_push(samples, ended=None):
        calls.append((samples.clone(), ended))
        return fe_push(samples, ended)
    s._fe.push = recording_push
    outs, pos = [], 0
    for n in chunks:
        ended = [-1, lens[1]] if pos <= lens[1] < pos + n else None
        outs.append(s.push_audio(x[:, pos:pos + n], ended))
        pos += n
    outs.append(s.finish())
    logits = torch.cat([o.logits for o in outs], dim=1)
    labels = [sum((o.labels[b] for o in outs), []) for b in range(2)]

    offline, n16 = rs(x, torch.tensor(lens, device=cuda))
    assert n16.tolist() == [6237, 4000] and fbank.n_frames(n16.tolist()) == [37, 23]
    assert len(calls) == len(chunks) + 1 and max(c.shape[1] for c, _ in calls) <= 1280
    assert torch.equal(torch.cat([c for c, _ in calls], dim=1), offline)
    assert [e for _, e in calls if e is not None] == [[-1, 4000], [6237, -1]]
    ref_outs, pos = [], 0
    for samples, ended in calls:
        n = samples.shape[1]
        ref_outs.append(plain.push_audio(offline[:, pos:pos + n].contiguous(), ended))
        pos += n
    ref_outs.append(plain.finish())
    ref_logits = torch.cat([o.logits for o in ref_outs], dim=1)
    torch.cuda.synchronize()
    assert logits.shape == ref_logits.shape == (2, 10, sh.class_n)
    assert torch.equal(logits, ref_logits), float((logits - ref_logits).abs().max())
    assert s.hypotheses == plain.hypotheses == labels
    with pytest.raises(ValueError):
        s.push_audio(x[:, :160])
    s.reset()
    assert s.push_audio(x[:, :bound]).logits.shape[1] == 0


def test_errors(cuda):
    from srf_amd import fbank, resample
    from srf_amd.streaming import StreamingRouter
    for bad in (3999, 192001, [8000] * 9, [], 16000.5):
        with pytest.raises(ValueError):
            resample.Resampler(bad, device=cuda)
    with pytest.raises(ValueError):
        resample.Resampler(48000, rate_out=1000, device=cuda)
    with pytest.raises(ValueError, match='1048576'):
        resample.Resampler(191999, 192000, device=cuda)
    with pytest.raises(ValueError):
        resample.SpeedPerturb(factors=(0.1, 1.0), device=cuda)   # 1600 Hz
    bank = resample.Resampler([14400, 16000, 17600], device=cuda)
    x = torch.zeros((2, 64), dtype=torch.int16, device=cuda)
    n = torch.tensor([64, 10], device=cuda)
    for choice in ([0, 3], [-1, 0], [0], torch.tensor([0, 1, 2])):
        with pytest.raises(ValueError):
            bank(x, n, choice)
    with pytest.raises(ValueError):
        bank.n_out(10, 3)
    for samples, lens in [(x.double(), n), (x[0], n), (x.cpu(), n), (x, n[:1]), (x.cpu().numpy(), n)]:
        with pytest.raises(ValueError):
            bank(samples, lens)
    with pytest.raises(ValueError):
        resample.ResampleStream(bank, 2, 64)          # several rates in one stream
    one = resample.Resampler(48000, device=cuda)
    s = resample.ResampleStream(one, 2, 64)
    for samples in (x.new_zeros((2, 65)), x.cpu(), x.double(), x[:1], x[0]):
        with pytest.raises(ValueError):
            s.push(samples)
    with pytest.raises(ValueError):
        s.push(x, [65, -1])                            # an end beyond the chunk
    assert s.pushed == 0 and s.out_done == 0           # a refused push advances nothing
    f = one.filters[0]
    assert s.push(x).shape == (2, resample.stream_final(64, f['first'], f['taps'], f['iu'])) == (2, 16)
    kw, sh, P, _ = load_model_fixture('c2_mini')
    from srf_amd.sequence_router import SequenceRouter
    model = SequenceRouter(config_from_shape(kw), None, sh.class_n, device=cuda)
    with pytest.raises(ValueError):
        StreamingRouter(model, 2, max_chunk=16, resampler=one)                       # no front end
    with pytest.raises(ValueError):
        StreamingRouter(model, 2, max_chunk=16, frontend=fbank.Fbank(device=cuda),
                        resampler=resample.Resampler(48000, 8000, device=cuda))      # not 16 kHz
