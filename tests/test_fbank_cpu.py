"""Waveform front end, the parts that need no GPU: the framing rule, the oracle
(tests/fbank_ref.py) pinned by anchor values, the kernels' host-built tables against it,
argument validation of the streaming entry points, the C ABI binding and the CMVN file
format (srf_amd/fbank.py)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import fbank_ref as R

LOG_EPS = -15.942385


def test_framing_rule():
    from srf_amd import _lib, fbank
    for n, t in [(0, 0), (399, 0), (400, 1), (559, 1), (560, 2), (2237, 12)]:
        assert fbank.n_frames(n) == t and R.n_frames(n) == t and _lib.lib().srf_fbank_num_frames(n) == t
    assert fbank.n_frames([399, 400, 559, 560]) == [0, 1, 1, 2]
    assert fbank.n_frames(torch.tensor([399, 400, 559, 560])).tolist() == [0, 1, 1, 2]


def _mel_checks(w):
    for f, lo, hi, total in [(0, 1, 3, 1.594219), (39, 225, 255, 15.915928)]:
        nz = np.nonzero(w[f])[0]
        assert (nz[0], nz[-1]) == (lo, hi) and len(nz) == hi - lo + 1
        assert abs(w[f].sum() - total) < 1e-6
    assert not w[:, 0].any()
    assert (w != 0).sum(axis=0).max() == 2


def test_mel_filterbank_oracle():
    _mel_checks(R.mel_weights())


def test_tables_match_oracle():
    """The tables the kernels read (host, double, rounded once) are the oracle's to one
    float32 rounding."""
    from srf_amd import fbank
    tb = fbank.tables()
    w = np.zeros((R.N_MEL, R.N_BINS))
    for f in range(R.N_MEL):
        lo, n = tb['mel_first'][f], tb['mel_count'][f]
        w[f, lo:lo + n] = tb['mel_weights'][f, :n]
        assert not tb['mel_weights'][f, n:].any()
    _mel_checks(w)
    assert np.array_equal(w.astype(np.float32), R.mel_weights().astype(np.float32))
    assert np.array_equal(tb['window'], R.povey_window().astype(np.float32))
    k = np.arange(256) * 2.0 * np.pi / 512
    assert np.array_equal(tb['twiddle'], np.stack([np.cos(k), -np.sin(k)], axis=1).astype(np.float32))


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_silence_and_dc_hit_the_floor(dtype):
    for x in (np.zeros(800), np.full(800, 1234.0)):
        s = R.static(x, dtype)
        assert s.shape == (3, 41) and s.dtype == dtype
        assert np.abs(s - LOG_EPS).max() < 1e-6


ANCHORS_STATIC = [(0, 0, 20.115505882), (0, 1, 14.403634260), (0, 2, 14.800281971), (0, 20, 19.435629932),
                  (0, 40, 23.210100663), (11, 0, 20.113771291), (11, 1, 13.795509095), (11, 40, 23.105262997)]
ANCHORS_FEATS = [(0, 41, -0.012880174), (0, 42, -0.415530115), (0, 82, -0.002898025), (0, 83, -0.097677573),
                 (0, 122, -0.007854749), (5, 42, -0.520349567), (5, 83, 0.016067247), (11, 41, 0.018195315),
                 (11, 82, -0.006868699), (11, 122, -0.013413629)]


def test_oracle_anchors():
    i = np.arange(2237, dtype=np.int64)
    x = (7 * i * i + 13 * i) % 4001 - 1900
    assert np.array_equal(x, R.signal_noise(2237))
    st, f = R.static(x), R.features(x)
    assert st.shape == (12, 41) and f.shape == (12, 123)
    for t, d, v in ANCHORS_STATIC:
        assert abs(st[t, d] - v) < 1e-6, (t, d, st[t, d], v)
    for t, d, v in ANCHORS_FEATS:
        assert abs(f[t, d] - v) < 1e-6, (t, d, f[t, d], v)
    assert np.array_equal(f[:, :41], st)


def test_oracle_float32_is_close_and_cmvn_formula():
    x = R.signal_noise(2237)
    a, b = R.features(x), R.features(x, dtype=np.float32)
    assert b.dtype == np.float32 and 0 < np.abs(a - b).max() < 1e-4
    mean, std = np.linspace(-1, 1, 123), np.linspace(0.5, 2, 123)
    assert np.allclose(R.features(x, mean, std), (a - mean + 1e-14) / (std + 1e-14), rtol=0, atol=1e-12)
    assert R.static(R.signal_wide(400 + 160 * 36 + 77))[:, 1:].min() > 8.4


def test_fbank_stream_ended_validation():
    """FbankStream.push validates ``ended`` as StreamingRouter.push does, in samples, before
    anything runs (so a CPU-resident state serves to show it)."""
    from srf_amd import fbank
    fe = fbank.Fbank(device='cpu')
    s = fbank.FbankStream(fe, 3, 1000)
    x = torch.zeros((3, 500), dtype=torch.int16)
    for bad in ([-1, -1], [-1, -2, -1], [-1, 501, -1]):
        with pytest.raises(ValueError):
            s.push(x, bad)
    with pytest.raises(ValueError):
        s.push(torch.zeros((3, 1001), dtype=torch.int16))
    with pytest.raises(ValueError):
        s.push(torch.zeros((2, 10), dtype=torch.int16))
    with pytest.raises(ValueError, match='HIP device'):
        s.push(x, [-1, 500, 0])            # valid: refused only because there is no CPU path
    assert s.pushed == 0 and s.lengths == [None] * 3
    with pytest.raises(ValueError):
        fbank.FbankStream(fe, 0, 1000)
    with pytest.raises(ValueError):
        fbank.Fbank(dither=-1.0, device='cpu')
    with pytest.raises(ValueError):
        fbank.Fbank(cmvn=(np.zeros(123), np.ones(122)), device='cpu')
    with pytest.raises(ValueError):
        fbank.FbankStream(fbank.Fbank(cmvn=(np.zeros((2, 123)), np.ones((2, 123))), device='cpu'), 3, 1000)


def test_sample_domain_ended_and_push_audio_bound():
    from srf_amd import streaming
    lens = streaming.check_ended([None, None], [-1, 2237], 2000, 400, unit='samples')
    assert lens == [None, 2237]
    with pytest.raises(ValueError, match='samples 2400 .. 2800'):
        streaming.check_ended(lens, [2399, -1], 2400, 400, unit='samples')
    with pytest.raises(ValueError, match='already declared'):
        streaming.check_ended(lens, [-1, 2500], 2400, 400, unit='samples')
    # n samples complete at most n // 160 + 1 frames, the flush adds 4, 3 may be waiting
    for max_chunk in (12, 16, 64):
        bound = streaming.audio_chunk_bound(max_chunk)
        assert bound == 160 * (max_chunk - 8) and bound // 160 + 8 <= max_chunk
        streaming.check_audio_chunk(bound, max_chunk)
        with pytest.raises(ValueError, match=str(bound)):
            streaming.check_audio_chunk(bound + 1, max_chunk)


def test_lib_signatures_and_argument_checks():
    from srf_amd import _lib
    L = _lib.lib()
    sig = _lib._SIGNATURES
    for name in ('srf_fbank_num_frames', 'srf_fbank_table_floats', 'srf_fbank_tables', 'srf_fbank_static',
                 'srf_fbank_deltas', 'srf_fbank_stats'):
        assert name in sig and hasattr(L, name)
    assert len(sig['srf_fbank_static'][1]) == 17 and sig['srf_fbank_static'][1][13] is ctypes.c_float
    assert len(sig['srf_fbank_deltas'][1]) == 15 and len(sig['srf_fbank_stats'][1]) == 7
    one = ctypes.c_void_p(16)   # never dereferenced: every call below is refused before any launch
    # frame 0 starts before the buffer's first sample
    assert L.srf_fbank_static(one, 1, one, one, 1, 800, 800, 160, 960, 0, 1, 0, 1, 0.0, 0, one, None) == -1
    assert b'before the buffer' in L.srf_last_error()
    # n_limit beyond the buffer
    assert L.srf_fbank_static(one, 1, one, one, 1, 800, 800, 0, 801, 0, 1, 0, 1, 0.0, 0, one, None) == -1
    # frames outside the statics buffer
    assert L.srf_fbank_static(one, 1, one, one, 1, 800, 800, 0, 800, 0, 3, 0, 2, 0.0, 0, one, None) == -1
    assert L.srf_fbank_static(one, 1, one, one, 1, 800, 800, 0, 800, 0, 3, 0, 3, -1.0, 0, one, None) == -1
    # deltas: statics frames outside the statics buffer, bad cmvn_rows
    assert L.srf_fbank_deltas(one, one, 2, 4, 0, 12, 0, 4, None, None, 0, one, 4, 0, None) == -1
    assert b'statics buffer' in L.srf_last_error()
    assert L.srf_fbank_deltas(one, one, 3, 12, 0, 12, 0, 4, one, one, 2, one, 4, 0, None) == -1
    assert L.srf_fbank_stats(one, one, 0, 4, 123, one, None) == -1
    assert L.srf_fbank_tables(None, 0) == -1


def test_cmvn_file_round_trip(tmp_path):
    from srf_amd import fbank
    rng = np.random.default_rng(3)
    mean, std = rng.standard_normal(123) * 7, rng.random(123) + 0.1
    path = str(tmp_path / 'cmvn_spk_abc.txt')
    fbank.save_cmvn(path, mean, std)
    m = np.loadtxt(path)                   # what misc_helper.load_cmvn reads
    assert m.shape == (2, 123) and np.array_equal(m[0], mean) and np.array_equal(m[1], std)
    a, b = fbank.load_cmvn(path)
    assert np.array_equal(a, mean) and np.array_equal(b, std)
    st = fbank.CmvnStats(device='cpu')
    st.sums[:123] = torch.tensor(mean * 10)
    st.sums[123:246] = torch.tensor((std ** 2 + mean ** 2) * 10)
    st.sums[246] = 10
    path2 = str(tmp_path / 'cmvn2.txt')
    st.save(path2)
    assert np.allclose(np.loadtxt(path2), np.stack([mean, std]), rtol=1e-9, atol=1e-9)
