"""Resampler without a device: the host tables against the numpy restatement, the output
count, anchors of the oracle itself, the streaming count rule and the refusals
(srf_amd/resample.py, csrc/resample.hip)."""
import ctypes

import numpy as np
import pytest

from tests import resample_ref as R

# fin -> fout: (iu, ou, taps), checked with a numpy prototype when the filter was specified
SHAPES = {(48000, 16000): (3, 1, 37), (44100, 16000): (441, 160, 34), (8000, 16000): (1, 2, 13),
          (14400, 16000): (9, 10, 13), (17600, 16000): (11, 10, 14)}


def _ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize('fin,fout', list(SHAPES) + [(15999, 16000), (16000, 16000), (192000, 4000)])
def test_tables_match_oracle(fin, fout):
    from srf_amd import resample
    f = R.Filter(fin, fout)
    flat, (t,) = resample.tables(fin, fout)
    assert (t['iu'], t['ou'], t['taps']) == (f.iu, f.ou, f.taps)
    if (fin, fout) in SHAPES:
        assert (f.iu, f.ou, f.taps) == SHAPES[(fin, fout)]
    assert t['first'].tolist() == f.first.tolist()
    assert t['w'].dtype == np.float32 and t['w'].shape == f.w.shape
    err = np.abs(t['w'].astype(np.float64) - f.w)
    assert (err <= _ulp32(f.w)).all(), float((err / _ulp32(f.w)).max())
    assert flat[0] == 1 and flat[1] == fout and flat.size == 8 + 64 + f.ou * (1 + f.taps)
    if fin == fout:
        assert t['taps'] == 1 and t['first'].tolist() == [0] and t['w'].tolist() == [[1.0]]


def test_bank_layout_and_44100_first_range():
    from srf_amd import resample
    rates = [14400, 16000, 17600]
    flat, per = resample.tables(rates, 16000)
    assert flat[0] == 3 and [int(flat[8 + 8 * r + 5]) for r in range(3)] == rates
    for t, fin in zip(per, rates):
        f = R.Filter(fin, 16000)
        assert (t['iu'], t['ou'], t['taps']) == (f.iu, f.ou, f.taps) and t['first'].tolist() == f.first.tolist()
    f = R.Filter(44100, 16000)
    assert (int(f.first.min()), int(f.first.max())) == (-16, 422)


@pytest.mark.parametrize('fin,fout', list(SHAPES))
def test_n_out(fin, fout):
    from srf_amd import _lib, resample
    f = R.Filter(fin, fout)
    L = _lib.lib()
    lens = [0, 1, f.iu - 1, f.iu, f.iu + 1, 7 * f.iu + 3, 2 ** 31 - 1, 2 ** 40]
    for n in lens:
        want = -((-n * f.ou) // f.iu)
        # every o with o / fout < n / fin
        assert (want - 1) * f.iu < n * f.ou <= want * f.iu or n == want == 0
        assert f.n_out(n) == resample.n_out(n, fin, fout) == L.srf_resample_num_out(n, fin, fout) == want
    assert resample.n_out(lens[:6], fin, fout) == [f.n_out(n) for n in lens[:6]]
    import torch
    assert resample.n_out(torch.tensor(lens), fin, fout).tolist() == [f.n_out(n) for n in lens]
    assert f.n_out(f.iu) == f.ou


def test_oracle_anchors():
    """DC gain (Kaldi's is 1.0005 too), a 1 kHz tone through 48 -> 16 kHz keeps its amplitude
    away from the edges, a 12 kHz tone (beyond the 7.92 kHz cutoff) comes out 50 dB down."""
    for fin, fout in SHAPES:
        f = R.Filter(fin, fout)
        gain = f.w.sum(axis=1)
        print(f'{fin} -> {fout}: DC gain {gain.min():.6f} .. {gain.max():.6f}')
        assert np.abs(gain - 1.0).max() <= 1e-3
        y = R.resample(f, np.full(40 * f.iu + 400, 1000.0))
        assert np.abs(y[60:-60] - 1000.0).max() <= 1.0
    f = R.Filter(48000, 16000)
    n = np.arange(4800)
    y = R.resample(f, 10000.0 * np.sin(2 * np.pi * 1000.0 * n / 48000.0))
    want = 10000.0 * np.sin(2 * np.pi * 1000.0 * np.arange(y.size) / 16000.0)
    err = np.abs(y - want)[20:-20].max()
    print(f'1 kHz tone: max |err| / amplitude {err / 10000.0:.2e}')
    assert y.size == 1600 and err <= 1e-3 * 10000.0
    y = R.resample(f, 10000.0 * np.sin(2 * np.pi * 12000.0 * n / 48000.0 + 0.3))
    down = 20 * np.log10(np.abs(y[20:-20]).max() / 10000.0)
    print(f'12 kHz tone: {down:.1f} dB')
    assert down <= -50.0


def test_oracle_float32_is_close():
    """The float32 restatement stays within 0.30 of the rounding limit (taps + 2) 2^-24 sum |w x|."""
    worst = 0.0
    for fin, fout in SHAPES:
        f = R.Filter(fin, fout)
        x = R.signal_wide(1500)
        y64, y32, bd = R.resample(f, x), R.resample(f, x, np.float32), R.bound(f, x)
        ratio = (np.abs(y32.astype(np.float64) - y64) / ((f.taps + 2) * 2.0 ** -24 * np.maximum(bd, 1e-30))).max()
        print(f'{fin} -> {fout}: float32 restatement at {ratio:.3f} of the limit')
        worst = max(worst, ratio)
    assert worst <= 0.30


@pytest.mark.parametrize('fin,fout', list(SHAPES))
def test_stream_count_rule(fin, fout):
    from srf_amd import resample
    f = R.Filter(fin, fout)
    (t,) = resample.tables(fin, fout)[1]
    hold = resample.stream_hold(t['first'], t['taps'], t['iu'])
    prev, held = 0, 0
    for pushed in range(3 * f.iu + 201):
        got = resample.stream_final(pushed, t['first'], t['taps'], t['iu'])
        assert got == R.stream_final_brute(f, pushed), pushed
        assert prev <= got <= f.n_out(pushed), pushed
        tail = resample.stream_tail(pushed, got, t['first'], t['iu'])
        assert 0 <= tail <= min(pushed, f.taps - 1), (pushed, tail)
        held = max(held, f.n_out(pushed) - got)
        prev = got
    print(f'{fin} -> {fout}: holds back {held} outputs at the most (bound {hold})')
    assert held <= hold <= 13


def test_refusals():
    from srf_amd import _lib, resample
    L = _lib.lib()

    def floats(rates, out=16000):
        return L.srf_resample_table_floats((ctypes.c_int * len(rates))(*rates), len(rates), out)
    assert floats([3999]) == 0 and b'3999' in L.srf_last_error()
    assert floats([192001]) == 0 and floats([16000], 3999) == 0
    assert floats([191999], 192000) == 0 and b'more than 1048576' in L.srf_last_error()
    assert floats([8000] * 9) == 0 and b'1 .. 8' in L.srf_last_error()
    assert floats([8000] * 8) == 8 + 64 + 8 * 2 * 14
    buf = np.empty(16, dtype=np.float32)
    arr = (ctypes.c_int * 1)(48000)
    assert L.srf_resample_tables(arr, 1, 16000, buf.ctypes.data_as(ctypes.c_void_p), 16) == -1
    assert b'need a host buffer' in L.srf_last_error()
    assert L.srf_resample_num_out(10, 3999, 16000) == 0 and b'3999' in L.srf_last_error()
    for bad in ([3999], [8000] * 9, [], 16000.5, [True]):
        with pytest.raises(ValueError):
            resample.tables(bad, 16000)
    with pytest.raises(ValueError, match='1048576'):
        resample.tables(191999, 192000)
    # the launch refuses before touching the device: a tap below a buffer that starts late, bad ranges
    for kw, msg in [(dict(s0=5, o0=0), b'before the buffer'), (dict(o0=9, o1=3), b'bad output range'),
                    (dict(n_limit=99), b'beyond the buffer'), (dict(q0=4), b'outside the output buffer'),
                    (dict(B=0), b'1 <= B'), (dict(rate_in=3999), b'3999')]:
        assert L.srf_resample(*_launch_args(**kw)) == -1 and msg in L.srf_last_error(), (kw, L.srf_last_error())


def _launch_args(B=1, s0=0, width=64, n_limit=64, o0=0, o1=8, q0=0, rate_in=48000):
    """srf_resample arguments with non-null dummy pointers that a refused call never reads."""
    p = ctypes.c_void_p(64)
    return [p, 1, p, None, p, (ctypes.c_int * 1)(rate_in), 1, 16000, B, 64, width, s0, n_limit, o0, o1, p, 32, q0, None,
            None]


def test_speed_perturb_draw_and_router_bound():
    from srf_amd import resample, streaming
    # the draw is a host function of (seed, step, B)
    g = resample.SpeedPerturb.draw
    sp = type('S', (), {'seed': 3, 'factors': [0.9, 1.0, 1.1]})()
    a, b, c = g(sp, 64, 5), g(sp, 64, 5), g(sp, 64, 6)
    assert a.tolist() == b.tolist() != c.tolist() and set(a.tolist()) == {0, 1, 2}
    (t,) = resample.tables(48000, 16000)[1]
    hold = resample.stream_hold(t['first'], t['taps'], t['iu'])
    assert hold == 6
    bound = streaming.resampled_chunk_bound(16, t['iu'], t['ou'], hold)
    assert bound == (1280 - 6) * 3
    # a chunk at the bound cannot make more than audio_chunk_bound outputs, one more sample can
    assert R.Filter(48000, 16000).n_out(bound) + hold <= 1280 < R.Filter(48000, 16000).n_out(bound + 3) + hold
