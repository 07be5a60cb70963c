"""The sliding-window CMVN without a device: hand-computed anchors for
the float64 oracle of tests/cmvn_ref.py, its conditioning on the inputs of
tests/test_cmvn_gpu.py, and the host-side logic of srf_amd/fbank.py that needs no kernel
(argument errors, state sizes, the history's slide schedule)."""
import numpy as np
import pytest
import torch

from tests import cmvn_ref as R

X5 = np.array([[1, 10], [2, 20], [4, 10], [7, 40], [5, 0]], dtype=np.float64)


def test_anchor_mean_only():
    """W = 3 on 5 frames, 2 dimensions: the window means are 1, 3/2, 7/3, 13/3, 16/3 and
    10, 15, 40/3, 70/3, 50/3."""
    y, last = R.stream(X5, 3, norm_vars=False)
    want = np.array([[0, 0], [1 / 2, 5], [5 / 3, -10 / 3], [8 / 3, 50 / 3], [-1 / 3, -50 / 3]])
    assert np.abs(y - want).max() <= 1e-14
    assert y[0, 0] == 0.0 and y[0, 1] == 0.0
    m, q, k = last
    assert np.allclose(m, [16 / 3, 50 / 3], rtol=1e-15) and np.allclose(q, [30, 1700 / 3], rtol=1e-15) and k == 3


def test_anchor_with_variance():
    """The same input: the window variances q - m^2 are 0 (floored at 1e-10), 1/4, 14/9, 38/9,
    14/9 and 0, 25, 200/9, 1400/9, 2600/9."""
    y, _ = R.stream(X5, 3, norm_vars=True)
    want = np.array([[0, 0], [1, 1], [5 / np.sqrt(14), -1 / np.sqrt(2)], [8 / np.sqrt(38), 50 / np.sqrt(1400)],
                     [-1 / np.sqrt(14), -50 / np.sqrt(2600)]])
    assert np.abs(y - want).max() <= 1e-13
    assert y[0, 0] == 0.0 and y[0, 1] == 0.0


def test_prior_schedule_and_carry():
    """W = 5, prior (mean 0, std 1) worth 2 frames, six frames of 3: c = 2, 2, 2, 1, 0, 0, so
    m = 3 n / (n + c) = 1, 3/2, 9/5, 12/5, 3, 3.  The last frame leaves m = 3, q = 9,
    n + c = 5; carried with speaker_frames = 4 that is the prior (3, 0, 4) of the next
    utterance [5, 5]: m = (5 + 4 * 3) / 5 and (10 + 3 * 3) / 5."""
    x = np.full((6, 1), 3.0)
    prior = (np.zeros(1), np.ones(1), 2.0)
    y, last = R.stream(x, 5, norm_vars=False, prior=prior)
    assert np.abs(y[:, 0] - [2, 1.5, 1.2, 0.6, 0, 0]).max() <= 1e-15
    yv, _ = R.stream(x, 5, norm_vars=True, prior=prior)
    assert abs(yv[0, 0] - 2 / np.sqrt(11 / 3 - 1)) <= 1e-15      # q = (9 + 2 (1 + 0)) / 3
    assert last[0][0] == 3.0 and last[1][0] == 9.0 and last[2] == 5.0

    mean, std, count = R.carry([last, None], (np.zeros(1), np.ones(1), 2.0), 4, 2, 1)
    assert mean.tolist() == [[3.0], [0.0]] and std.tolist() == [[0.0], [1.0]] and count.tolist() == [4.0, 2.0]
    x2 = np.full((2, 2, 1), 5.0)
    y2, lasts = R.batch(x2, [2, 0], 5, norm_vars=False, prior=(mean, std, count))
    assert np.abs(y2[0, :, 0] - [1.6, 1.2]).max() <= 1e-15 and not y2[1].any() and lasts[1] is None
    y2v, _ = R.batch(x2, [2, 0], 5, norm_vars=True, prior=(mean, std, count))
    assert abs(y2v[0, 0, 0] - 2.0) <= 1e-13                      # q = (25 + 4 * 9) / 5, v = 0.64
    # without a stream's own frames the old prior stays, with no prior at all the count is 0
    assert R.carry([None], None, 4, 1, 1)[2].tolist() == [0.0]


def test_exact_zeros_of_the_definition():
    """No prior: frame 0, a column that is constant over the window, and everything with
    W = 1 come out as exactly 0."""
    x = R.features(1, 40, 7, seed=9)[0].astype(np.float64)
    x[:, 3] = np.float32(-15.9424)
    for nv in (True, False):
        y, _ = R.stream(x, 16, norm_vars=nv)
        assert not y[0].any() and not y[:, 3].any() and y[1:, :3].all()
        assert not R.stream(x, 1, norm_vars=nv)[0].any()


@pytest.mark.parametrize('name', sorted(R.SHAPES))
def test_oracle_is_well_conditioned(name):
    """On the GPU test's inputs the oracle summed in ascending and in descending order
    agrees within 0.5 u, u = 2^-24 max(1, |y|): the order of the fp64 sums cannot decide a
    comparison at 4 u."""
    c = R.case(name)
    prior = None if c['prior'] is None else c['prior'] + (c['prior_frames'],)
    worst = 0.0
    for nv in (True, False):
        up, _ = R.batch(c['x'], c['lens'], c['window'], nv, prior)
        down, _ = R.batch(c['x'], c['lens'], c['window'], nv, prior, descending=True)
        assert np.isfinite(up).all()
        worst = max(worst, float((np.abs(up - down) / R.unit(up)).max()))
    print(f'{name}: ascending against descending sums: {worst:.2e} u')
    assert worst <= 0.5


def test_argument_errors():
    from srf_amd import fbank
    for w in (0, 4097, -3, 2.5):
        with pytest.raises(ValueError, match='window'):
            fbank.SlidingCmvn(window=w, device='cpu')
    fbank.SlidingCmvn(window=1, device='cpu'), fbank.SlidingCmvn(window=4096, device='cpu')
    for dim in (0, 129):
        with pytest.raises(ValueError, match='dim'):
            fbank.SlidingCmvn(dim=dim, device='cpu')
    for prior in [(np.zeros(123), np.ones(122)), (np.zeros(122), np.ones(122)), (np.zeros((2, 3, 123)),) * 2,
                  (np.zeros((0, 123)), np.ones((0, 123)))]:
        with pytest.raises(ValueError, match='prior'):
            fbank.SlidingCmvn(prior=prior, device='cpu')
    std = np.ones(123)
    std[7] = 0.0
    with pytest.raises(ValueError, match='positive'):
        fbank.SlidingCmvn(prior=(np.zeros(123), std), device='cpu')
    with pytest.raises(ValueError, match='positive'):
        fbank.SlidingCmvn(prior=(np.zeros(123), -np.ones(123)), device='cpu')
    with pytest.raises(ValueError, match='prior_frames'):
        fbank.SlidingCmvn(prior_frames=-1, device='cpu')

    sc = fbank.SlidingCmvn(window=16, device='cpu')
    x = torch.zeros((2, 5, 123))
    with pytest.raises(ValueError, match='>= 0'):
        sc(x, [3, -1])
    with pytest.raises(ValueError, match='entries'):
        sc(x, [3])
    with pytest.raises(ValueError, match='float32'):
        sc(x.double(), [3, 3])
    with pytest.raises(ValueError, match='float32'):
        sc(torch.zeros((2, 5, 100)), [3, 3])
    with pytest.raises(ValueError, match='HIP device'):
        sc(x, [3, 5])
    rows = fbank.SlidingCmvn(prior=(np.zeros((2, 123)), np.ones((2, 123))), device='cpu')
    assert rows.prior_rows(2) == 2 and sc.prior_rows(7) == 0
    assert fbank.SlidingCmvn(prior=(np.zeros(123), np.ones(123)), device='cpu').prior_rows(7) == 1
    with pytest.raises(ValueError, match='rows'):
        rows.prior_rows(3)
    with pytest.raises(ValueError, match='rows'):
        fbank.SlidingCmvnStream(rows, 3, 8)
    with pytest.raises(ValueError, match='>= 1'):
        fbank.SlidingCmvnStream(sc, 0, 8)

    s = fbank.SlidingCmvnStream(sc, 2, 4)
    with pytest.raises(ValueError, match='max_frames'):
        s.push(torch.zeros((2, 5, 123)))
    with pytest.raises(ValueError, match='float32'):
        s.push(torch.zeros((3, 4, 123)))
    with pytest.raises(ValueError, match='beyond'):
        s.push(torch.zeros((2, 4, 123)), [9, -1])
    with pytest.raises(ValueError, match='HIP device'):
        s.push(torch.zeros((2, 4, 123)))
    with pytest.raises(ValueError, match='sliding CMVN'):
        fbank.Fbank(cmvn=fbank.SlidingCmvn(dim=40, device='cpu'), device='cpu')
    with pytest.raises(ValueError, match='nothing to carry'):
        fbank.FbankStream(fbank.Fbank(device='cpu'), 2, 1000).reset(carry=True)


def test_state_sizes_and_front_end_wiring():
    from srf_amd import fbank
    assert (fbank.CMVN_TILE, fbank.CMVN_MAX_DIM, fbank.CMVN_MAX_WINDOW) == (32, 128, 4096)
    mean, std = R.prior_stats(123)
    sc = fbank.SlidingCmvn(window=600, prior=(mean, std), device='cpu')
    assert sc.mean.dtype == torch.float64 and sc.mean.shape == (1, 123) and sc.count.tolist() == [200.0]
    assert np.array_equal(sc.mean[0].numpy(), mean.astype(np.float64))
    s = fbank.SlidingCmvnStream(sc, 3, 20)
    assert s.history.shape == (3, 599 + 32 + 20, 123) and s.history.dtype == torch.float32
    assert s.last.shape == (3, 247) and s.last.dtype == torch.float64 and not s.last.any()
    assert s.prior_mean.shape == s.prior_std.shape == (3, 123) and s.prior_count.tolist() == [200.0] * 3
    assert np.array_equal(s.prior_std[2].numpy(), std.astype(np.float64))
    none = fbank.SlidingCmvnStream(fbank.SlidingCmvn(window=16, dim=5, device='cpu'), 2, 8)
    assert none.history.shape == (2, 15 + 32 + 8, 5) and none.prior_count.tolist() == [0.0, 0.0]

    fe = fbank.Fbank(cmvn=sc, device='cpu')
    assert fe.sliding is sc and fe.mean is None and fe.cmvn_rows(1) == 0 and fe.cmvn_rows(28) == 0
    assert fbank.Fbank(device='cpu').sliding is None
    fs = fbank.FbankStream(fe, 3, 1000)
    assert fs._cmvn.max_frames == 1000 // 160 + 1 + 4 and fs._cmvn.B == 3
    assert fbank.FbankStream(fbank.Fbank(cmvn=(mean, std), device='cpu'), 3, 1000)._cmvn is None


def test_abi_refusals():
    """srf_cmvn_sliding is bound as include/srf.h declares it and refuses, before any launch,
    what would read or write outside its buffers."""
    import ctypes
    from srf_amd import _lib
    L = _lib.lib()
    sig = _lib._SIGNATURES['srf_cmvn_sliding'][1]
    assert len(sig) == 19 and sig[8] is ctypes.c_void_p and sig[11] is ctypes.c_int and hasattr(L, 'srf_cmvn_sliding')
    one = ctypes.c_void_p(16)   # never dereferenced: every call below is refused before any launch

    def call(B=2, rows=100, D=123, f0=0, t0=0, t1=100, prior=None, prior_rows=0, W=16, To=100, o0=0, feats=one):
        return L.srf_cmvn_sliding(feats, one, B, rows, D, f0, t0, t1, prior, prior, prior, prior_rows, W, 1, one, To,
                                  o0, None, None)
    assert call(t1=0) == 0                                   # nothing to do is no error
    for kw, msg in [(dict(B=0), b'B'), (dict(D=0), b'D'), (dict(D=129), b'D'), (dict(W=0), b'window'),
                    (dict(W=4097), b'window'), (dict(t0=5, t1=4), b'frame range'), (dict(t0=-1), b'frame range'),
                    (dict(prior_rows=3, prior=one), b'prior_rows'), (dict(prior_rows=1), b'null'),
                    (dict(feats=None), b'null'),
                    (dict(To=99), b'output buffer'), (dict(o0=1), b'output buffer'),
                    (dict(rows=99), b'input buffer'),
                    # frames [40, 50) need the window of frame 32, frames 17 on: a buffer from 18 on is short
                    (dict(f0=18, t0=40, t1=50, rows=60, o0=40, To=10), b'input buffer')]:
        assert call(**kw) == -1, kw
        assert msg in L.srf_last_error(), (kw, L.srf_last_error())


@pytest.mark.parametrize('window', [1, 16, 600])
def test_history_slide_schedule(window):
    """After every chunk the history starts at the first frame that the window of the next
    frame's tile start reads, holds at most window - 1 frames plus one tile, and has room
    for the next chunk."""
    from srf_amd import fbank
    s = fbank.SlidingCmvnStream(fbank.SlidingCmvn(window=window, dim=2, device='cpu'), 1, 70)
    rng = np.random.default_rng(window)
    for m in [1, 31, 32, 33, 70] + rng.integers(1, 71, 60).tolist():
        assert s.pushed - s._f0 + m <= s.rows
        old_f0 = s._f0
        s.pushed += m
        hist, rows, shift, keep = s._slide()
        need = max(0, s.pushed // 32 * 32 - window + 1)
        assert hist is s.history and rows == s.rows and s._f0 == need and shift == need - old_f0 >= 0
        assert keep == s.pushed - need <= window - 1 + 31 and shift + keep <= rows
