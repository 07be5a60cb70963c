"""The MWER reference (tests/mwer_ref.py) on its own, without a device: its gradient is the
gradient of its loss (central finite differences), it agrees with torch's ctc_loss and
autograd in float64, a hand-computed case gives loss_ewerr's three terms, and the cases
defined to be exactly zero are.  Also the argument checks of srf_mwer_workspace /
srf_mwer_loss and srf_ctc_beam_nbest, which refuse before any launch and so run here.
"""
import ctypes
import math

import numpy as np
import pytest

from tests import beam_ref, mwer_ref


def _case(seed, T=7, C=5, n=4, Lmax=3):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((T, C))
    hyps = [rng.integers(0, C - 1, size=int(rng.integers(0, Lmax + 1))).tolist() for _ in range(n)]
    errs = rng.integers(0, 7, size=n).tolist()
    return x, hyps, errs


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_reference_gradient_is_the_gradient_of_its_loss(seed):
    x, hyps, errs = _case(seed)
    blank = x.shape[1] - 1
    r = mwer_ref.mwer(x, hyps, errs, blank, grad_scale=0.5)
    h = 1e-6
    fd = np.zeros_like(x)
    for t in range(x.shape[0]):
        for c in range(x.shape[1]):
            xp, xm = x.copy(), x.copy()
            xp[t, c] += h
            xm[t, c] -= h
            fd[t, c] = 0.5 * (mwer_ref.mwer(xp, hyps, errs, blank)['loss']
                              - mwer_ref.mwer(xm, hyps, errs, blank)['loss']) / (2 * h)
    assert np.abs(r['w'].sum()) < 1e-12
    assert np.abs(r['grad'].sum(axis=1)).max() < 1e-12
    assert np.abs(fd - r['grad']).max() < 1e-8, np.abs(fd - r['grad']).max()


@pytest.mark.parametrize('seed', [3, 4])
def test_reference_agrees_with_torch_ctc_loss_in_float64(seed):
    import torch
    x, hyps, errs = _case(seed, T=9, C=6, n=5, Lmax=4)
    hyps[1] = []                      # the empty hypothesis
    hyps[2] = [1, 1, 1, 1, 1, 1]      # infeasible: 6 equal labels need 11 frames
    blank = x.shape[1] - 1
    r = mwer_ref.mwer(x, hyps, errs, blank, grad_scale=2.0)
    lls, ps, loss, grad = mwer_ref.torch_mwer(x[None], [x.shape[0]], [hyps], [errs], blank, torch.float64, 2.0)
    assert r['ll'][2] == -math.inf and lls[0][2] == -math.inf and r['p'][2] == 0
    ok = np.isfinite(r['ll'])
    assert np.abs(r['ll'][ok] - lls[0][ok]).max() < 1e-10
    assert np.abs(r['p'] - ps[0]).max() < 1e-12
    assert abs(r['loss'] - loss[0]) < 1e-12
    assert np.abs(r['grad'] - grad[0]).max() < 1e-12


def test_known_answer_follows_loss_ewerr():
    """One frame, three classes (blank = 2), logits log([0.5, 0.3, 0.2]).  The hypotheses
    [0], [1], [] have P_CTC 0.5, 0.3, 0.2; with errors 0, 2, 4:
    1) P_hat = P / sum P = [0.5, 0.3, 0.2] (the list is all labellings of one frame);
    2) the errors as given; 3) W_hat = (0 + 2 + 4) / 3 = 2;
    loss = 0.5 (0 - 2) + 0.3 (2 - 2) + 0.2 (4 - 2) = -0.6.
    With only [0] and [1] listed: P_hat = [0.625, 0.375], errors 0, 2, W_hat = 1,
    loss = 0.625 (-1) + 0.375 (1) = -0.25, w = P_hat (e - W_hat - loss) = [-0.46875, 0.46875]."""
    x = np.log(np.array([[0.5, 0.3, 0.2]]))
    r = mwer_ref.mwer(x, [[0], [1], []], [0, 2, 4], blank=2)
    assert np.allclose(np.exp(r['ll']), [0.5, 0.3, 0.2], atol=1e-15)
    assert np.allclose(r['p'], [0.5, 0.3, 0.2], atol=1e-15)
    assert r['ebar'] == 2.0
    assert abs(r['loss'] + 0.6) < 1e-15
    r = mwer_ref.mwer(x, [[0], [1]], [0, 2], blank=2)
    assert np.allclose(r['p'], [0.625, 0.375], atol=1e-15)
    assert r['ebar'] == 1.0 and abs(r['loss'] + 0.25) < 1e-15
    assert np.allclose(r['w'], [-0.46875, 0.46875], atol=1e-15)
    # one frame: occ_i is the indicator of hypothesis i's class
    assert np.allclose(r['grad'], [[-0.46875, 0.46875, 0.0]], atol=1e-15)


def test_cases_defined_to_be_exactly_zero():
    x, hyps, errs = _case(5)
    blank = x.shape[1] - 1
    for hy, er in ((hyps[:1], [3]), (hyps, [3] * len(hyps)), ([], []), ([[0] * 20, [1] * 20], [1, 2])):
        r = mwer_ref.mwer(x, hy, er, blank)
        assert r['loss'] == 0.0 and not r['grad'].any() and not r['w'].any()
    r = mwer_ref.mwer(x, [[0] * 20, [1] * 20], [1, 2], blank)
    assert not r['p'].any() and (r['ll'] == -math.inf).all()
    r = mwer_ref.mwer(x[:0], hyps, errs, blank)
    assert r['loss'] == 0.0 and not r['p'].any()


def test_reference_beam_lists_the_best_prefix_first():
    for T, C, W in ((12, 6, 8), (40, 8, 16)):
        for seed in range(3):
            x = beam_ref.case_logits(seed, T, C)
            want, want_lp, gap = beam_ref.beam_search(x, C - 1, W)
            beam = mwer_ref.beam_nbest(x, C - 1, W)
            assert list(beam[0][0]) == want and beam[0][1] == want_lp
            assert len(beam) <= W and len({p for p, _ in beam}) == len(beam)
            tots = [v for _, v in beam]
            assert tots == sorted(tots, reverse=True)
            if len(beam) > 1:
                assert abs((tots[0] - tots[1]) - gap) < 1e-12


def test_mwer_entry_points_refuse_bad_arguments_without_gpu():
    from srf_amd import _lib
    L = _lib.lib()
    # 4 (B Tmax C + B N Tmax 2 (2 Lmax + 1) + B N) bytes
    assert L.srf_mwer_workspace(28, 200, 32, 4, 200) == 4 * (28 * 200 * 32 + 28 * 4 * 200 * 2 * 401 + 28 * 4)
    assert L.srf_mwer_workspace(1, 1, 2, 1, 0) == 4 * (2 + 2 + 1)
    for B, T, C, N, Lmax, word in ((0, 10, 8, 4, 5, b'B >= 1'), (1, 0, 8, 4, 5, b'Tmax'), (1, 10, 1, 4, 5, b'C >= 2'),
                                   (1, 10, 8, 0, 5, b'1 <= N <= 32'), (1, 10, 8, 33, 5, b'1 <= N <= 32'),
                                   (1, 10, 8, 4, -1, b'Lmax >= 0'), (1, 10, 8, 4, 3000, b'LDS'),
                                   (1, 10, 9000, 4, 5, b'LDS'), (1, 70000, 8, 4, 5, b'Tmax')):
        assert L.srf_mwer_workspace(B, T, C, N, Lmax) == 0, (B, T, C, N, Lmax)
        assert word in L.srf_last_error(), (L.srf_last_error(), word)
    fake = ctypes.c_void_p(4096)   # never dereferenced: every call below is refused before a launch
    need = L.srf_mwer_workspace(2, 10, 8, 4, 5)

    def call(B=2, T=10, C=8, N=4, Lmax=5, blank=7, ws=need, logits=fake, loss=fake):
        return L.srf_mwer_loss(logits, fake, fake, fake, fake, fake, B, T, C, N, Lmax, blank, 1.0, fake, fake, loss,
                               None, fake, ws, None)
    assert call(N=33) == -1 and b'1 <= N <= 32' in L.srf_last_error()
    assert call(C=1) == -1 and b'C >= 2' in L.srf_last_error()
    assert call(blank=8) == -1 and b'blank' in L.srf_last_error()
    assert call(blank=-1) == -1 and b'blank' in L.srf_last_error()
    assert call(logits=None) == -1 and b'null pointer' in L.srf_last_error()
    assert call(loss=None) == -1 and b'null pointer' in L.srf_last_error()
    assert call(ws=need - 1) == -4 and b'workspace' in L.srf_last_error()


def test_beam_nbest_refuses_bad_arguments_without_gpu():
    from srf_amd import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(4096)
    need = L.srf_ctc_beam_state_bytes(1, 8, 4, 10)

    def call(state_bytes=need, W=4, N=2, max_len=10, state=fake, n_hyp=fake, C=8):
        return L.srf_ctc_beam_nbest(state, state_bytes, 1, C, W, 10, N, max_len, fake, fake, fake, n_hyp, None)
    assert call(N=0) == -1 and b'1 <= N <= beam_width' in L.srf_last_error()
    assert call(N=5) == -1 and b'1 <= N <= beam_width' in L.srf_last_error()
    assert call(max_len=0) == -1 and b'max_len >= 1' in L.srf_last_error()
    assert call(W=129, N=1) == -1 and b'beam_width' in L.srf_last_error()
    assert call(C=129) == -1 and b'C <= 128' in L.srf_last_error()
    assert call(state_bytes=need - 1) == -1 and b'state block' in L.srf_last_error()
    assert call(state=None) == -1 and b'null pointer' in L.srf_last_error()
    assert call(n_hyp=None) == -1 and b'null pointer' in L.srf_last_error()


def test_python_wrappers_refuse_before_the_device():
    import torch
    from srf_amd import ctc, mwer, trainer_sr
    with pytest.raises(ValueError, match='device tensor'):
        ctc.beam_search_nbest_device(torch.zeros(1, 3, 4), [3], 3, 4, 2)
    nb = ctc.NBest(torch.zeros(1, 2, 3, dtype=torch.int32), torch.zeros(1, 2, dtype=torch.int32),
                   torch.zeros(1, 2), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError, match='device tensor'):
        mwer.mwer_loss_and_grad(torch.zeros(1, 3, 4), [3], nb, torch.zeros(1, 2), 3, 1.0)
    assert nb.lists() == [[]]
    with pytest.raises(ValueError, match='n_best'):
        trainer_sr.MwerOptions(n_best=33)
    with pytest.raises(ValueError, match='beam_width'):
        trainer_sr.MwerOptions(n_best=8, beam_width=4)
    o = trainer_sr.MwerOptions()
    assert (o.n_best, o.beam_width, o.ctc_weight, o.separator, o.fold) == (4, 16, 0.01, None, None)
    with pytest.raises(ValueError, match='graphs'):
        trainer_sr.distributed_train_step([], 4, None, None, None, None, 1, 0, None, graphs=object(), mwer=o)
