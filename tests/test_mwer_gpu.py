"""srf_mwer_loss on given hypotheses (decoupled from the beam) against the float64
restatement tests/mwer_ref.py, on mwer_ref.KERNEL_CASES: one case per recursion size
class of the kernel (a hypothesis's S = 2 L + 1 in <= 128, <= 256, <= 512, > 512), one on
either side of every class boundary, hypotheses that cross a 64-lane group, and N = 32.
Lengths are ragged, the label padding and the logits past an utterance's length are
poisoned, rows hold repeated labels and one hypothesis is empty.

Tolerances.  hyp_logp: 1e-4 (1 + |want|), as the beam and CTC tests use.  p_hat, loss and
grad: the same formula evaluated with torch on the CPU in float32 (F.ctc_loss and autograd,
mwer_ref.torch_mwer) differs from float64 on exactly these inputs by at most
    p_hat 1.99e-5,   loss 1.99e-5,   grad 2.02e-4      (mwer_ref.measure_fp32_error())
and the device gets 4 x that (it uses the exp2 / log2 instructions and another summation
order).  The figures come from the CPU float32 run, not from the kernel.
"""
import math

import numpy as np
import pytest
import torch

from srf_amd import mwer, ops
from srf_amd.ctc import NBest
from tests import mwer_ref

pytestmark = pytest.mark.gpu

TOL_P = 4 * 1.99e-5      # 4 x the float32 CPU error of p_hat on KERNEL_CASES
TOL_LOSS = 4 * 1.99e-5   # ... of loss
TOL_GRAD = 4 * 2.02e-4   # ... of grad (grad_scale = 1)
MIN_SECOND_P = 0.05      # in every utterance at least two hypotheses carry this much


def _device_inputs(case, N, dev, n_hyp=None):
    hyp, hyp_len, cnt = mwer_ref.dense_hyps(case['hyps'], N, case['Lmax'])
    if n_hyp is not None:
        cnt = np.asarray(n_hyp, dtype=np.int32)
    t = lambda a, dt: torch.tensor(a, dtype=dt, device=dev)   # noqa: E731
    err = np.zeros((len(case['hyps']), N), dtype=np.int32)
    for b, e in enumerate(case['errs']):
        err[b, :len(e)] = e
    return (t(case['logits'], torch.float32), t(case['lens'], torch.int32), t(hyp, torch.int32),
            t(hyp_len, torch.int32), t(cnt, torch.int32), t(err, torch.int32))


def _check(case, want, out, N):
    loss, grad, p_hat, hyp_logp = (None if v is None else v.cpu().double().numpy() for v in out)
    for b, r in enumerate(want):
        n = len(r['ll'])
        T = case['lens'][b]
        for i in range(n):
            if r['ll'][i] == -math.inf:
                assert hyp_logp[b, i] == -math.inf, (b, i)
            else:
                assert abs(hyp_logp[b, i] - r['ll'][i]) <= 1e-4 * (1 + abs(r['ll'][i])), (b, i, hyp_logp[b, i])
        assert (hyp_logp[b, n:] == -math.inf).all() and not p_hat[b, n:].any()
        print(f'utt {b}: |p| {np.abs(p_hat[b, :n] - r["p"]).max() if n else 0:.2e} (tol {TOL_P:.2e})  '
              f'|loss| {abs(loss[b] - r["loss"]):.2e} (tol {TOL_LOSS:.2e})  '
              f'|grad| {np.abs(grad[b] - r["grad"]).max():.2e} (tol {TOL_GRAD:.2e})  '
              f'|row sum| {np.abs(grad[b].sum(axis=1)).max():.2e}')
        if n:
            assert np.abs(p_hat[b, :n] - r['p']).max() <= TOL_P
        assert abs(loss[b] - r['loss']) <= TOL_LOSS
        assert np.abs(grad[b] - r['grad']).max() <= TOL_GRAD
        assert np.abs(grad[b].sum(axis=1)).max() <= TOL_GRAD
        assert not grad[b, T:].any()
        assert np.isfinite(grad[b]).all()


@pytest.mark.parametrize('index', range(len(mwer_ref.KERNEL_CASES)))
def test_mwer_loss_matches_float64(cuda, index):
    B, N, T, C, Lmax = mwer_ref.KERNEL_CASES[index][:5]
    case = mwer_ref.kernel_case(index)
    want = mwer_ref.mwer_batch(case['logits'], case['lens'], case['hyps'], case['errs'], case['blank'])
    for b, r in enumerate(want):   # the condition on the inputs, from the reference alone
        assert np.sort(r['p'])[-2] >= MIN_SECOND_P, (b, r['p'])
    assert any(T_b < T for T_b in case['lens']) or B == 1
    args = _device_inputs(case, N, cuda)
    out = ops.mwer_loss_and_grad(*args, case['blank'], 1.0)
    _check(case, want, out, N)
    # the loss alone (grad = NULL) and a second call: the same bits
    lo = ops.mwer_loss_and_grad(*args, case['blank'], 1.0, want_grad=False)
    assert lo[1] is None
    again = ops.mwer_loss_and_grad(*args, case['blank'], 1.0)
    for k in (0, 2, 3):
        assert torch.equal(out[k].view(torch.int32), lo[k].view(torch.int32))
        assert torch.equal(out[k].view(torch.int32), again[k].view(torch.int32))
    assert torch.equal(out[1].view(torch.int32), again[1].view(torch.int32))


def _edge_case():
    """Case 0's shape with five utterances: (0) no hypothesis, (1) one hypothesis, (2) one
    infeasible hypothesis among feasible ones, (3) all infeasible, (4) equal errors."""
    base = mwer_ref.kernel_case(0)
    rng = np.random.default_rng(77)
    T, C = base['logits'].shape[1:]
    logits = rng.standard_normal((5, T, C)).astype(np.float32)
    lens = [12, 11, 12, 9, 10]
    for b, Tb in enumerate(lens):
        logits[b, Tb:] = np.nan
    long_row = [1] * 12                     # 12 equal labels need 23 frames
    hyps = [[], [[0, 1, 2]], [[0, 1], long_row, [1, 1, 3], [2]], [long_row, [2] * 10, [0, 0, 0, 0, 0, 0]],
            [[0, 1], [1, 0, 2], [], [3, 3]]]
    errs = [[], [5], [1, 0, 4, 2], [1, 2, 3], [3, 3, 3, 3]]
    return {'logits': logits, 'lens': lens, 'hyps': hyps, 'errs': errs, 'blank': C - 1, 'Lmax': 12}


def test_edge_cases(cuda):
    case = _edge_case()
    N = 4
    want = mwer_ref.mwer_batch(case['logits'], case['lens'], case['hyps'], case['errs'], case['blank'])
    assert want[2]['ll'][1] == -math.inf and np.sort(want[2]['p'])[-2] >= MIN_SECOND_P
    assert (want[3]['ll'] == -math.inf).all()
    out = ops.mwer_loss_and_grad(*_device_inputs(case, N, cuda), case['blank'], 1.0)
    _check(case, want, out, N)
    loss, grad, p_hat, hyp_logp = out
    for b in (0, 1, 3, 4):   # defined to be exactly zero
        assert float(loss[b]) == 0.0 and not grad[b].any().item(), b
    assert not p_hat[0].any().item() and not p_hat[3].any().item()
    assert float(p_hat[1, 0]) == 1.0
    assert float(p_hat[2, 1]) == 0.0 and grad[2].any().item()


def test_grad_scale_and_autograd(cuda):
    index = 0
    N = mwer_ref.KERNEL_CASES[index][1]
    case = mwer_ref.kernel_case(index)
    logits, lens, hyp, hyp_len, cnt, err = _device_inputs(case, N, cuda)
    logits = torch.nan_to_num(logits, nan=0.0)   # autograd multiplies the padding by g
    nbest = NBest(hyp, hyp_len, torch.zeros_like(err, dtype=torch.float32), cnt)
    loss1, grad1, p1, ll1 = mwer.mwer_loss_and_grad(logits, lens, nbest, err, case['blank'], 1.0)
    loss3, grad3, _, _ = mwer.mwer_loss_and_grad(logits, lens, nbest, err, case['blank'], 0.125)
    assert torch.equal(loss1, loss3)
    assert torch.equal(grad3, grad1 * 0.125)   # a power of two scales exactly
    x = logits.clone().requires_grad_(True)
    out = mwer.mwer_loss(x, lens, nbest, err, case['blank'])
    assert torch.equal(out.detach(), loss1)
    g = torch.tensor([0.5, -2.0, 3.0], device=cuda)
    out.backward(g)
    assert torch.equal(x.grad, grad1 * g[:, None, None])
    with torch.no_grad():
        assert not mwer.mwer_loss(logits, lens, nbest, err, case['blank']).requires_grad
