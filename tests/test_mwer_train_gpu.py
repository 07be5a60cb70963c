"""trainer_sr.process_train_step_mwer on the c2_mini fixture (dropout disabled): the loss it
reports and the logit gradient that seeds its backward equal the float64 restatement
(tests/mwer_ref.py) computed on the CPU from the step's own logits and N-best list, with
word errors (a separator) and with label errors (a fold), with and without the CTC term;
``hypothesis_errors`` equals tests/score_ref.py / tests/words_ref.py on the same rows; the
parameters move and stay finite.  Tolerances: those of tests/test_mwer_gpu.py for the MWER
part, scaled by grad_scale for the gradient, plus 1e-4 (relative to 1 + |nll| for the
loss, to the unit-scale CTC gradient otherwise) times ctc_weight for the CTC part.
``distributed_train_step(mwer=None)`` is the path it was, and refuses ``graphs`` with
``mwer``.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from srf_amd import ctc, mwer, scoring, train_helper, trainer_sr
from tests import mwer_ref, score_ref, words_ref
from tests.helpers import config_from_shape, load_model_fixture
from tests.test_mwer_gpu import TOL_GRAD, TOL_LOSS

pytestmark = pytest.mark.gpu

N_BEST, BEAM = 4, 16
SEPARATOR = 43
FOLD = [x // 2 for x in range(62)] + [-1]            # 63 classes onto 31, the blank dropped
# The fixture's parameters are untrained, its hypotheses have a label per frame and share
# nothing with the fixture's labels: every hypothesis would have the same error count, which
# is the exact-zero case.  These references share a first word (label 23, then the separator
# 43) and single labels with some of the first utterance's hypotheses and not with others,
# so the errors of a list differ (asserted below on the host references).
LABELS = [[23, 43, 50, 61, 20], [28, 38, 43, 25, 36]]


class _Spy:
    """The model, keeping the logits of its forward and the gradient that reaches them."""

    def __init__(self, model):
        self.__dict__['model'] = model

    def __call__(self, *args, **kw):
        y = self.model(*args, **kw)
        self.__dict__['logits'] = y.detach().clone()
        y.register_hook(lambda g: self.__dict__.__setitem__('seed', g.detach().clone()))
        return y

    def __getattr__(self, name):
        return getattr(self.model, name)

    def __setattr__(self, name, value):
        setattr(self.model, name, value)


def _setup(dev, opti='adam'):
    from srf_amd.sequence_router import SequenceRouter
    kw, sh, P, z = load_model_fixture('c2_mini')
    cfg = config_from_shape(kw, train_opti_type=opti)   # 'adam': a constant rate; None: the warm-up schedule
    model = SequenceRouter(cfg, None, sh.class_n, device=dev)
    model.load_params(P)
    model.dropout_enabled = False
    inputs = (torch.tensor(z['feats'], dtype=torch.float32, device=dev),
              torch.tensor(LABELS, dtype=torch.int32, device=dev), torch.tensor(z['inp_len']),
              torch.tensor([len(r) for r in LABELS], dtype=torch.int32, device=dev))
    return model, train_helper.get_optimizer(cfg), inputs, sh.class_n - 1, z


def _ctc_reference(logits, lens, labels, tar_len, blank):
    """(nll [B], d sum(nll) / d logits) in float64 on the CPU."""
    x = torch.tensor(logits, dtype=torch.float64, requires_grad=True)
    lp = F.log_softmax(x, dim=-1).transpose(0, 1)
    nll = F.ctc_loss(lp, torch.tensor(labels, dtype=torch.long), torch.tensor(lens, dtype=torch.long),
                     torch.tensor(tar_len, dtype=torch.long), blank=blank, reduction='none')
    nll.sum().backward()
    return nll.detach().numpy(), x.grad.numpy()


@pytest.mark.parametrize('ctc_weight', [0.0, 0.01])
@pytest.mark.parametrize('words', [True, False])
def test_mwer_step_matches_reference(cuda, ctc_weight, words):
    model, opt, inputs, blank, z = _setup(cuda)
    spy = _Spy(model)
    options = trainer_sr.MwerOptions(N_BEST, BEAM, ctc_weight, SEPARATOR if words else None, None if words else FOLD)
    metric = (scoring.WordErrorRate(SEPARATOR, device=cuda) if words else scoring.ErrorRate(fold=FOLD, device=cuda))
    p0 = model.flat_params.clone()
    loss_state = trainer_sr.Mean()
    pe_loss = trainer_sr.process_train_step_mwer(4, inputs, spy, opt, loss_state, None, 1, blank, None, options,
                                                 error_state=metric)
    torch.cuda.synchronize()
    assert not torch.equal(model.flat_params, p0) and bool(torch.isfinite(model.flat_params).all())
    assert opt.iterations == 1

    # the step's own list, from the step's own logits
    logits = spy.logits
    B, T, C = logits.shape
    lens = [-(-int(v) // 4) for v in z['inp_len']]
    logit_len = torch.tensor(lens, dtype=torch.int32, device=cuda)
    nbest = ctc.beam_search_nbest_device(logits, logit_len, blank, BEAM, N_BEST)
    lists = nbest.lists()
    hyps = [[p for p, _ in rows] for rows in lists]
    assert all(len(h) == N_BEST for h in hyps)
    labels = LABELS

    # hypothesis_errors against the host references, row by row
    got = mwer.hypothesis_errors(nbest, inputs[1], inputs[3], options.separator, options.fold).cpu().tolist()
    errs = [[(words_ref.align(h, ref, SEPARATOR) if words else score_ref.align(h, ref, FOLD))['counts'][0]
             for h in rows] for rows, ref in zip(hyps, labels)]
    assert got == [[int(e) for e in row] for row in errs], (got, errs)
    assert any(len(set(row)) > 1 for row in errs), errs   # else loss and gradient are exactly zero

    # loss and seed gradient
    scale = 1.0 / B
    x = logits.cpu().double().numpy()
    want = mwer_ref.mwer_batch(x, lens, hyps, errs, blank, grad_scale=scale)
    nll, g_ctc = _ctc_reference(x, lens, LABELS, [len(r) for r in LABELS], blank)
    for b in range(B):
        g_ctc[b, lens[b]:] = 0
    loss = pe_loss.cpu().double().numpy()
    seed = spy.seed.cpu().double().numpy()
    for b, r in enumerate(want):
        want_loss = r['loss'] + ctc_weight * nll[b]
        tol = TOL_LOSS + ctc_weight * 1e-4 * (1 + abs(nll[b]))
        print(f'utt {b}: loss {loss[b]:.6f} want {want_loss:.6f} (tol {tol:.2e}), errors {errs[b]}, p {r["p"]}')
        assert abs(loss[b] - want_loss) <= tol
        want_g = r['grad'] + ctc_weight * scale * g_ctc[b]
        tol_g = scale * (TOL_GRAD + ctc_weight * 1e-4)
        err = np.abs(seed[b] - want_g).max()
        print(f'utt {b}: seed gradient max {np.abs(want_g).max():.3e}, error {err:.2e} (tol {tol_g:.2e})')
        assert err <= tol_g
    assert abs(loss_state.result() - float(np.mean(loss))) <= 1e-6 * (1 + abs(float(np.mean(loss))))
    # the metric saw hypothesis 0 of every utterance
    res = metric.result()
    assert res['utterances'] == B
    first = [(words_ref.align(rows[0], ref, SEPARATOR) if words else score_ref.align(rows[0], ref, FOLD))['counts']
             for rows, ref in zip(hyps, labels)]
    assert res['substitutions'] + res['deletions'] + res['insertions'] == sum(int(c[0]) for c in first)


def test_distributed_step_without_mwer_is_the_path_it_was(cuda, monkeypatch):
    """mwer=None reaches process_train_step with the arguments it always got, and one step
    from equal initial parameters leaves parameters bit-equal to process_train_step's (the
    reference's schedule, lr(0) = 0, so that the comparison is exact: the routing backward
    sums with float atomics and two runs of one step differ in the last bits of the
    gradient, which is compared at the 1e-5 max|g| of tests/test_model_gpu.py)."""
    m_a, opt_a, inputs, blank, z = _setup(cuda, opti=None)
    m_b, opt_b, _, _, _ = _setup(cuda, opti=None)
    batch = (z['feats'].astype(np.float32), np.array(LABELS, dtype=np.int32), z['inp_len'],
             np.array([len(r) for r in LABELS], dtype=np.int32))
    calls = []
    plain = trainer_sr.process_train_step

    def spy_plain(*a, **k):
        calls.append(('plain', len(a), sorted(k)))
        return plain(*a, **k)
    monkeypatch.setattr(trainer_sr, 'process_train_step', spy_plain)
    monkeypatch.setattr(trainer_sr, 'process_train_step_mwer', lambda *a, **k: calls.append(('mwer', a[-1])))
    la, lb = trainer_sr.Mean(), trainer_sr.Mean()
    p0 = m_a.flat_params.clone()
    n = trainer_sr.distributed_train_step([batch], 4, m_a, opt_a, la, None, 1, blank, None, log=None, mwer=None)
    assert n == 1 and calls == [('plain', 9, [])]
    plain(4, inputs, m_b, opt_b, lb, None, 1, blank, None)
    torch.cuda.synchronize()
    assert torch.equal(m_a.flat_params, m_b.flat_params) and torch.equal(m_a.flat_params, p0)
    assert opt_a.iterations == opt_b.iterations == 1
    mag = m_b.flat_grad.abs().max().item()
    diff = (m_a.flat_grad - m_b.flat_grad).abs().max().item()
    print(f'loss {la.result()!r} vs {lb.result()!r}; max|g| {mag:.3e}, max gradient difference {diff:.3e}')
    assert abs(la.result() - lb.result()) <= 1e-6 * abs(lb.result())
    assert mag > 0 and diff <= 1e-5 * mag
    # a second step moves the parameters (lr(1) > 0)
    trainer_sr.distributed_train_step([batch], 4, m_a, opt_a, None, None, 1, blank, None, log=None)
    plain(4, inputs, m_b, opt_b, None, None, 1, blank, None)
    torch.cuda.synchronize()
    assert calls[1] == ('plain', 9, []) and not torch.equal(m_a.flat_params, p0)
    assert not torch.equal(m_b.flat_params, p0) and bool(torch.isfinite(m_a.flat_params).all())
    options = trainer_sr.MwerOptions()
    with pytest.raises(ValueError, match='graphs'):
        trainer_sr.distributed_train_step([batch], 4, m_a, opt_a, None, None, 1, blank, None, graphs=object(), log=None,
                                          mwer=options)
    n = trainer_sr.distributed_train_step([batch], 4, m_a, opt_a, None, None, 1, blank, None, log=None, mwer=options)
    assert n == 1 and calls[2:] == [('mwer', options)]
