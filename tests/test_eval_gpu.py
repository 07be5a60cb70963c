"""The evaluation path on the GPU (``training=False``: BatchNorm on its moving
statistics, no dropout, and under ``torch.no_grad()`` the forward that keeps nothing
for a backward) against the evaluation-mode fixtures of the CPU oracle
(tests/golden/model_*_eval.npz, oracle/gen_golden.py EVAL_CASES): the model itself,
the SDR stack's no-backward plans, and trainer_sr's validation / test steps.

The fixtures' moving statistics come from an independent batch, so evaluation-mode
logits differ from training-mode logits by 0.06 to 1.5: a mode mix-up cannot pass.

Tolerances are the project's own (tests/test_model_gpu.py): logits
|err| <= 1e-4 * (1 + |ref|); CTC NLL |err| <= 1e-4 * max(1, |ref|); greedy label
sequences bit-exact (the fixtures guarantee a top-1 / top-2 margin of >= 10 logit
tolerances on every decoded frame).

Not covered: the branch of ops.SdrStack for a last-layer u above 1 GiB under
no_grad (``not pose_ahead``: the last layer's pose on the recurrence's stream into
a range buffer).  No test-sized shape reaches it (C5's last-layer u is 54 MB at
the fixture's 10 frames)."""
import contextlib

import numpy as np
import pytest
import torch

from oracle import srf_oracle as so
from tests.helpers import config_from_shape, load_eval_fixture

pytestmark = pytest.mark.gpu

FIXTURES = ['c1_mini', 'c2_mini', 'c3_mini_sdr', 'c2_mini_einsum', 'c2_mini_lowmemory', 'c3_mini_sdr_lowmemory',
            'c4_mini', 'c4_real', 'c3_real', 'c5_real']
MOVING = ['bn0_moving_mean', 'bn0_moving_var', 'bn1_moving_mean', 'bn1_moving_var']


@pytest.fixture(scope='module')
def built(cuda):
    """built(name, **config overrides) -> (model, shape, base arrays, eval arrays).
    Each fixture is loaded and its model built once for the module (regenerating
    C5's parameters takes seconds, its forward does not): evaluation writes neither
    parameters nor moving statistics, which the tests assert, so the tests can share
    the models; what a test may have set on one (sdr_stack, sdr_options and the
    plans made from them) is reset on every call.  ``dropout_enabled`` stays at its
    default True: evaluation must ignore it."""
    from srf_amd.sequence_router import SequenceRouter
    cache = {}

    def get(name, **over):
        key = (name, tuple(sorted(over.items())))
        if key not in cache:
            kw, sh, P, z, ev = load_eval_fixture(name)
            model = SequenceRouter(config_from_shape(kw, **over), None, sh.class_n, device=cuda)
            model.load_params(P)
            cache[key] = (model, sh, z, ev)
        model, sh, z, ev = cache[key]
        model.sdr_stack, model.sdr_options = True, {}
        model._geoms.clear()
        assert model.dropout_enabled
        for k in range(2):   # the fixture's moving statistics are (still) in the buffers
            for s in ('mean', 'var'):
                assert np.array_equal(getattr(model, f'bn{k}_moving_{s}').cpu().numpy(), ev[f'bn{k}.moving_{s}'])
        return model, sh, z, ev
    yield get
    cache.clear()


def _inputs(z, dev):
    return (torch.tensor(z['feats'], dtype=torch.float32, device=dev), torch.tensor(z['labels'], device=dev),
            torch.tensor(z['inp_len'], dtype=torch.int32, device=dev), torch.tensor(z['tar_len'], device=dev))


def _logit_check(got, ref, what):
    assert got.shape == ref.shape
    err = np.abs(got - ref)
    print(f'{what}: max logit err {err.max():.3e}, in tolerances {(err / (1e-4 * (1 + np.abs(ref)))).max():.3f}')
    assert np.all(err <= 1e-4 * (1 + np.abs(ref))), err.max()


@pytest.mark.parametrize('grad', [False, True], ids=['no_grad', 'grad'])
@pytest.mark.parametrize('name', FIXTURES)
def test_eval_logits_nll_greedy(cuda, built, name, grad):
    """model(..., training=False) under no_grad (nothing kept for a backward: no
    couplings, SDR u posed into reused range buffers) and with grad enabled (the
    coupling-storing forward): logits, NLL at ceil lengths, greedy decode at the
    validation step's ceil and the test step's floor lengths, all against the oracle;
    the moving statistics are read, never written."""
    from srf_amd import ctc
    model, sh, z, ev = built(name)
    feats, labels, inp_len, tar_len = _inputs(z, cuda)
    before = [getattr(model, n).clone() for n in MOVING]
    with (contextlib.nullcontext() if grad else torch.no_grad()):
        logits = model(feats, input_lengths=inp_len, training=False)
        assert logits.requires_grad == grad
        nll = ctc.ctc_loss(labels, logits, tar_len, (inp_len + 3) // 4, blank_index=sh.class_n - 1)
    torch.cuda.synchronize()
    for n, b in zip(MOVING, before):
        assert torch.equal(getattr(model, n), b), n
    _logit_check(logits.detach().cpu().double().numpy(), ev['logits'].astype(np.float64), name)
    nll = nll.detach().cpu().double().numpy()
    assert np.all(np.abs(nll - ev['nll']) <= 1e-4 * np.maximum(1, np.abs(ev['nll']))), (nll, ev['nll'])
    blank = sh.class_n - 1
    assert ctc.greedy_decode(logits, (inp_len + 3) // 4, blank) == ev['greedy_ceil']
    assert ctc.greedy_decode(logits, inp_len // 4, blank) == ev['greedy_floor']


@pytest.mark.parametrize('name,chunks', [('c3_mini_sdr', 1), ('c3_mini_sdr', 3), ('c3_mini_sdr', 64),
                                         ('c3_real', 4), ('c5_real', 3)])
def test_eval_sdr_stack_plans(cuda, built, name, chunks):
    """The SDR stack without a backward (plan.need_bwd False under no_grad): every
    range posed into a reused nmax-frame u buffer, the last layer's pose run ahead on
    a third stream into a whole-T buffer, no couplings (also on C5's streaming
    recurrence) -- for one range, several (the buffers are cycled) and one frame per
    range (64 > T').  Logits against the oracle, and within 1e-5 (1 + max|ref|) of
    the same model run layer by layer (model.sdr_stack = False)."""
    outs = []
    model, sh, z, ev = built(name)
    model.sdr_options = dict(n_chunks=chunks)
    feats, _, inp_len, _ = _inputs(z, cuda)
    for stack in (True, False):
        model.sdr_stack = stack
        with torch.no_grad():
            logits = model(feats, input_lengths=inp_len, training=False)
        torch.cuda.synchronize()
        outs.append(logits)
        if stack:
            plan = model._stack_plan(feats.shape[0], logits.shape[1])
            assert plan.need_bwd is False
            ranges = [sum(1 for k in range(plan.K) if b[k] < b[k + 1]) for b in plan.fwd]
            if chunks > 1:
                assert min(ranges) > 1, ranges
            _logit_check(logits.cpu().double().numpy(), ev['logits'].astype(np.float64), f'{name} n_chunks={chunks}')
    d = (outs[0] - outs[1]).abs().max().item()
    print(f'{name} n_chunks={chunks}: stack vs layer by layer {d:.3e}')
    assert d <= 1e-5 * (1 + outs[1].abs().max().item())


@pytest.mark.parametrize('name', ['c2_mini', 'c3_mini_sdr'])
def test_valid_and_test_steps(cuda, built, name, capsys):
    """trainer_sr.process_valid_step returns the oracle's evaluation-mode NLL and
    feeds the metric; process_test_step decodes at floor(len / 4) (trainer_sr.py:110;
    the fixture's greedy_floor).  With a beam, every hypothesis fits its floor
    length and is at least as likely under the oracle's logits as the greedy one."""
    from srf_amd import trainer_sr
    model, sh, z, ev = built(name)
    inputs = _inputs(z, cuda)
    blank = sh.class_n - 1
    state = trainer_sr.Mean()
    nll = trainer_sr.process_valid_step(4, inputs, model, state, blank).cpu().double().numpy()
    assert np.all(np.abs(nll - ev['nll']) <= 1e-4 * np.maximum(1, np.abs(ev['nll']))), (nll, ev['nll'])
    assert state.count == len(nll)
    assert abs(state.result() - ev['nll'].mean()) <= 1e-4 * max(1, abs(ev['nll'].mean()))
    utts = [f'utt{b}' for b in range(len(nll))]
    test_inputs = (inputs[0], inputs[1], inputs[2], inputs[3], utts)
    hyps = trainer_sr.process_test_step(4, test_inputs, model)
    assert hyps == ev['greedy_floor']
    beam = trainer_sr.process_test_step(4, test_inputs, model, beam_width=16)
    out = capsys.readouterr().out
    assert all(f'UTTID: {u}' in out for u in utts)
    ref = ev['logits'].astype(np.float64)
    for b, (h, g) in enumerate(zip(beam, ev['greedy_floor'])):
        n = int(z['inp_len'][b]) // 4
        assert len(h) <= n, (b, h, n)
        nb, ng = so.ctc_nll(ref[b, :n], np.array(h, dtype=np.int64), blank), \
            so.ctc_nll(ref[b, :n], np.array(g, dtype=np.int64), blank)
        print(f'{name} utt {b}: beam nll {nb:.4f} greedy nll {ng:.4f}')
        assert nb <= ng, (b, h, g, nb, ng)


def test_eval_fp8_pose(cuda, built):
    """C5 with the opt-in fp8 pose in evaluation mode under no_grad, shaped like
    tests/test_parity_scale_gpu.py::test_c5_fp8_pose_end_to_end: the plan keeps u in
    bf16 on the layers the fixture emulated; per utterance max|gpu - o64| <=
    1.5 max|emul - o64| + 1e-3 (1 + max|o64|), the same for the NLL, and the median
    |gpu - o64| <= 1.5 median |emul - o64| (o64: the plain oracle on the same moving
    statistics, emul: the float64 mirror with the pose's e4m3 / bf16 quantisation)."""
    from srf_amd import ctc
    model, sh, z, ev = built('c5_real_fp8', model_pose_fp8=True)
    assert model.pose_fp8
    feats, labels, inp_len, tar_len = _inputs(z, cuda)
    with torch.no_grad():
        logits = model(feats, input_lengths=inp_len, training=False)
        nll = ctc.ctc_loss(labels, logits, tar_len, (inp_len + 3) // 4, blank_index=sh.class_n - 1)
    plan = model._stack_plan(feats.shape[0], logits.shape[1])
    assert plan.need_bwd is False
    assert [bool(b) for b in plan.ubf] == [bool(b) for b in ev['bf16_layers']]
    got, nll = logits.cpu().double().numpy(), nll.cpu().double().numpy()
    emul, o64 = ev['logits'].astype(np.float64), ev['logits_o64'].astype(np.float64)
    ax = tuple(range(1, got.ndim))
    e_gpu, e_emul = np.abs(got - o64), np.abs(emul - o64)
    print(f'fp8 eval: max|gpu - o64| {e_gpu.max(ax)}, max|emul - o64| {e_emul.max(ax)}, medians '
          f'{np.median(e_gpu):.3e} {np.median(e_emul):.3e}, nll {nll} emul {ev["nll"]} o64 {ev["nll_o64"]}')
    lim = 1.5 * e_emul.max(ax) + 1e-3 * (1 + np.abs(o64).max(ax))
    assert np.all(e_gpu.max(ax) <= lim), (e_gpu.max(ax), lim)
    assert np.median(e_gpu) <= 1.5 * np.median(e_emul), (np.median(e_gpu), np.median(e_emul))
    nlim = 1.5 * np.abs(ev['nll'] - ev['nll_o64']) + 1e-3 * np.maximum(1, np.abs(ev['nll_o64']))
    assert np.all(np.abs(nll - ev['nll_o64']) <= nlim), (nll, ev['nll'], ev['nll_o64'])
