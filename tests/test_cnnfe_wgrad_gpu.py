"""Stage-2 kernel gradients (g_k1a / g_k1b) of the HIP CNN front end on the shapes at
which conv2_wgrad_rows_kernel's structure can go wrong: the ring of staged y1 rows
restarting inside a workgroup's rows, both time paddings, masked rows, workgroups
without rows, a row count that is no multiple of the rows per workgroup, F1 odd with
F2 < 31, and F2 = 33 on the other side of the kernel choice (conv2_wgrad32_kernel).

No tolerance fixed in advance: tests/torch_ref.cnnfe in float64 is the reference and
the same restatement in float32 on the CPU the yardstick, per tensor
    max|gpu - f64| <= 4 max|f32 - f64| + 1e-6 max|f64|.
Precondition, checked on the CPU: both precisions take the same maxout branch at every
position of both stages (tests/cnnfe_wgrad_cases.reference counts the flips), so that
the kernel and not a flipped near-tie decides the error."""
import numpy as np
import pytest
import torch

from tests import cnnfe_wgrad_cases as wc

KEYS = ('conv1a_kernel', 'conv1b_kernel')


def _gpu_grads(cuda, ref):
    from srf_amd import ops
    Pg = {k: v.float().to(cuda).requires_grad_() for k, v in ref['P'].items()}
    moving = [torch.zeros(64, device=cuda), torch.ones(64, device=cuda), torch.zeros(64, device=cuda),
              torch.ones(64, device=cuda)]
    out = ops.cnnfe(torch.tensor(ref['feats'], dtype=torch.float32, device=cuda), ref['inp_len'].to(cuda),
                    [Pg[k] for k in ops.CNNFE_PARAMS], moving, True, ref['p'], wc.DROP_SEED)
    (out * ref['gout'].float().to(cuda)).sum().backward()
    torch.cuda.synchronize()
    return {k: Pg[k].grad.detach().cpu() for k in KEYS}


def test_case_structure():
    """The cases reach what they are meant to (launcher arithmetic restated in cnnfe_wgrad_cases)."""
    C = wc.CASES
    assert wc.spans_boundary(*C['span_boundary'][:2]) and wc.spans_boundary(*C['feat41_rows3'][:2])
    rr, T2 = wc.row_ranges(*C['span_boundary'][:2])
    assert rr[0][1] - rr[0][0] == 2 and any(e - b == 1 for b, e in rr) and any(e == b for b, e in rr)
    assert wc.row_ranges(*C['feat41_rows3'][:2])[0][0] == (0, 3)
    for name in ('one_row', 'three_rows', 'short_utts'):   # one row per workgroup, the rest have none
        rr, T2 = wc.row_ranges(*C[name][:2])
        assert sum(e > b for b, e in rr) == C[name][0] * T2 < wc.RANGES
    assert wc.dims(37, 123)[0] % 2 == 1 and wc.dims(40, 123)[0] % 2 == 0        # pt2 = 1 / pt2 = 0
    assert wc.dims(1, 41)[1] % 2 == 1 and wc.dims(1, 41)[3] == 11                 # pf2 = 1, F2 < 31
    assert not wc.by_rows(129) and all(wc.by_rows(c[4]) for n, c in C.items() if not n.startswith('feat129'))
    B, T, _, _, feat_dim, _ = C['feat129_full_planes']      # old path, g_ab planes without padding
    _, _, T2, F2 = wc.dims(T, feat_dim)
    assert not wc.by_rows(feat_dim) and (B * T2 * F2) % wc.PLANE_PX == 0
    B, T, _, _, feat_dim, _ = C['feat129_old_path']         # and with padding
    assert (B * wc.dims(T, feat_dim)[2] * wc.dims(T, feat_dim)[3]) % wc.PLANE_PX != 0


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(wc.CASES))
def test_cnnfe_wgrad(cuda, name):
    """Observed on an MI355X, max|gpu - f64| / max|f32 - f64| of g_k1a, g_k1b, default build
    then -DSRF_CONV2_WGRAD_ROWS=0 (the old kernels) in brackets:
    short_utts 0.42, 0.39 (0.42, 0.35); span_boundary 0.48, 0.38 (0.50, 0.38);
    pt2_1 0.26, 0.30 (0.29, 0.34); pt2_0_drop 0.43, 0.45 (0.44, 0.54);
    one_row 3.90, 2.23 (3.90, 2.23: bit-identical); three_rows 0.83, 0.76 (0.80, 0.76);
    feat41 0.87, 0.69 (0.70, 0.75); feat41_rows3 0.25, 0.27 (0.23, 0.29);
    feat129_old_path 0.56, 0.55 in both (the same kernel); feat129_full_planes 0.39, 0.46.
    The worst err / bound is 0.36 (one_row g_k1a) in both builds, so the old kernels pass
    the factor 4 with more than 2x headroom and it stands.  Per tensor the default build's
    error is 0.84 .. 1.25 times the old build's (largest: feat41 g_k1a, 1.52e-5 against
    1.22e-5); compared by hand, not asserted."""
    ref = wc.reference(name)
    assert ref['flips'] == 0, f"{ref['flips']} maxout branches differ between float32 and float64: pick another seed"
    got = _gpu_grads(cuda, ref)
    worst = 0.0
    for k in KEYS:
        g64, g32 = ref['g64'][k], ref['g32'][k]
        e_gpu = np.abs(got[k].double().numpy() - g64).max()
        e_f32 = np.abs(g32 - g64).max()
        mag = np.abs(g64).max()
        bound = 4 * e_f32 + 1e-6 * mag
        print(f'wgrad {name} {k}: max|gpu - f64| {e_gpu:.3e}, max|f32 - f64| {e_f32:.3e}, max|f64| {mag:.3e}, '
              f'e_gpu / e_f32 {e_gpu / max(e_f32, 1e-300):.3f}, err / bound {e_gpu / bound:.3f}')
        worst = max(worst, e_gpu / bound)
    assert worst <= 1.0, worst


@pytest.mark.gpu
def test_cnnfe_wgrad_deterministic(cuda):
    """Two backward calls on the same inputs: bit-identical g_k1a / g_k1b (slabs and a
    fixed-order reduce, no float atomics)."""
    ref = wc.reference('span_boundary')
    a = _gpu_grads(cuda, ref)
    b = _gpu_grads(cuda, ref)
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k
