"""The din-32 routing passes r >= 1 from the stored couplings (route_fwd32.hip:
route_fwd32_kernel / route_bwd32_kernel with four row tiles per wave, route_fwd32p_kernel /
route_bwd32p_kernel pipelined with two) and the finishes behind them (route_dr.hip
bwd_finish_kernel), at the smallest shapes that reach every path of their capsule loops.

Shapes: F = 74 frames is three 32-frame tiles with the last one partial, in_n = 9 input
capsules.  J * dout = 640 takes the four-row-tile kernels with eight waves and masked rows
past 640; J = 16 the pipelined kernels with eight waves; J = 8 with four waves and R = 2.
Plans: the default; 1 uniform chunk (nine capsules: the odd tail of the pipelined loop,
which is unrolled by two); 2 chunks (5 + 4); 9 chunks (one capsule each: every x DMA of
the prologue and the loop clamps to the chunk's only capsule); and, for the pipelined
kernels, a balanced plan whose spans cross the tile edges.  R = 3 and R = 2 together cover
the three ways the backward finish treats A = sum of the later passes' gVc: not stored
(first launch), read and stored (between two passes), slab sums alone and not stored
(after pass 1); with R = 2, A is never touched.

Tolerances are the project's: v against the numpy oracle 2e-5 (1 + |ref|); gradients
against the float64 mirror 1e-4 max(1, max|ref|); gradients against the backward that
recomputes the logits (store_couplings=False) 2e-5 max(1, max|b|).  g_W and g_bias are
sums in a fixed order (only g_emb goes through float atomics), so two runs of one plan
give the same bits.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import naive_mirror as nm
from oracle import srf_oracle as so

pytestmark = pytest.mark.gpu

BAL = 1 << 20   # srf::kBalFlag

# B, T, N, D, lpad, rpad, J, iters, mask_first
CASE_TW4 = (2, 37, 3, 32, 1, 1, 20, 3, True)     # route_fwd32_kernel / route_bwd32_kernel <32,32,8,4>
CASE_P8 = (2, 37, 3, 32, 1, 1, 16, 3, False)     # pipelined, eight waves
CASE_P4 = (2, 37, 3, 32, 1, 1, 8, 2, True)       # pipelined, four waves, R = 2

PLANS = [
    pytest.param(CASE_TW4, 0, id='tw4-default'),
    pytest.param(CASE_TW4, 1, id='tw4-1-chunk'),
    pytest.param(CASE_TW4, 2, id='tw4-2-chunks'),
    pytest.param(CASE_TW4, 9, id='tw4-9-chunks'),
    pytest.param(CASE_P8, 0, id='p8-default'),
    pytest.param(CASE_P8, 1, id='p8-1-chunk-odd-tail'),
    pytest.param(CASE_P8, 2, id='p8-2-chunks'),
    pytest.param(CASE_P8, 9, id='p8-9-chunks'),
    pytest.param(CASE_P8, BAL | 5, id='p8-balanced-G5'),
    pytest.param(CASE_P4, 0, id='p4-default'),
    pytest.param(CASE_P4, 1, id='p4-1-chunk-odd-tail'),
    pytest.param(CASE_P4, 2, id='p4-2-chunks'),
    pytest.param(CASE_P4, 9, id='p4-9-chunks'),
    pytest.param(CASE_P4, BAL | 5, id='p4-balanced-G5'),
]


@functools.lru_cache(maxsize=None)
def _inputs(case):
    B, T, N, D, lp, rp, J, it, mf = case
    rng = np.random.default_rng(31)
    in_n = N * (lp + rp + 1)
    emb = rng.standard_normal((B, T, N, D)) * 0.5
    W = rng.standard_normal((in_n, J, D, D)) * 0.1
    bias = rng.standard_normal((in_n, J, D)) * 0.1
    gv = rng.standard_normal((B, T, J, D))
    return emb, W, bias, gv


@functools.lru_cache(maxsize=None)
def _oracle(case):
    """fp64, once per case: v (numpy restatement) and the gradients (autograd of the torch mirror)."""
    B, T, N, D, lp, rp, J, it, mf = case
    emb, W, bias, gv = _inputs(case)
    v = so.dynamic_routing(so.pose(so.window(emb, lp, rp), W, bias), it, mf)
    ce, cW, cb = (torch.tensor(a, requires_grad=True) for a in (emb, W, bias))
    ep = torch.nn.functional.pad(ce, (0, 0, 0, 0, lp, rp))
    xw = torch.cat([ep[:, w:w + T] for w in range(lp + rp + 1)], dim=2)
    nm.dynamic_routing(nm.pose_tiled(xw, cW, cb), it, mf).backward(torch.tensor(gv))
    return v, ce.grad.numpy(), cW.grad.numpy(), cb.grad.numpy()


def _run(case, plan, dev, store_couplings=True):
    """v and (g_emb, g_W, g_bias) as the kernels wrote them (fp32, on the host)."""
    from srf_amd.ops import RouteGeom, dynamic_routing
    B, T, N, D, lp, rp, J, it, mf = case
    emb, W, bias, gv = _inputs(case)
    g = RouteGeom(B, T, N, D, lp, rp, J, D, it, mf, plan)
    g.store_couplings = store_couplings
    te, tW, tb = (torch.tensor(a, dtype=torch.float32, device=dev, requires_grad=True) for a in (emb, W, bias))
    v = dynamic_routing(te, tW, tb, g)
    v.backward(torch.tensor(gv, dtype=torch.float32, device=dev))
    torch.cuda.synchronize()
    return [v.detach().cpu().numpy()] + [t.grad.detach().cpu().numpy() for t in (te, tW, tb)]


_recomputed = {}


def _run_recompute(case, dev):
    """The gradients of the backward that recomputes the logits (route_pass_kernel), once per case."""
    if case not in _recomputed:
        _recomputed[case] = _run(case, 0, dev, store_couplings=False)
    return _recomputed[case]


@pytest.mark.parametrize('case,plan', PLANS)
def test_stored_coupling_passes(cuda, case, plan):
    ref = _oracle(case)
    got = _run(case, plan, cuda)
    again = _run(case, plan, cuda)
    rec = _run_recompute(case, cuda)
    names = ('g_emb', 'g_W', 'g_bias')
    figures = {'v': np.abs(got[0] - ref[0]).max()}
    for name, g, r, b in zip(names, got[1:], ref[1:], rec[1:]):
        figures[name] = (np.abs(g - r).max(), np.abs(r).max(), np.abs(g.astype(np.float64) - b).max(), np.abs(b).max())
    print(case, plan, figures)
    assert np.all(np.abs(got[0] - ref[0]) <= 2e-5 * (1 + np.abs(ref[0]))), figures['v']
    for name, g, r, b in zip(names, got[1:], ref[1:], rec[1:]):
        err = np.abs(g - r).max()
        assert err <= 1e-4 * max(1.0, np.abs(r).max()), (name, 'against the float64 mirror', err, np.abs(r).max())
        d = np.abs(g.astype(np.float64) - b).max()
        assert d <= 2e-5 * max(1.0, np.abs(b).max()), (name, 'against the recomputing backward', d)
    assert np.array_equal(got[2], again[2]), 'g_W differs between two runs of one plan'
    assert np.array_equal(got[3], again[3]), 'g_bias differs between two runs of one plan'
