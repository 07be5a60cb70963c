"""The balanced split of the DR routing passes r >= 1 (route_fwd32.hip SegWalk: persistent
workgroups that walk segments of the (frame tile, input capsule) space) on the GPU.

Small shapes take a balanced plan with a given workgroup count G through the plan argument
BAL | G (RouteGeom n_chunks), the encoding of the bench inner layers' default plan.  Each
case is checked against the fp64 oracle at the tolerances of tests/test_route_dr_gpu.py
(forward 2e-5 (1 + |ref|), gradients 1e-4 max(1, max|ref|)) and against an explicit
chunked plan at the bounds of its test_route_dr_chunking_invariant (forward 1e-5,
gradients 2e-5 max(1, max|a|)).  Every kernel a balanced plan can select appears:
route_fwd32p / route_bwd32p (two row tiles per wave), route_fwd32 / route_bwd32 (four, with
the masked first capsule), four-wave workgroups with two iterations, and din 16.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import naive_mirror as nm
from oracle import srf_oracle as so

pytestmark = pytest.mark.gpu

BAL = 1 << 20   # srf::kBalFlag

# B, T, N, D, lpad, rpad, J, iters, mask_first
CASE_P = (2, 40, 4, 32, 1, 1, 16, 3, False)    # 3 tiles (last ragged) x 12 capsules, U = 36
CASE_4 = (2, 40, 4, 32, 1, 1, 32, 3, True)     # four row tiles per wave, masked first capsule
CASE_NW4 = (1, 35, 8, 32, 1, 2, 8, 2, True)    # R = 2, NW = 4
CASE_D16 = (3, 37, 8, 16, 4, 4, 63, 3, True)   # din 16

PLANS = [
    pytest.param(CASE_P, 5, id='p-G5-span-crosses-a-tile-edge'),
    pytest.param(CASE_P, 7, id='p-G7-one-capsule-segment-at-a-tile-start'),
    pytest.param(CASE_P, 1, id='p-G1-one-workgroup-walks-all-tiles'),
    pytest.param(CASE_P, 36, id='p-G36-every-segment-one-capsule'),
    pytest.param(CASE_4, 5, id='tw4-masked-G5'),
    pytest.param(CASE_4, 7, id='tw4-masked-G7'),
    pytest.param(CASE_NW4, 5, id='nw4-two-iterations-G5'),
    pytest.param(CASE_D16, 7, id='din16-G7'),
]


@functools.lru_cache(maxsize=None)
def _inputs(case):
    B, T, N, D, lp, rp, J, it, mf = case
    rng = np.random.default_rng(21)
    in_n = N * (lp + rp + 1)
    emb = rng.standard_normal((B, T, N, D)) * 0.5
    W = rng.standard_normal((in_n, J, D, D)) * 0.1
    bias = rng.standard_normal((in_n, J, D)) * 0.1
    gv = rng.standard_normal((B, T, J, D))
    return emb, W, bias, gv


@functools.lru_cache(maxsize=None)
def _oracle(case):
    """fp64: v (numpy restatement) and the gradients (autograd of the torch mirror), once per case."""
    B, T, N, D, lp, rp, J, it, mf = case
    emb, W, bias, gv = _inputs(case)
    v = so.dynamic_routing(so.pose(so.window(emb, lp, rp), W, bias), it, mf)
    ce, cW, cb = (torch.tensor(a, requires_grad=True) for a in (emb, W, bias))
    ep = torch.nn.functional.pad(ce, (0, 0, 0, 0, lp, rp))
    xw = torch.cat([ep[:, w:w + T] for w in range(lp + rp + 1)], dim=2)
    nm.dynamic_routing(nm.pose_tiled(xw, cW, cb), it, mf).backward(torch.tensor(gv))
    return v, ce.grad.numpy(), cW.grad.numpy(), cb.grad.numpy()


def _run(case, plan, dev):
    from srf_amd.ops import RouteGeom, dynamic_routing
    B, T, N, D, lp, rp, J, it, mf = case
    emb, W, bias, gv = _inputs(case)
    g = RouteGeom(B, T, N, D, lp, rp, J, D, it, mf, plan)
    assert g.n_chunks == plan
    te, tW, tb = (torch.tensor(a, dtype=torch.float32, device=dev, requires_grad=True) for a in (emb, W, bias))
    v = dynamic_routing(te, tW, tb, g)
    v.backward(torch.tensor(gv, dtype=torch.float32, device=dev))
    torch.cuda.synchronize()
    return [v.detach().cpu().double().numpy()] + [t.grad.cpu().double().numpy() for t in (te, tW, tb)]


_chunked = {}


def _run_chunked(case, dev):
    if case not in _chunked:
        _chunked[case] = _run(case, 3, dev)
    return _chunked[case]


def _check_oracle(case, got):
    ref = _oracle(case)
    assert np.all(np.abs(got[0] - ref[0]) <= 2e-5 * (1 + np.abs(ref[0]))), np.abs(got[0] - ref[0]).max()
    for name, g, r in zip(('g_emb', 'g_W', 'g_bias'), got[1:], ref[1:]):
        err = np.abs(g - r).max()
        assert err <= 1e-4 * max(1.0, np.abs(r).max()), (name, err, np.abs(r).max())


@pytest.mark.parametrize('case,G', PLANS)
def test_balanced_plan_matches_oracle_and_chunked(cuda, case, G):
    from srf_amd import _lib
    B, T, N, D, lp, rp, J, it, mf = case
    info = (ctypes.c_int * 5)()
    n = _lib.lib().srf_route_dr_split_table(B, T, N, D, lp, rp, J, D, BAL | G, info, None, 0)
    assert n >= G and info[0] == 1 and info[1] == G, 'the plan argument must give the balanced split asked for'
    got = _run(case, BAL | G, cuda)
    _check_oracle(case, got)
    ref = _run_chunked(case, cuda)
    assert np.abs(ref[0] - got[0]).max() < 1e-5
    for name, a, b in zip(('g_emb', 'g_W', 'g_bias'), ref[1:], got[1:]):
        assert np.abs(a - b).max() <= 2e-5 * max(1.0, np.abs(a).max()), (name, np.abs(a - b).max())


def test_nothing_reads_or_writes_vc_after_the_last_iteration(cuda):
    """saved's last plane (Vc^R) pre-filled with NaN, forward and backward through the C
    ABI: the plane is still NaN afterwards and v and the gradients match the oracle, so
    the forward no longer writes it and nothing reads it."""
    from srf_amd import _lib
    L = _lib.lib()
    case = CASE_P
    B, T, N, D, lp, rp, J, it, mf = case
    emb, W, bias, gv = _inputs(case)
    te, tW, tb, tg = (torch.tensor(a, dtype=torch.float32, device=cuda) for a in (emb, W, bias, gv))
    args = (B, T, N, D, lp, rp, J, D, it, int(mf), BAL | 5)
    ws_args = args[:9] + (BAL | 5,)
    FJD = B * T * J * D
    n_saved = L.srf_route_dr_saved_floats(B, T, J, D, it)
    assert n_saved == 2 * it * FJD
    saved = torch.zeros(n_saved, device=cuda)
    saved[(2 * it - 1) * FJD:] = float('nan')

    def ptr(t):
        return ctypes.c_void_p(t.data_ptr())

    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    v = torch.empty((B, T, J, D), device=cuda)
    cpl = torch.empty(L.srf_route_dr_coupling_floats(*args[:9]), device=cuda)
    assert cpl.numel() > 0
    fws = L.srf_route_dr_fwd_workspace(*ws_args)
    ws = torch.empty(fws, device=cuda, dtype=torch.uint8)
    _lib.check(L.srf_route_dr_fwd_ex(ptr(te), ptr(tW), ptr(tb), *args, ptr(v), ptr(saved), ptr(cpl), ptr(ws), fws,
                                     stream), 'fwd')
    g_emb, g_W, g_b = torch.empty_like(te), torch.empty_like(tW), torch.empty_like(tb)
    bws = L.srf_route_dr_bwd_workspace(*ws_args)
    ws2 = torch.empty(bws, device=cuda, dtype=torch.uint8)
    _lib.check(L.srf_route_dr_bwd_ex(ptr(te), ptr(tW), ptr(tb), *args, ptr(saved), ptr(cpl), ptr(tg), ptr(g_emb),
                                     ptr(g_W), ptr(g_b), ptr(ws2), bws, stream), 'bwd')
    torch.cuda.synchronize()
    assert bool(torch.isnan(saved[(2 * it - 1) * FJD:]).all())
    assert bool(torch.isfinite(saved[:(2 * it - 1) * FJD]).all())
    _check_oracle(case, [t.cpu().double().numpy() for t in (v, g_emb, g_W, g_b)])
