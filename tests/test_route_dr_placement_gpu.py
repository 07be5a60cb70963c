"""The XCD placement of a balanced plan's spans (route_fwd32.h bal_place) on the GPU: which
block runs which span cannot change a sum.

Each case runs the forward and the backward through the C ABI twice, with the placement on
and off (srf_route_dr_set_bal_placement), on the shapes of
tests/test_route_dr_balanced_gpu.py with workgroup counts whose map is not the identity:
G not a multiple of 8 (9, 12, 36), gcd(n_ft, G) > 1 (CASE_P / CASE_4: n_ft 3 with 9, 12,
24, 36; CASE_NW4: n_ft 2; CASE_D16: n_ft 4) and gcd = 1 (CASE_P with 16).  v, saved, the
coupling storage, g_W and g_bias are bit-identical: every segment writes the same slab
slot from the same operands in the same order.  g_emb is accumulated with float atomics,
whose order follows the blocks, so it is held to the fp64 oracle at that file's tolerance.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests.test_route_dr_balanced_gpu import BAL, CASE_4, CASE_D16, CASE_NW4, CASE_P, _inputs, _oracle

pytestmark = pytest.mark.gpu

GS = (9, 12, 16, 24, 36)
CASES = {'p': CASE_P, 'tw4-masked': CASE_4, 'nw4-two-iterations': CASE_NW4, 'din16': CASE_D16}


def _units(case):
    B, T, N, D, lp, rp, J, it, mf = case
    return -(-B * T // 32) * N * (lp + rp + 1)


PLANS = [pytest.param(case, G, id=f'{name}-G{G}') for name, case in CASES.items() for G in GS if G <= _units(case)]


def _run(case, G, dev):
    """Forward and backward from stored couplings: v, saved, couplings, g_emb, g_W, g_bias."""
    from srf_amd import _lib
    L = _lib.lib()
    B, T, N, D, lp, rp, J, it, mf = case
    emb, W, bias, gv = _inputs(case)
    te, tW, tb, tg = (torch.tensor(a, dtype=torch.float32, device=dev) for a in (emb, W, bias, gv))
    args = (B, T, N, D, lp, rp, J, D, it, int(mf), BAL | G)
    ws_args = args[:9] + (BAL | G,)

    def ptr(t):
        return ctypes.c_void_p(t.data_ptr())

    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    # zero-filled: the regions no pass writes compare equal
    saved = torch.zeros(L.srf_route_dr_saved_floats(B, T, J, D, it), device=dev)
    cpl = torch.zeros(L.srf_route_dr_coupling_floats(*args[:9]), device=dev)
    assert cpl.numel() > 0
    v = torch.empty((B, T, J, D), device=dev)
    fws = L.srf_route_dr_fwd_workspace(*ws_args)
    ws = torch.empty(fws, device=dev, dtype=torch.uint8)
    _lib.check(L.srf_route_dr_fwd_ex(ptr(te), ptr(tW), ptr(tb), *args, ptr(v), ptr(saved), ptr(cpl), ptr(ws), fws,
                                     stream), 'fwd')
    g_emb, g_W, g_b = torch.empty_like(te), torch.empty_like(tW), torch.empty_like(tb)
    bws = L.srf_route_dr_bwd_workspace(*ws_args)
    ws2 = torch.empty(bws, device=dev, dtype=torch.uint8)
    _lib.check(L.srf_route_dr_bwd_ex(ptr(te), ptr(tW), ptr(tb), *args, ptr(saved), ptr(cpl), ptr(tg), ptr(g_emb),
                                     ptr(g_W), ptr(g_b), ptr(ws2), bws, stream), 'bwd')
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in
            dict(v=v, saved=saved, couplings=cpl, g_emb=g_emb, g_W=g_W, g_bias=g_b).items()}


@pytest.mark.parametrize('case,G', PLANS)
def test_placement_changes_no_sum(cuda, case, G):
    from srf_amd import _lib
    L = _lib.lib()
    B, T, N, D, lp, rp, J, it, mf = case
    geom = (B, T, N, D, lp, rp, J, D, BAL | G)
    info = (ctypes.c_int * 5)()
    n = L.srf_route_dr_split_table(*geom, info, None, 0)
    assert n >= G and info[0] == 1 and info[1] == G, 'the plan argument must give the balanced split asked for'
    m = (ctypes.c_int * G)()
    try:
        assert L.srf_route_dr_set_bal_placement(1) == 0
        assert L.srf_route_dr_split_placement(*geom, m, G) == G
        # (n_ft 2 with G 16 sorts into the identity; every other case moves blocks)
        print('blocks moved:', sum(int(w != b) for b, w in enumerate(m)), 'of', G)
        on = _run(case, G, cuda)
        assert L.srf_route_dr_set_bal_placement(0) == 0
        off = _run(case, G, cuda)
    finally:
        L.srf_route_dr_set_bal_placement(1)
    for k in ('v', 'saved', 'couplings', 'g_W', 'g_bias'):
        a, b = on[k].view(np.uint32), off[k].view(np.uint32)
        assert np.array_equal(a, b), (k, int((a != b).sum()))
    ref = _oracle(case)
    assert np.all(np.abs(on['v'] - ref[0]) <= 2e-5 * (1 + np.abs(ref[0])))
    for got in (on, off):
        for name, r in zip(('g_emb', 'g_W', 'g_bias'), ref[1:]):
            err = np.abs(got[name].astype(np.float64) - r).max()
            print(f'{name}: max err {err:.3e} (max |ref| {np.abs(r).max():.3e})')
            assert err <= 1e-4 * max(1.0, np.abs(r).max()), (name, err, np.abs(r).max())
