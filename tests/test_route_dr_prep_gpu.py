"""What the DR forward's operand preparation writes (route_fwd32.hip: absmax_kernel and
prep32_onepass_kernel), byte for byte against tests/prep_ref.py.

srf_route_dr_fwd_ex runs with coupling storage; srf_route_dr_operand_layout says where
Ws, bs, xs, hdr, WT and xT lie in it.  Every case must take the split-fp16 backward
formats (asserted, none skipped).  The shapes are the smallest where the one-pass
indexing can go wrong: F below one 16-frame block, utterance edges inside a block and
inside a tile's halo, lpad != rpad, a one-sided window, N not a power of two, several
64-frame tiles with a ragged last one, JD < JDp, the 1024-row layer.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import prep_ref as pr

pytestmark = pytest.mark.gpu

# B, T, N, D, lpad, rpad, J, iters
CASES = [
    (1, 9, 4, 32, 1, 1, 8, 3),
    (2, 17, 3, 32, 2, 1, 6, 3),
    (3, 61, 8, 32, 2, 2, 12, 3),
    (1, 70, 5, 32, 0, 2, 5, 3),
    (1, 20, 2, 32, 1, 1, 32, 3),
    (4, 13, 2, 32, 2, 2, 4, 2),
]
REGIONS = ('Ws', 'bs', 'xs', 'hdr', 'WT', 'xT')


def _mk(case, seed):   # as tests/test_route_dr_gpu.py
    B, T, N, D, lp, rp, J, it = case
    rng = np.random.default_rng(seed)
    in_n = N * (lp + rp + 1)
    emb = rng.standard_normal((B, T, N, D)) * 0.5
    W = rng.standard_normal((in_n, J, D, D)) * 0.1
    bias = rng.standard_normal((in_n, J, D)) * 0.1
    return [a.astype(np.float32) for a in (emb, W, bias)]


@functools.lru_cache(maxsize=None)
def _inputs(case):
    return _mk(case, 7)


def _layout(case):
    from srf_amd import _lib
    B, T, N, D, lp, rp, J, it = case
    out = (ctypes.c_longlong * 17)()
    _lib.check(_lib.lib().srf_route_dr_operand_layout(B, T, N, D, lp, rp, J, D, it, out), 'operand_layout')
    lay = {k: (out[2 * n], out[2 * n + 1]) for n, k in enumerate(REGIONS)}
    return lay, {'JDp': out[12], 'xplane': out[13], 'Fp': out[14], 'wt16': out[15], 'xt16': out[16]}


def _forward(case, emb, W, bias, dev, with_couplings=True):
    """v and (with_couplings) the coupling storage as bytes, through the C ABI."""
    from srf_amd import _lib
    L = _lib.lib()
    B, T, N, D, lp, rp, J, it = case
    te, tW, tb = (torch.tensor(a, dtype=torch.float32, device=dev) for a in (emb, W, bias))
    args = (B, T, N, D, lp, rp, J, D, it, 0, 0)
    plan = L.srf_route_dr_auto_chunks(*args[:8])
    args = args[:10] + (plan,)

    def ptr(t):
        return ctypes.c_void_p(t.data_ptr()) if t is not None else None

    saved = torch.zeros(L.srf_route_dr_saved_floats(B, T, J, D, it), device=dev)
    v = torch.empty((B, T, J, D), device=dev)
    cpl = None
    if with_couplings:
        n = L.srf_route_dr_coupling_floats(*args[:9])
        assert n > 0
        cpl = torch.full((n,), float('nan'), device=dev)
    fws = L.srf_route_dr_fwd_workspace(*args[:9], plan)
    ws = torch.empty(fws, device=dev, dtype=torch.uint8)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(L.srf_route_dr_fwd_ex(ptr(te), ptr(tW), ptr(tb), *args, ptr(v), ptr(saved), ptr(cpl), ptr(ws), fws,
                                     stream), 'fwd')
    torch.cuda.synchronize()
    return v.cpu().numpy(), (cpl.cpu().numpy().view(np.uint8) if with_couplings else None)


def _check(case, emb, W, bias, dev):
    B, T, N, D, lp, rp, J, it = case
    lay, info = _layout(case)
    assert info['wt16'] == 1 and info['xt16'] == 1, 'the case must take the split-fp16 formats'
    assert info['Fp'] == (B * T + 15) // 16 * 16 and info['xplane'] == B * T * N * D + 32
    in_n = N * (lp + rp + 1)
    ref, aw, bx = pr.regions(emb, W.reshape(in_n, J * D, D), bias.reshape(in_n, J * D), lp, rp, info['JDp'])
    v, cpl = _forward(case, emb, W, bias, dev)
    assert np.isfinite(v).all()
    for name in REGIONS:
        off, nbytes = lay[name]
        want = ref[name].tobytes()
        assert nbytes == len(want), (name, nbytes, len(want))
        got = cpl[4 * off:4 * off + nbytes].tobytes()
        if got != want:
            g = np.frombuffer(got, np.uint16 if name != 'hdr' else np.uint32)
            w = np.frombuffer(want, g.dtype)
            bad = np.flatnonzero(g != w)
            raise AssertionError(f'{name}: {bad.size} of {g.size} words differ, first at {bad[:8]} '
                                 f'(got {g[bad[:4]]}, want {w[bad[:4]]})')
    return aw, bx


@pytest.mark.parametrize('case', CASES, ids=[f'case{k}' for k in range(len(CASES))])
def test_prepared_operands_match_the_definition(cuda, case):
    _check(case, *_inputs(case), cuda)


def test_scaled_operands_shift_the_exponents(cuda):
    """emb 2^-20 and W 2^9: the split exponents move by +20 and -9 (to 32 and 6 with these
    inputs), so every plane is scaled by another power of two than in the cases above and
    the header's 2^-(aw+bx) is far from 1."""
    case = CASES[2]
    emb, W, bias = _inputs(case)
    aw, bx = _check(case, emb * np.float32(2.0 ** -20), W * np.float32(2.0 ** 9), bias, cuda)
    assert (aw, bx) == (pr.split_exp(W) - 9, pr.split_exp(emb) + 20) and aw != 0 and bx != 0


def test_all_zero_emb(cuda):
    case = CASES[2]
    emb, W, bias = _inputs(case)
    aw, bx = _check(case, np.zeros_like(emb), W, bias, cuda)
    assert bx == 0


def test_forward_without_coupling_storage_gives_the_same_v(cuda):
    case = CASES[2]
    v1, _ = _forward(case, *_inputs(case), cuda)
    v0, _ = _forward(case, *_inputs(case), cuda, with_couplings=False)
    assert v0.tobytes() == v1.tobytes()
