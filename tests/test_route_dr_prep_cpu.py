"""The numpy reference of the DR operand preparation (tests/prep_ref.py) against a direct
loop over (i, f, e), and the host query that locates the regions (no GPU)."""
import ctypes

import numpy as np

from tests import prep_ref as pr
from tests.test_route_dr_prep_gpu import CASES, REGIONS, _inputs


def test_reference_xT_matches_a_direct_loop():
    case = CASES[1]   # an utterance edge inside a 16-frame block, lpad != rpad
    B, T, N, D, lp, rp, J, it = case
    emb, W, bias = _inputs(case)
    in_n = N * (lp + rp + 1)
    ref, aw, bx = pr.regions(emb, W.reshape(in_n, J * D, D), bias.reshape(in_n, J * D), lp, rp, 256)
    loop = pr.xT_loop(emb, lp, rp, bx)
    assert loop.shape == ref['xT'].shape and loop.tobytes() == ref['xT'].tobytes()
    # frame 17 = (b 1, t 0): its left window rows lie in utterance 0 and are zero
    assert not ref['xT'][0:2 * N, 1, :, :, 1].any()
    assert ref['xT'][2 * N:, 1, 0, :, 1].all()


def test_reference_split_is_exact_to_the_third_term():
    rng = np.random.default_rng(3)
    a = rng.standard_normal(4096).astype(np.float32)
    e = pr.split_exp(a)
    assert 2.0 ** 13 <= np.abs(a).max() * 2.0 ** e < 2.0 ** 14
    hi, lo = pr.split2h(a, e)
    err = np.abs(a.astype(np.float64) * 2.0 ** e - hi.astype(np.float64) - lo.astype(np.float64))
    assert err.max() <= 2.0 ** -22 * np.abs(a).max() * 2.0 ** e
    assert pr.split_exp(np.zeros(4, np.float32)) == 0
    assert pr.split_exp(np.full(4, 2.0 ** 100, np.float32)) == -60
    b = pr.bf16_rne(np.array([1.0, 1.00390625, 1.01171875, -3.0], np.float32))   # ties to even
    assert list(b) == [0x3f80, 0x3f80, 0x3f82, 0xc040]


def test_operand_layout_locates_every_region_inside_the_coupling_storage():
    from srf_amd import _lib
    L = _lib.lib()
    for case in CASES:
        B, T, N, D, lp, rp, J, it = case
        out = (ctypes.c_longlong * 17)()
        _lib.check(L.srf_route_dr_operand_layout(B, T, N, D, lp, rp, J, D, it, out), 'operand_layout')
        total = L.srf_route_dr_coupling_floats(B, T, N, D, lp, rp, J, D, it)
        assert out[15] == 1 and out[16] == 1, case
        spans = sorted((out[2 * k], out[2 * k] + (out[2 * k + 1] + 3) // 4) for k in range(len(REGIONS)))
        assert spans[0][0] > 0 and spans[-1][1] <= total
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), (case, spans)
        in_n, JD = N * (lp + rp + 1), J * D
        assert out[12] % 64 == 0 and out[12] >= JD and out[13] == B * T * N * D + 32
        assert out[14] == (B * T + 15) // 16 * 16
        assert out[1] == 2 * in_n * out[12] * D * 2 and out[11] == in_n * D * out[14] * 4
    # a shape without coupling storage (one iteration) is refused
    out = (ctypes.c_longlong * 17)()
    assert L.srf_route_dr_operand_layout(1, 9, 4, 32, 1, 1, 8, 32, 1, out) != 0
