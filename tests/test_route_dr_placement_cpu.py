"""Placement of a balanced plan's spans on the XCDs (route_fwd32.h bal_place), checked on
the host through srf_route_dr_split_placement: no GPU.

Block b of a balanced pass runs workgroup map[b].  Workgroup w walks capsule
(p_w + k) % in_n at its step k, p_w = bal_first(w) % in_n, and the dispatcher deals blocks
round-robin over 8 XCDs, so the phases p_w of the blocks b = x (mod 8) decide which W slabs
XCD x holds in its L2 at any time.  The placement sorts the workgroups by phase, XCD-major:
the n_x workgroups of XCD x take n_x of the G / d distinct phase values in a row
(d = gcd(n_ft, G) workgroups share each), at most ceil(n_x / d) + 1 <= (n_x + d) / d + 1 of
them, d * in_n / G capsules apart, plus one capsule for the floors in bal_first.
"""
import ctypes
import math

import numpy as np
import pytest

from srf_amd import _lib

BAL = 1 << 20   # srf::kBalFlag

# (n_ft, in_n) -> B, T, N, D, lpad, rpad, J: frames = B * T, n_ft = ceil(frames / 32)
SHAPES = {
    (3, 12): (2, 40, 4, 32, 1, 1, 16),
    (2, 24): (1, 35, 8, 32, 1, 1, 8),
    (3, 72): (3, 30, 8, 16, 4, 4, 63),
    (7, 12): (7, 32, 4, 32, 1, 1, 16),
    (59, 80): (59, 32, 16, 32, 2, 2, 16),
    (175, 80): (28, 200, 16, 32, 2, 2, 16),
}
GS = [1, 3, 5, 6, 7, 8, 9, 12, 16, 24, 36, 64, 128, 255, 256]
CASES = [pytest.param(k, G, id=f'nft{k[0]}-in{k[1]}-G{G}') for k in SHAPES for G in GS if G <= k[0] * k[1]]


def _geom(key):
    B, T, N, D, lp, rp, J = SHAPES[key]
    assert (-(-B * T // 32), N * (lp + rp + 1)) == key
    return (B, T, N, D, lp, rp, J, D)


def _placement(key, G):
    L = _lib.lib()
    n = L.srf_route_dr_split_placement(*_geom(key), BAL | G, None, 0)
    assert n == G, L.srf_last_error()
    m = (ctypes.c_int * n)()
    assert L.srf_route_dr_split_placement(*_geom(key), BAL | G, m, n) == n
    return np.array(m, dtype=np.int64)


def _table(key, G):
    L = _lib.lib()
    info = (ctypes.c_int * 5)()
    n = L.srf_route_dr_split_table(*_geom(key), BAL | G, info, None, 0)
    assert n > 0 and info[0] == 1 and info[1] == G, L.srf_last_error()
    tab = (ctypes.c_int * (5 * n))()
    assert L.srf_route_dr_split_table(*_geom(key), BAL | G, info, tab, n) == n
    return list(info), np.array(tab, dtype=np.int64).reshape(n, 5)


def _arc(phases, in_n):
    """Length of the shortest circular arc of 0 .. in_n - 1 that holds every phase."""
    s = np.unique(phases)
    if len(s) == 1:
        return 0
    gaps = np.diff(np.concatenate([s, s[:1] + in_n]))
    return int(in_n - gaps.max())


@pytest.fixture
def placement_on():
    L = _lib.lib()
    try:
        assert L.srf_route_dr_set_bal_placement(1) == 0
        yield L
    finally:
        L.srf_route_dr_set_bal_placement(1)


@pytest.mark.parametrize('key,G', CASES)
def test_placement_is_a_permutation_with_neighbouring_phases_per_xcd(placement_on, key, G):
    n_ft, in_n = key
    U = n_ft * in_n
    m = _placement(key, G)
    assert sorted(m.tolist()) == list(range(G))
    if G <= 8:
        assert m.tolist() == list(range(G))
    d = math.gcd(n_ft, G)
    for x in range(min(8, G)):
        ws = m[x::8]
        n_x = (G - x + 7) // 8
        assert len(ws) == n_x
        arc = _arc((ws * U // G) % in_n, in_n)   # bal_first(w) % in_n
        bound = -(-in_n * (n_x + d) // G) + 1
        assert arc <= bound, (x, arc, bound, ws.tolist())


@pytest.mark.parametrize('key,G', CASES)
def test_setter_switches_the_map_and_leaves_the_segment_table(placement_on, key, G):
    L = placement_on
    on_map, on_tab = _placement(key, G), _table(key, G)
    assert L.srf_route_dr_set_bal_placement(0) == 0
    off_map, off_tab = _placement(key, G), _table(key, G)
    assert off_map.tolist() == list(range(G))
    assert on_tab[0] == off_tab[0] and np.array_equal(on_tab[1], off_tab[1])
    assert L.srf_route_dr_set_bal_placement(1) == 0
    assert np.array_equal(_placement(key, G), on_map)


def test_bench_inner_layer_arc():
    """The bench's inner layers (175 tiles x 80 capsules, G = 256): every XCD within 9
    capsules under the placement, 77 of the 80 with block b = workgroup b."""
    L = _lib.lib()
    key, G = (175, 80), 256
    try:
        arcs = {}
        for on in (1, 0):
            L.srf_route_dr_set_bal_placement(on)
            m = _placement(key, G)
            arcs[on] = max(_arc((m[x::8] * (175 * 80) // G) % 80, 80) for x in range(8))
        assert arcs == {1: 9, 0: 77}
    finally:
        L.srf_route_dr_set_bal_placement(1)


def test_chunked_plans_and_errors():
    L = _lib.lib()
    g = _geom((3, 12))
    m = (ctypes.c_int * 4)()
    assert L.srf_route_dr_split_placement(*g, 3, m, 4) == 0          # a chunked plan
    assert L.srf_route_dr_split_placement(*g, BAL | 36, m, 4) == 36   # more workgroups than capacity
    assert L.srf_route_dr_split_placement(*g, -1, m, 4) < 0
    assert L.srf_route_dr_split_placement(*g, BAL | 5, None, 4) < 0
    assert L.srf_route_dr_split_placement(1, 5, 2, 64, 1, 1, 4, 64, 0, m, 4) < 0   # not a 32x32-pass shape
