"""The work split of the DR routing passes r >= 1 (route_fwd32.hip: fwd32_plan, SegWalk),
checked on the host from the segment table srf_route_dr_split_table returns: no GPU.

A plan is either chunked (n_ftiles * n_chunks workgroups, one i-chunk each) or balanced
(G persistent workgroups, each a contiguous span of the units u = tile * in_n + capsule,
cut into segments at the tile edges).  A small shape takes a balanced plan through the plan
argument BAL | G, the encoding srf_route_dr_auto_chunks returns for the bench's inner layers.
"""
import ctypes

import numpy as np
import pytest

from srf_amd import _lib

BAL = 1 << 20   # srf::kBalFlag
AUTO_INNER = BAL | 256   # the default plan of the C4 inner layers

# B, T, N, D, lpad, rpad, J, iters, mask_first: the shapes of tests/test_route_dr_balanced_gpu.py
SMALL = [
    (2, 40, 4, 32, 1, 1, 16, 3, False),
    (2, 40, 4, 32, 1, 1, 32, 3, True),
    (1, 35, 8, 32, 1, 2, 8, 2, True),
    (3, 37, 8, 16, 4, 4, 63, 3, True),
]
# the two C4 bench layers (tests/test_parity_scale_gpu.py): 5,600 frames, 80 input capsules
BENCH = [
    (28, 200, 16, 32, 2, 2, 16, 3, False),
    (28, 200, 16, 32, 2, 2, 32, 3, True),
]


def _geom(case):
    B, T, N, D, lp, rp, J, it, mf = case
    return (B, T, N, D, lp, rp, J, D)


def _units(case):
    B, T, N, D, lp, rp, J, it, mf = case
    in_n = N * (lp + rp + 1)
    return -(-B * T // 32), in_n


def _table(case, plan):
    L = _lib.lib()
    info = (ctypes.c_int * 5)()
    n = L.srf_route_dr_split_table(*_geom(case), plan, info, None, 0)
    assert n > 0, L.srf_last_error()
    tab = (ctypes.c_int * (5 * n))()
    assert L.srf_route_dr_split_table(*_geom(case), plan, info, tab, n) == n
    keys = ('balanced', 'workgroups', 'units', 'slots', 'plan')
    return dict(zip(keys, info)), np.array(tab, dtype=np.int64).reshape(n, 5)


def _check_table(case, plan):
    """Every (tile, capsule) once; slots of a tile distinct and below the slot count; the
    workspaces hold that many slabs.  Returns (info, table)."""
    L = _lib.lib()
    B, T, N, D, lp, rp, J, it, mf = case
    n_ft, in_n = _units(case)
    info, tab = _table(case, plan)
    cover = np.zeros((n_ft, in_n), dtype=np.int64)
    slots = {}
    for w, ft, i0, i1, slot in tab:
        assert 0 <= w < info['workgroups'] and 0 <= ft < n_ft and 0 <= i0 <= i1 <= in_n, (w, ft, i0, i1)
        cover[ft, i0:i1] += 1
        assert 0 <= slot < info['slots'], (w, ft, slot, info)
        assert slot not in slots.setdefault(ft, set()), (w, ft, slot)
        slots[ft].add(slot)
    assert np.all(cover == 1), np.argwhere(cover != 1)[:8]
    # a tile's slots are 0 .. count - 1: the finish sums exactly the first `count` slabs
    for ft, s in slots.items():
        assert s == set(range(len(s))), (ft, sorted(s))
    # a workgroup's segments in the order it walks them: tiles ascending, contiguous units
    for w in np.unique(tab[:, 0]):
        seg = tab[tab[:, 0] == w]
        u0 = seg[:, 1] * in_n + seg[:, 2]
        u1 = seg[:, 1] * in_n + seg[:, 3]
        assert np.all(u0[1:] == u1[:-1]), (w, seg)
    slab = B * T * J * D * 4
    need = max(len(s) for s in slots.values()) * slab
    assert L.srf_route_dr_fwd_workspace(*_geom(case), it, info['plan']) >= need
    assert L.srf_route_dr_bwd_workspace(*_geom(case), it, info['plan']) >= need
    return info, tab


@pytest.mark.parametrize('case', SMALL)
def test_forced_balanced_plans_cover_the_work_once(case):
    n_ft, in_n = _units(case)
    U = n_ft * in_n
    for G in (1, 3, 5, 7, U):
        info, tab = _check_table(case, BAL | G)
        assert info['balanced'] == 1 and info['workgroups'] == G and info['units'] == U
        assert info['plan'] == BAL | G
        # the spans are the floor split: workgroup w owns [w U // G, (w + 1) U // G)
        for w in range(G):
            seg = tab[tab[:, 0] == w]
            assert seg[0, 1] * in_n + seg[0, 2] == w * U // G
            assert seg[-1, 1] * in_n + seg[-1, 3] == (w + 1) * U // G


def test_issue_example_segment_counts():
    """(2, 40, 4, 32, 1, 1, 16): 3 tiles of 12 capsules, U = 36.  G = 5: the tiles have 2, 3
    and 2 segments; G = 7: a 1-capsule segment at a tile's start; G = 36: all of them are."""
    case = SMALL[0]
    assert _units(case) == (3, 12)
    _, tab = _table(case, BAL | 5)
    assert [int((tab[:, 1] == ft).sum()) for ft in range(3)] == [2, 3, 2]
    _, tab = _table(case, BAL | 7)
    assert any(i0 == 0 and i1 == 1 for _, _, i0, i1, _ in tab)
    _, tab = _table(case, BAL | 36)
    assert len(tab) == 36 and np.all(tab[:, 3] - tab[:, 2] == 1)
    _, tab = _table(case, BAL | 1)
    assert tab[:, :4].tolist() == [[0, 0, 0, 12], [0, 1, 0, 12], [0, 2, 0, 12]]


@pytest.mark.parametrize('case', SMALL + BENCH)
def test_default_and_chunked_plans(case):
    """The default plan and explicit chunk counts go through the same table; an explicit
    chunk count stays chunked, and the default's plan argument reproduces the default."""
    L = _lib.lib()
    auto = L.srf_route_dr_auto_chunks(*_geom(case))
    info, tab = _check_table(case, 0)
    assert info['plan'] == auto and auto > 1
    info2, tab2 = _check_table(case, auto)
    assert info2 == info and np.array_equal(tab, tab2)
    n_ft, in_n = _units(case)
    for nc in (1, 3, 4, 5, in_n):
        info, tab = _check_table(case, nc)
        assert info['balanced'] == 0 and info['plan'] == nc and info['workgroups'] == n_ft * nc
        assert info['slots'] == nc


@pytest.mark.parametrize('case', BENCH)
def test_bench_shapes_balanced_over_the_resident_workgroups(case):
    """175 tiles x 80 capsules, plan BAL | 0 (as many workgroups as are resident): G = 256,
    at most 3 segments per tile, and every workgroup within one unit of U / G = 54.7 (no
    boundary is snapped)."""
    info, tab = _check_table(case, BAL)
    U = 175 * 80
    assert info == dict(balanced=1, workgroups=256, units=U, slots=3, plan=BAL | 256)
    per_tile = np.bincount(tab[:, 1], minlength=175)
    assert per_tile.min() >= 2 and per_tile.max() <= 3
    load = np.bincount(tab[:, 0], weights=tab[:, 3] - tab[:, 2], minlength=256)
    assert np.all(np.abs(load - U / 256) < 1.0), (load.min(), load.max())
    assert np.bincount(tab[:, 0], minlength=256).max() <= 2   # a span crosses at most one tile edge


def test_default_plans_of_the_bench_shapes():
    """What the cost model picks where it was measured: the balanced split for
    the inner layers (two row tiles per wave), 4 uniform chunks for layer 6 (four row
    tiles), where the balanced split measured slower."""
    L = _lib.lib()
    assert L.srf_route_dr_auto_chunks(*_geom(BENCH[0])) == AUTO_INNER
    assert L.srf_route_dr_auto_chunks(*_geom(BENCH[1])) == 4


def test_bad_plan_arguments_are_errors():
    L = _lib.lib()
    info = (ctypes.c_int * 5)()
    case = SMALL[0]
    in_n = _units(case)[1]
    assert L.srf_route_dr_split_table(*_geom(case), in_n + 1, info, None, 0) < 0
    assert L.srf_route_dr_split_table(*_geom(case), -1, info, None, 0) < 0
    # din 64 has no 32x32 passes, hence no table and no balanced plan
    assert L.srf_route_dr_split_table(1, 5, 2, 64, 1, 1, 4, 64, 0, info, None, 0) < 0
