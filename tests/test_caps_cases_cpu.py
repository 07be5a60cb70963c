"""Preconditions of tests/test_caps_rows_gpu.py that need no GPU (tests/caps_cases.py):
the column-sum cases reach the route they are labelled with under the thresholds
restated beside the table, their integer inputs sum exactly in fp32, and no maxout
pair of a primary-capsule case is closer than fp32 can resolve."""
import numpy as np
import pytest

from tests import caps_cases as cc


@pytest.mark.parametrize('route,rows,n,slices,last', cc.COLSUM_CASES, ids=cc.colsum_ids())
def test_colsum_case_reaches_its_route(route, rows, n, slices, last):
    got, got_slices, rps = cc.colsum_route(rows, 2 * n)
    assert got == route
    if route == 'two':
        assert got_slices == slices and rows - (got_slices - 1) * rps == last
        assert got_slices <= cc.MAX_SLICES      # the scratch srf_capsnorm_params_workspace sizes
    else:
        assert slices is None and last is None


def test_colsum_cases_cover_every_route_and_edge():
    routes = {c[0] for c in cc.COLSUM_CASES}
    assert routes == {'single', 'one16', 'one64', 'two'}
    rows = {(c[0], c[1]) for c in cc.COLSUM_CASES}
    # both sides of each row threshold
    assert ('single', cc.SINGLE_MAX_ROWS) in rows and ('one16', cc.SINGLE_MAX_ROWS + 1) in rows
    assert ('one16', cc.ONE_MAX_ROWS) in rows and ('two', cc.ONE_MAX_ROWS + 1) in rows
    # both sides of each width threshold
    cb = {(c[0], cc.cblocks(2 * c[2])) for c in cc.COLSUM_CASES}
    assert ('one16', cc.ONE64_MIN_CBLOCKS - 1) in cb and ('one64', cc.ONE64_MIN_CBLOCKS) in cb
    assert ('two', cc.ONE_WIDE_CBLOCKS - 1) in cb and ('one64', cc.ONE_WIDE_CBLOCKS) in cb
    # a partial last slice, and a partial last column block of both colsum_one widths
    assert any(c[0] == 'two' and c[4] < -(-c[1] // c[3]) for c in cc.COLSUM_CASES)
    assert any(c[0] == 'one16' and (2 * c[2]) % 16 for c in cc.COLSUM_CASES)
    assert any(c[0] == 'one64' and (2 * c[2]) % 64 for c in cc.COLSUM_CASES)


@pytest.mark.parametrize('route,rows,n,slices,last', cc.COLSUM_CASES, ids=cc.colsum_ids())
def test_colsum_integer_sums_are_exact_in_fp32(route, rows, n, slices, last):
    assert cc.COLSUM_INT_RANGE * rows < 2 ** 24
    if rows * n <= 1 << 20:   # the draw itself, where it is small
        x = cc.colsum_exact_input(rows, n)
        assert x.dtype == np.float32 and np.all(x == np.round(x)) and np.abs(x).max() <= cc.COLSUM_INT_RANGE


@pytest.mark.parametrize('name', list(cc.PRIMARY_CASES))
def test_maxout_pairs_are_resolved_by_fp32(name):
    """Smallest float64 |v1 - v2| over the live positions >= 8 x the largest error of the
    float32 restatement of v1 - v2 (a condition on the inputs: the seeds of
    caps_cases.PRIMARY_CASES are chosen for it, and the large cases draw the few frames
    with a closer pair again).  The restatement sums in a written order, so the figures
    are the same on every machine: f4100 3.18e-4 against 1.78e-5, f2100 4.33e-4 against
    2.69e-5, the small cases 61 to 1100 times their error."""
    c, X, inp_len, P, drop, _ = cc.primary_inputs(name)
    assert (drop is not None) == (c['p'] > 0)
    gap, err = cc.maxout_gap(X, inp_len, P, drop)
    print(f'{name}: smallest |v1 - v2| {gap:.3e}, float32 error {err:.3e}, ratio {gap / err:.1f}')
    assert err > 0 and gap >= cc.MAXOUT_MARGIN * err, (gap, err)


def test_primary_case_shapes_reach_their_batches():
    """fchunk = ceil(F / 64) frames per wgrad chunk in batches of 32; 16 frames per g_X group."""
    f = {k: c['B'] * c['T'] for k, c in cc.PRIMARY_CASES.items()}
    assert f['f4100'] == 4100 and -(-4100 // 64) == 65 and 65 % 32 == 1 and 4100 % 16 == 4
    assert f['f2100'] == 2100 and -(-2100 // 64) == 33
    w = lambda c: 2 * c['PH'] * c['PD'] + 20 * c['PD']   # wpart columns
    assert cc.colsum_route(4100, w(cc.PRIMARY_CASES['f4100'])) == ('two', 64, 65)
    assert cc.colsum_route(2100, w(cc.PRIMARY_CASES['f2100']))[0] == 'one16'
    for c in cc.PRIMARY_CASES.values():
        assert len(c['lens']) == c['B'] and max(-(-l // 4) for l in c['lens']) == c['T']


def test_capsnorm_cases_reach_their_routes():
    want = ['one16', 'two', 'one16', 'two', 'two', 'two']
    for (B, T, J, D, head, p), route in zip(cc.CAPSNORM_CASES, want):
        n, F = J * D, B * T
        wave_bwd = not head and n in (256, 512, 1024)
        rows = -(-F // 4) if wave_bwd else F
        cols = 2 * n + (2 * J if head else 0)
        assert cc.colsum_route(rows, cols)[0] == route, (B, T, J, D)
        assert F * n <= 17_000_000
