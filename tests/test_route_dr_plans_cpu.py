"""The host decisions of the DR layer (route_dr.hip: resolve), pinned against a recorded
fixture: no GPU.

For a grid of shapes that crosses every boundary the plan encodes (din 64 and J * dout > 1024
leave the 32x32 passes, iters 1 stores no couplings, iters <= 3 / <= 4 pick the gW / gx kernel
families, the frame count moves the cost models), tests/golden/dr_plans.json holds what the size
and plan queries of the C interface returned when the fixture was recorded.  The test asserts
exact equality, so a change to the plan code that moves a workspace offset, a coupling layout or
a default split shows up here before it reaches a GPU.

    SRF_LIB_PATH=<library to record from> python tests/test_route_dr_plans_cpu.py --write

rewrites the fixture (only for a change that is meant to move these values).
"""
import ctypes
import itertools
import json
import os
import sys

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'dr_plans.json')

BAL = 1 << 20   # srf::kBalFlag
PLAN_ARGS = (0, 1, 3, BAL | 5)
DINS = (8, 16, 32, 64)
JS = (4, 16, 32, 63)          # 63 x 32 > 1024: din 32 on the exact-fp32 passes
ITERS = (1, 2, 3, 4, 5)
BTS = ((1, 5), (2, 40), (28, 200))
NLRS = ((4, 1, 1), (8, 4, 4), (16, 2, 2))
COLUMNS = ('B', 'T', 'N', 'din', 'lpad', 'rpad', 'J', 'iters', 'auto_chunks', 'saved_floats', 'coupling_floats',
           'fwd_workspace', 'bwd_workspace', 'split_default', 'split_balanced')


def grid():
    """din x J x iters in full; of the nine (B, T) x (N, lpad, rpad) pairs each cell takes three,
    a Latin square shifted from cell to cell, so every pair meets every din, J and iters."""
    rows = []
    for (a, din), (b, J), (c, iters) in itertools.product(enumerate(DINS), enumerate(JS), enumerate(ITERS)):
        for k in range(3):
            rows.append(BTS[k] + NLRS[(k + a + b + c) % 3] + (din, J, iters))
    return rows


def record(L, B, T, N, lpad, rpad, din, J, iters):
    geom = (B, T, N, din, lpad, rpad, J, din)
    info = (ctypes.c_int * 5)()

    def split(plan):
        n = L.srf_route_dr_split_table(*geom, plan, info, None, 0)
        return list(info) if n >= 0 else n

    split_default, split_balanced = split(0), split(BAL | 5)
    # the balanced argument only where the split table accepts it
    args = [p for p in PLAN_ARGS if p != (BAL | 5) or isinstance(split_balanced, list)]
    return [B, T, N, din, lpad, rpad, J, iters,
            L.srf_route_dr_auto_chunks(*geom),
            L.srf_route_dr_saved_floats(B, T, J, din, iters),
            L.srf_route_dr_coupling_floats(*geom, iters),
            [L.srf_route_dr_fwd_workspace(*geom, iters, p) for p in args],
            [L.srf_route_dr_bwd_workspace(*geom, iters, p) for p in args],
            split_default, split_balanced]


def record_all():
    from srf_amd import _lib
    L = _lib.lib()
    return [record(L, *shape) for shape in grid()]


def test_plans_match_the_recorded_fixture():
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert golden['columns'] == list(COLUMNS)
    got = record_all()
    assert len(got) == len(golden['rows']) and 200 <= len(got) <= 400
    for g, want in zip(got, golden['rows']):
        assert g == want, dict(zip(COLUMNS, zip(g, want)))


def test_grid_crosses_the_decision_boundaries():
    """Both pass families, stored and recomputed couplings, balanced and chunked defaults."""
    with open(GOLDEN) as f:
        rows = [dict(zip(COLUMNS, r)) for r in json.load(f)['rows']]
    assert any(isinstance(r['split_default'], list) for r in rows) and any(r['split_default'] == -1 for r in rows)
    assert {r['coupling_floats'] > 0 for r in rows if r['iters'] > 1 and r['din'] <= 32} == {True, False}
    assert all(r['coupling_floats'] == 0 for r in rows if r['iters'] == 1 or r['din'] == 64)
    assert {r['auto_chunks'] >= BAL for r in rows} == {True, False}
    assert all(len(r['fwd_workspace']) == (4 if isinstance(r['split_balanced'], list) else 3) for r in rows)


if __name__ == '__main__':
    if sys.argv[1:] != ['--write']:
        sys.exit('usage: SRF_LIB_PATH=<library> python tests/test_route_dr_plans_cpu.py --write')
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    with open(GOLDEN, 'w') as f:
        f.write('{"columns": %s,\n "rows": [\n' % json.dumps(list(COLUMNS)))
        f.write(',\n'.join('  ' + json.dumps(r) for r in record_all()))
        f.write('\n]}\n')
    print(f'wrote {GOLDEN}')
