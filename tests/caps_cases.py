"""Shapes, seeds and input builders shared by tests/test_caps_cases_cpu.py and
tests/test_caps_rows_gpu.py, so that the CPU preconditions are checked on the
bytes the GPU tests use.

Three tables: the column-sum shapes (one per route of srf::colsum and per edge of
a route), the primary-capsule cases past the small-F regime, and the capsnorm /
head cases whose partial rows pass 128 and 4096."""
import numpy as np
import torch

from tests import torch_ref as tr

# ---------------------------------------------------------------- column sum
# The route thresholds of srf::colsum (srf_amd/csrc/reduce.hip), restated:
#   rows <= 128                                   one pass of colsum_stage2
#   rows <= 4096 or cblocks >= 128, cblocks < 64  colsum_one<16>
#   rows <= 4096 or cblocks >= 128, cblocks >= 64 colsum_one<64>
#   otherwise                                     colsum_stage1 + colsum_stage2 with
#     slices = min(64, ceil(1024 / cblocks), max(1, rows / 16)), then
#     rows_per_slice = ceil(rows / slices), slices = ceil(rows / rows_per_slice)
# where cblocks = ceil(cols / 64).  A change to one of them in reduce.hip orphans
# the cases below whose comment quotes it (test_caps_cases_cpu.py checks the labels
# against this restatement, not against the library).
SINGLE_MAX_ROWS = 128
ONE_MAX_ROWS = 4096
ONE_WIDE_CBLOCKS = 128
ONE64_MIN_CBLOCKS = 64
MAX_SLICES = 64
SLICE_CBLOCK_BUDGET = 1024
MIN_ROWS_PER_SLICE = 16


def cblocks(cols):
    return -(-cols // 64)


def colsum_route(rows, cols):
    """(route, slices, rows_per_slice); the last two are None unless two-stage."""
    if rows <= SINGLE_MAX_ROWS:
        return 'single', None, None
    cb = cblocks(cols)
    if rows <= ONE_MAX_ROWS or cb >= ONE_WIDE_CBLOCKS:
        return ('one16' if cb < ONE64_MIN_CBLOCKS else 'one64'), None, None
    slices = max(1, min(MAX_SLICES, -(-SLICE_CBLOCK_BUDGET // cb)))
    slices = min(slices, max(1, rows // MIN_ROWS_PER_SLICE))
    rps = -(-rows // slices)
    return 'two', -(-rows // rps), rps


# (route, rows, n, slices, rows in the last slice); cols = 2 n.  Each is the smallest
# shape that reaches its route or an edge of it.
COLSUM_CASES = [
    # rows <= 128: lower threshold; cols = 26, cblocks = 1
    ('single', 1, 13, None, None),
    # rows <= 128: upper threshold
    ('single', 128, 13, None, None),
    # 129 > 128, cblocks = 1 < 64: smallest row count of colsum_one<16>; 26 columns are
    # two 16-column blocks, the last with 10 live columns; 64 row lanes, 129 = 2 * 64 + 1
    ('one16', 129, 13, None, None),
    # 4096 * 64 = 256 K: the last row count before the two-stage route
    ('one16', 4096, 13, None, None),
    # cols = 4032, cblocks = 63: widest slab still <16>; 1030 = 16 * 64 + 6 rows, not a
    # multiple of the 64 row lanes
    ('one16', 1030, 2016, None, None),
    # cols = 4034, cblocks = 64: first <64> width, 2 live columns in the last block
    ('one64', 129, 2017, None, None),
    # <64> has 16 row lanes; 1030 = 64 * 16 + 6
    ('one64', 1030, 2017, None, None),
    # rows > 4096 but cols = 8130, cblocks = 128 >= 128: colsum_one<64> by width (133 MB)
    ('one64', 4097, 4065, None, None),
    # 4097 > 4096, cblocks = 1: min(64, 1024, 256) = 64 slices of ceil(4097 / 64) = 65
    # rows, 63 * 65 = 4095, so the last slice holds 2
    ('two', 4097, 8, 64, 2),
    # cols = 2048, cblocks = 32: 1024 / 32 = 32 slices of ceil(4097 / 32) = 129 rows,
    # 31 * 129 = 3999, so the last holds 98
    ('two', 4097, 1024, 32, 98),
    # cols = 8128, cblocks = 127 (the widest two-stage slab): ceil(1024 / 127) = 9 slices
    # of ceil(4097 / 9) = 456 rows, 8 * 456 = 3648, so the last holds 449
    ('two', 4097, 4064, 9, 449),
    # the C3 workload's own shape (F = 28 * 200, n = 1024): 32 slices of exactly 175
    ('two', 5600, 1024, 32, 175),
]

COLSUM_INT_RANGE = 64   # exact case: integers in [-64, 64]; 64 * rows < 2^24 keeps fp32 exact


def colsum_ids():
    return [f'{r}-{rows}x{2 * n}' for r, rows, n, _, _ in COLSUM_CASES]


def colsum_exact_input(rows, n):
    """[rows, 2n] float32 of integers uniform in [-64, 64]."""
    rng = np.random.default_rng(1000 + rows + n)
    return rng.integers(-COLSUM_INT_RANGE, COLSUM_INT_RANGE + 1, size=(rows, 2 * n), dtype=np.int8).astype(np.float32)


def colsum_float_input(rows, n):
    """[rows, 2n] float32: standard normal times 10^U(-3, 3) per column."""
    rng = np.random.default_rng(2000 + rows + n)
    scale = (10.0 ** rng.uniform(-3, 3, size=2 * n)).astype(np.float32)
    x = rng.standard_normal((rows, 2 * n), dtype=np.float32)
    x *= scale
    return x


# ---------------------------------------------------------------- primary capsules
# name -> B, T, lens, X's trailing shape (F2, C), PH, PD, p (input dropout; the encaps
# dropout is 0.2 whenever p > 0, as in test_primary_caps), seed of X and of g_z.
# The inputs are chosen for the maxout precondition (maxout_gap): the small cases by
# their seed alone; redraw=True draws again the few frames that hold a pair too close
# (_widen_maxout), which no seed avoids at these sizes.
PRIMARY_CASES = {
    # F = 4100: fchunk = ceil(4100 / 64) = 65, wgrad batches of 32, 32, 1; 4100 = 256 * 16
    # + 4, so the last proj_bwd_x_vec frame group holds 4; wpart has 2 * 32 + 20 * 8 = 224
    # columns (cblocks = 4) and 4100 > 4096 rows: two-stage, min(64, 256, 256) = 64 slices
    # of 65 rows, the last holds 5
    'f4100': dict(B=2, T=2050, lens=[8200, 6001], F2=31, C=64, PH=4, PD=8, p=0.0, seed=30, redraw=True),
    # F = 2100: fchunk = 33, batches of 32 and 1; wpart has 2 * 512 + 20 * 32 = 1664
    # columns, cblocks = 26 < 64 and 128 < 2100 <= 4096: colsum_one<16>
    'f2100': dict(B=3, T=700, lens=[2800, 2311, 1202], F2=31, C=64, PH=16, PD=32, p=0.2, seed=7, redraw=True),
    # the generic kernels, at test_primary_caps' own B = 3, T = 11:
    # PH = 12: proj_fwd_kernel in output groups of 8 + 4, proj_bwd_x_kernel, the MFMA
    # wgrad with its pok mask (12 of 16 columns live)
    'ph12': dict(B=3, T=11, lens=[44, 37, 20], F2=31, C=64, PH=12, PD=8, p=0.2, seed=1),
    # PH = 24 > 16: proj_bwd_w_kernel in two passes of 16 + 8 (and the generic forward
    # in groups of 8 + 8 + 8, the generic g_X)
    'ph24': dict(B=3, T=11, lens=[44, 37, 20], F2=31, C=64, PH=24, PD=8, p=0.2, seed=2),
    # K = 35, not a multiple of 4: generic forward and g_X; the MFMA wgrad's third
    # 16-row K tile holds 3 live rows
    'k35': dict(B=3, T=11, lens=[44, 37, 20], F2=5, C=7, PH=8, PD=16, p=0.2, seed=1),
    # K = 20: the MFMA forward with Kq = 16, so 2 of its 16 K-waves live, the second
    # with 4 of its 16 columns
    'k20': dict(B=3, T=11, lens=[44, 37, 20], F2=5, C=4, PH=8, PD=16, p=0.2, seed=3),
}
PRIMARY_DROP_SEED = 99
REDRAW_MARGIN = 16   # _widen_maxout's own threshold: headroom over MAXOUT_MARGIN
MAXOUT_MARGIN = 8   # smallest float64 |v1 - v2| >= 8 x the float32 restatement's error of v1 - v2


def primary_params(K, PH, PD):
    """The parameter draws of test_primary_caps (float64)."""
    g = torch.Generator().manual_seed(1)
    return {'proj_kernel': torch.randn(K, PH, generator=g, dtype=torch.float64) * 0.05,
            'proj_bias': torch.randn(PH, generator=g, dtype=torch.float64) * 0.1,
            'encaps1_kernel': torch.randn(3, 3, 1, PD, generator=g, dtype=torch.float64) * 0.3,
            'encaps1_bias': torch.randn(PD, generator=g, dtype=torch.float64) * 0.1,
            'encaps2_kernel': torch.randn(3, 3, 1, PD, generator=g, dtype=torch.float64) * 0.3,
            'encaps2_bias': torch.randn(PD, generator=g, dtype=torch.float64) * 0.1,
            'ln_input_gamma': 1 + 0.1 * torch.randn(PH * PD, generator=g, dtype=torch.float64),
            'ln_input_beta': 0.1 * torch.randn(PH * PD, generator=g, dtype=torch.float64)}


def primary_inputs(name, seed=None):
    """(case, X float64 [B,T,F2,C], inp_len int32, P, drop or None, g_z float64) of a case.
    X and g_z are float32-representable, so both sides start from the same numbers."""
    c = PRIMARY_CASES[name]
    B, T, PH, PD = c['B'], c['T'], c['PH'], c['PD']
    rng = np.random.default_rng(c['seed'] if seed is None else seed)
    X = rng.standard_normal((B, T, c['F2'], c['C'])).astype(np.float32).astype(np.float64)
    gz = rng.standard_normal((B, T, PH, PD)).astype(np.float32).astype(np.float64)
    P = {k: v.float().double() for k, v in primary_params(c['F2'] * c['C'], PH, PD).items()}
    drop = None
    if c['p'] > 0:
        s = PRIMARY_DROP_SEED
        drop = {'encaps1': torch.tensor(tr.dropout_mult(s, 4, (B, T, PH, PD), 0.2)),
                'encaps2': torch.tensor(tr.dropout_mult(s, 5, (B, T, PH, PD), 0.2)),
                'input': torch.tensor(tr.dropout_mult(s, 6, (B, T, PH * PD), c['p']))}
    inp_len = np.array(c['lens'], dtype=np.int32)
    if c.get('redraw'):
        _widen_maxout(X, inp_len, P, drop, rng)
    return c, X, inp_len, P, drop, gz


def _maxout_branches(X, P, drop):
    """v1, v2 of tr.primary_caps (the two conv outputs after their dropout) in float64."""
    Xt = torch.tensor(X)
    B, T = Xt.shape[:2]
    e = (Xt.reshape(B, T, -1) @ P['proj_kernel'] + P['proj_bias']).unsqueeze(-1)
    v1 = tr.conv2d_same(e, P['encaps1_kernel'], P['encaps1_bias'], 1)
    v2 = tr.conv2d_same(e, P['encaps2_kernel'], P['encaps2_bias'], 1)
    if drop is not None:
        v1 = v1 * drop['encaps1']
        v2 = v2 * drop['encaps2']
    return v1, v2


def _maxout_branches_f32(X, P, drop):
    """The same in float32, from elementwise products and sums only, in a written order:
    the projection adds its K products one after another, each conv its nine taps in
    (dt, dp) order.  A float32 matmul sums in an order that depends on the BLAS, the CPU
    and the thread count (the error of v1 - v2 of case f4100 came out as 6.4e-6 on one
    machine and 1.8e-5 on another), so it cannot state a precondition; plain sequential
    summation is the same on every machine and is the least accurate order of the lot."""
    f32 = torch.float32
    B, T = X.shape[:2]
    Xk = torch.tensor(X, dtype=f32).reshape(B * T, -1).t().contiguous()   # [K, F]
    W = P['proj_kernel'].to(f32)
    acc = torch.zeros(B * T, W.shape[1], dtype=f32)
    for k in range(W.shape[0]):
        acc = acc + Xk[k][:, None] * W[k]
    e = (acc + P['proj_bias'].to(f32)).reshape(B, T, -1)
    PH = e.shape[2]
    ep = torch.nn.functional.pad(e, (1, 1, 1, 1))
    out = []
    for k in ('encaps1', 'encaps2'):
        Kk, v = P[k + '_kernel'].to(f32), P[k + '_bias'].to(f32).expand(B, T, PH, -1)
        for dt in range(3):
            for dp in range(3):
                v = v + ep[:, dt:dt + T, dp:dp + PH, None] * Kk[dt, dp, 0]
        out.append(v * drop[k].to(f32) if drop is not None else v)
    return out


def _maxout_diffs(X, inp_len, P, drop):
    """v1 - v2 in float64, the same from the float32 restatement, and the mask of the
    positions where the selection matters."""
    with torch.no_grad():
        a1, a2 = _maxout_branches(X, P, drop)
        b1, b2 = _maxout_branches_f32(X, P, drop)
        T = a1.shape[1]
        live = tr.time_mask(torch.tensor(inp_len), 4, T, torch.float64)[:, :, None, None].expand_as(a1) > 0
        if drop is not None:
            live = live & ~((drop['encaps1'] == 0) & (drop['encaps2'] == 0))
        return a1 - a2, (b1 - b2).double(), live


def maxout_gap(X, inp_len, P, drop):
    """(gap, err): the smallest float64 |v1 - v2| and the largest |(v1 - v2)_f32 -
    (v1 - v2)_f64| over the positions where the selection matters: valid in time, and
    not dropped in both branches (there v1 = v2 = 0 on every side and no gradient
    flows).  A position dropped in one branch counts, its gap being the other's |v|."""
    d64, d32, live = _maxout_diffs(X, inp_len, P, drop)
    return d64[live].abs().min().item(), (d32 - d64)[live].abs().max().item()


def _widen_maxout(X, inp_len, P, drop, rng):
    """Redraw (from rng, in place) the frames of X at which some live |v1 - v2| is below
    REDRAW_MARGIN x the float32 error, until none is.  With 10^5 to 10^6 comparisons a
    seed alone does not give the margin: the first draw of f4100 leaves 4 of 113 632 live
    pairs closer than 8 x the error (9 closer than 16 x, in 9 frames of 4100), that of
    f2100 40 of 775 901 (90, in 88 frames of 2100).  Every position stays in the
    comparison; only its input changes, and the result is a function of the seed."""
    for _ in range(50):
        d64, d32, live = _maxout_diffs(X, inp_len, P, drop)
        err = (d32 - d64)[live].abs().max().item()
        bad = (live & (d64.abs() < REDRAW_MARGIN * err)).any(-1).any(-1).numpy()
        if not bad.any():
            return
        for b, t in zip(*np.nonzero(bad)):
            X[b, t] = rng.standard_normal(X.shape[2:]).astype(np.float32)
    raise AssertionError('the maxout gaps did not widen in 50 rounds')


# ---------------------------------------------------------------- capsnorm and head
# (B, T, J, D, head, p): what the backward's column sum sees
CAPSNORM_CASES = [
    # n = 256: wave kernels, 4 frames per wave; 513 frames give 129 partial rows (the last
    # holds 1 frame): colsum_one<16> over 512 columns
    (3, 171, 16, 16, False, 0.1),
    # 16388 frames give 4097 partial rows: two-stage, 512 columns, cblocks = 8, 64 slices
    # of 65, the last holds 2; 17 MB of input
    (4, 4097, 16, 16, False, 0.0),
    # n = 128: block kernel, one partial row per frame; 129 rows: colsum_one<16>
    (1, 129, 8, 16, False, 0.1),
    # block kernel, 4097 rows: two-stage, 256 columns, 64 slices of 65
    (1, 4097, 8, 16, False, 0.1),
    # head, n = 1008: block kernels; 2 * 1008 + 2 * 63 = 2142 columns, cblocks = 34,
    # ceil(1024 / 34) = 31 slices of 133 rows, the last holds 107; the ColSplit scatter
    # into four outputs of widths 1008, 1008, 63, 63
    (1, 4097, 63, 16, True, 0.1),
    # head, n = 1024: wave forward, block backward; 2 * 1024 + 2 * 32 = 2112 columns,
    # cblocks = 33, 32 slices of 129
    (1, 4097, 32, 32, True, 0.0),
]
CAPSNORM_SEED, CAPSNORM_LAYER = 5, 2


def capsnorm_inputs(B, T, J, D, p, seed=CAPSNORM_SEED, layer=CAPSNORM_LAYER, rng_seed=3):
    """test_capsnorm_and_head's draws at another shape: v, (gamma_mid, beta_mid,
    gamma_out, beta_out), dropout multiplier or None, the loss weights' generator."""
    rng = np.random.default_rng(rng_seed)
    v = (rng.standard_normal((B, T, J, D)) * 0.3).astype(np.float32).astype(np.float64)
    g = torch.Generator().manual_seed(2)
    gm = 1 + 0.1 * torch.randn(J * D, generator=g, dtype=torch.float64)
    bm = 0.1 * torch.randn(J * D, generator=g, dtype=torch.float64)
    go = 1 + 0.1 * torch.randn(J, generator=g, dtype=torch.float64)
    bo = 0.1 * torch.randn(J, generator=g, dtype=torch.float64)
    params = [t.float().double() for t in (gm, bm, go, bo)]
    drop = torch.tensor(tr.dropout_mult(seed, tr.STREAMS['mid0'] + layer, (B, T, J * D), p)) if p > 0 else None
    return v, params, drop, rng


# ---------------------------------------------------------------- range entry points
RANGE_B, RANGE_T = 3, 13
RANGE_WIDTHS = [(16, 16), (8, 16)]          # (J, D): n = 256 wave kernel, n = 128 block kernel
RANGES = [(2, 9), (0, 13), (4, 4)]          # the last is empty
RANGE_N_ITEMS = [(2, 9, 1), (5, 7, 3)]      # (t0, t1, layer): the grid is sized by the first
RANGE_P, RANGE_SEED = 0.1, 11
SENTINEL = 12345.0
