"""CPU side of tests/test_cnnfe_wgrad_gpu.py: the cases, their inputs, and the float64 /
float32 restatements (tests/torch_ref.cnnfe) of the stage-2 kernel gradients.

The launcher arithmetic of conv2_wgrad_rows_kernel is restated here (RANGES row ranges
of ceil(B T2 / RANGES) output rows; the kernel serves F2 <= 32) so that the cases can
assert which of them put an utterance boundary inside one workgroup's rows, leave
workgroups without rows, or fall to conv2_wgrad32_kernel."""
import functools

import numpy as np
import torch

from tests import torch_ref as tr

RANGES = 256          # kWrRanges
ROWS_MAX_F2 = 32      # wgrad_by_rows: F2 <= 32

# name -> (B, T, lengths, dropout, feat_dim, data seed)
CASES = {
    # several short utterances: the ring restarts at every utterance start (one row per workgroup)
    'short_utts': (5, 13, [13, 9, 4, 1, 13], 0.0, 123, 1),
    # 301 rows in ranges of 2: ranges span utterance boundaries (T2 = 7), the last one
    # holds a single row, 105 workgroup pairs have none; pt2 = 1; masked rows; dropout
    'span_boundary': (43, 26, [26, 26, 19, 7, 1, 22, 26, 13, 2, 26, 25, 24, 3] * 3 + [26, 11, 5, 26], 0.2, 123, 2),
    # pt2 = 1 (T1 = 19) and pt2 = 0 (T1 = 20), masked rows inside the tile, nonzero BN1 shift
    'pt2_1': (3, 37, [37, 30, 21], 0.0, 123, 3),
    'pt2_0_drop': (2, 40, [40, 33], 0.2, 123, 4),
    # fewer rows than ranges
    'one_row': (1, 1, [1], 0.0, 123, 5),
    'three_rows': (2, 6, [6, 1], 0.2, 123, 6),
    # F1 = 21 odd (pf2 = 1), F2 = 11: one k-step of a row is all padding
    'feat41': (3, 21, [21, 14, 5], 0.2, 41, 7),
    # ranges of 3 rows (750 rows): the ring goes round inside a workgroup and across boundaries (T2 = 25)
    'feat41_rows3': (30, 100, [100, 100, 77, 51, 18, 3, 100, 64, 99, 42] * 3, 0.0, 41, 8),
    # F2 = 33: the other side of the predicate (gab_split_t + conv2_wgrad32_kernel)
    'feat129_old_path': (2, 10, [10, 7], 0.0, 129, 9),
    # the same path with P2 = 64 rows x 33 = 2,112 a multiple of 64: the planes of g_ab have no padding, the last
    # pixel of the last plane is the last element of their workspace region and gmax / wdsc follow it directly
    'feat129_full_planes': (4, 64, [64, 64, 50, 64], 0.0, 129, 10),
}

PLANE_PX = 64         # kTpPx: the g_ab planes are padded to a multiple of it

DROP_SEED = 77


def dims(T, feat_dim):
    T1, F1 = -(-T // 2), -(-feat_dim // 2)
    return T1, F1, -(-T1 // 2), -(-F1 // 2)


def by_rows(feat_dim):
    return dims(1, feat_dim)[3] <= ROWS_MAX_F2


def row_ranges(B, T):
    """[(first row, end row)] of the RANGES workgroup pairs over the B T2 output rows."""
    T2 = dims(T, 1)[2]
    R = B * T2
    per = -(-R // RANGES)
    return [(min(R, k * per), min(R, k * per + per)) for k in range(RANGES)], T2


def spans_boundary(B, T):
    rr, T2 = row_ranges(B, T)
    return any(e > b and b // T2 != (e - 1) // T2 for b, e in rr)


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    P = {}
    cin = 1
    for k in range(2):
        for ab in 'ab':
            lim = (6.0 / (9 * cin + 9 * 64)) ** 0.5
            P[f'conv{k}{ab}_kernel'] = (torch.rand(3, 3, cin, 64, generator=g, dtype=torch.float64) * 2 - 1) * lim
            P[f'conv{k}{ab}_bias'] = 0.05 * torch.randn(64, generator=g, dtype=torch.float64)
        P[f'bn{k}_gamma'] = 1 + 0.1 * torch.randn(64, generator=g, dtype=torch.float64)
        P[f'bn{k}_beta'] = 0.3 * torch.randn(64, generator=g, dtype=torch.float64)   # BN1 shift well off zero
        cin = 64
    return {k: v.float().double() for k, v in P.items()}   # what both sides compute with


def _branches(feats, inp_len, P, drop):
    """Maxout choice (branch a >= branch b) of both stages, restating tests/torch_ref.cnnfe."""
    x = feats.unsqueeze(-1)
    sel = []
    for k in range(2):
        x1 = tr.conv2d_same(x, P[f'conv{k}a_kernel'], P[f'conv{k}a_bias'], 2)
        x2 = tr.conv2d_same(x, P[f'conv{k}b_kernel'], P[f'conv{k}b_bias'], 2)
        if drop is not None:
            x1 = x1 * drop[f'conv{k}a']
            x2 = x2 * drop[f'conv{k}b']
        sel.append(x1 >= x2)
        x = torch.maximum(x1, x2)
        m = tr.time_mask(inp_len, 2 ** (k + 1), x.shape[1], x.dtype)[:, :, None, None]
        x = x * m
        mu = x.mean(dim=(0, 1, 2))
        var = x.var(dim=(0, 1, 2), unbiased=False)
        x = ((x - mu) * torch.rsqrt(var + 1e-3) * P[f'bn{k}_gamma'] + P[f'bn{k}_beta']) * m
    return sel


@functools.lru_cache(maxsize=None)
def reference(name):
    """Inputs, the float64 and float32 stage-2 kernel gradients of sum(out * gout), and the
    number of positions at which the two precisions take different maxout branches."""
    B, T, lens, p, feat_dim, seed = CASES[name]
    assert len(lens) == B and max(lens) <= T
    T1, F1, T2, F2 = dims(T, feat_dim)
    P = _params(100 + seed)
    rng = np.random.default_rng(seed)
    feats = rng.standard_normal((B, T, feat_dim)).astype(np.float32).astype(np.float64)
    for b, l in enumerate(lens):
        feats[b, l:] = 0
    gout = torch.tensor(rng.standard_normal((B, T2, F2, 64)).astype(np.float32).astype(np.float64))
    inp_len = torch.tensor(np.array(lens, dtype=np.int32))
    drop = None
    if p > 0:
        drop = {}
        for k, (Tk, Fk) in enumerate(((T1, F1), (T2, F2))):
            ma, mb = tr.dropout_mult_pair(DROP_SEED, tr.STREAMS[f'conv{k}a'], (B, Tk, Fk, 64), p)
            drop[f'conv{k}a'] = torch.tensor(ma)
            drop[f'conv{k}b'] = torch.tensor(mb)
    grads = {}
    for dt in (torch.float64, torch.float32):
        Pd = {k: v.to(dt).clone().requires_grad_() for k, v in P.items()}
        dd = None if drop is None else {k: v.to(dt) for k, v in drop.items()}
        out = tr.cnnfe(torch.tensor(feats, dtype=dt), inp_len, Pd, dd)
        assert tuple(out.shape) == (B, T2, F2, 64)
        (out * gout.to(dt)).sum().backward()
        grads[dt] = {k: Pd[k].grad.double().numpy() for k in ('conv1a_kernel', 'conv1b_kernel')}
    with torch.no_grad():
        s64 = _branches(torch.tensor(feats), inp_len, P, drop)
        s32 = _branches(torch.tensor(feats, dtype=torch.float32), inp_len, {k: v.float() for k, v in P.items()},
                        None if drop is None else {k: v.float() for k, v in drop.items()})
    flips = sum(int((a != b).sum()) for a, b in zip(s64, s32))
    return dict(B=B, T=T, lens=lens, p=p, feat_dim=feat_dim, P=P, feats=feats, inp_len=inp_len, gout=gout,
                g64=grads[torch.float64], g32=grads[torch.float32], flips=flips)
