"""The capsule glue kernels (srf_amd/csrc/caps.hip) and the column sum
(srf_amd/csrc/reduce.hip) on every row-count path; tests/test_caps_gpu.py holds the
small-shape cases.  Shapes, seeds and inputs come from tests/caps_cases.py, whose
preconditions tests/test_caps_cases_cpu.py checks without a GPU.

srf::colsum, called through srf_capsnorm_bwd_params (colsum(gpart, F, 2n) scattered
into two outputs of width n), at the smallest shape of each route and edge:
  rows <= 128                                     one pass of colsum_stage2
  rows <= 4096 or cblocks >= 128, cblocks < 64    colsum_one<16>
  rows <= 4096 or cblocks >= 128, cblocks >= 64   colsum_one<64>
  otherwise                                       colsum_stage1 + colsum_stage2
Integer inputs must sum bit-exactly (a dropped, doubled or misplaced row or column);
float inputs within rows 2^-24 sum|in| per column, the worst case of any fp32
summation order, and bit-identically on a second call.

Primary capsules (float64 autograd reference and tolerances of test_primary_caps;
values elementwise): F = 4100 and F = 2100 (several wgrad batches per chunk with a
partial last one, a partial last g_X frame group, the two-stage and the colsum_one
column sum of wpart), and the generic projection kernels (PH = 12, PH = 24, K = 35)
and the MFMA forward with two live K-waves (K = 20).  No maxout pair of a case is
closer than 8 x the fp32 error of v1 - v2 (asserted again here).

capsnorm and head with more than 128 and more than 4096 partial rows, and the SDR
stack's range entry points (srf_capsnorm_{fwd,bwd}_range, _range_n) on their own:
rows inside a range against the reference, rows outside untouched bit for bit.

Tolerances: values |err| <= 1e-4 (1 + |ref|) per element; gradients
|err| <= 1e-3 max|ref| + 1e-6.  Each test prints its figures before it asserts."""
import numpy as np
import pytest
import torch

from tests import caps_cases as cc
from tests import torch_ref as tr

pytestmark = pytest.mark.gpu

SRF_EWORKSPACE = -4
GUARD = 64   # sentinel elements on each side of an output


def _params_call(x, rows, n, short=0):
    """srf_capsnorm_bwd_params on x [rows, 2n] (device): outputs as views into one
    sentinel-filled buffer, the workspace at exactly its size (less `short` bytes) plus
    a sentinel tail.  Returns rc, g_gamma, g_beta and whether every sentinel survived."""
    from srf_amd import _lib, ops
    L = _lib.lib()
    buf = torch.full((3 * GUARD + 2 * n,), cc.SENTINEL, dtype=torch.float32, device=x.device)
    g_gamma, g_beta = buf[GUARD:GUARD + n], buf[2 * GUARD + n:2 * GUARD + 2 * n]
    wb = L.srf_capsnorm_params_workspace(rows, n)
    ws = torch.full((wb + 256,), 0xA5, dtype=torch.uint8, device=x.device)
    rc = L.srf_capsnorm_bwd_params(ops._ptr(x), rows, n, ops._ptr(g_gamma), ops._ptr(g_beta), ops._ptr(ws),
                                   wb - short, ops._stream())
    torch.cuda.synchronize()
    guards = torch.cat([buf[:GUARD], buf[GUARD + n:2 * GUARD + n], buf[2 * GUARD + 2 * n:]])
    intact = bool(torch.all(guards == cc.SENTINEL)) and bool(torch.all(ws[wb:] == 0xA5))
    return rc, g_gamma.cpu().numpy(), g_beta.cpu().numpy(), intact


@pytest.mark.parametrize('route,rows,n,slices,last', cc.COLSUM_CASES, ids=cc.colsum_ids())
def test_colsum_exact(cuda, route, rows, n, slices, last):
    """Integers in [-64, 64]: every partial sum is an integer below 2^24, so the fp32
    sums equal the int64 ones in any order."""
    x = cc.colsum_exact_input(rows, n)
    want = x.astype(np.int64).sum(0)
    rc, gg, gb, intact = _params_call(torch.tensor(x, device=cuda), rows, n)
    assert rc == 0
    got = np.concatenate([gg, gb])
    bad = np.nonzero(got != want.astype(np.float32))[0]
    print(f'{route} {rows} x {2 * n}: {bad.size} of {2 * n} columns differ')
    assert bad.size == 0, (bad[:8], got[bad[:8]], want[bad[:8]])
    assert intact, 'a guard element or the workspace tail was written'


@pytest.mark.parametrize('route,rows,n,slices,last', cc.COLSUM_CASES, ids=cc.colsum_ids())
def test_colsum_float(cuda, route, rows, n, slices, last):
    """Standard normal times 10^U(-3, 3) per column: per column within
    rows 2^-24 sum_r |in[r][c]| of the float64 sum, and the same bits on a second call."""
    x = cc.colsum_float_input(rows, n)
    want = np.add.reduce(x, axis=0, dtype=np.float64)
    bound = rows * 2.0 ** -24 * np.add.reduce(np.abs(x), axis=0, dtype=np.float64)
    xd = torch.tensor(x, device=cuda)
    rc, gg, gb, intact = _params_call(xd, rows, n)
    assert rc == 0
    got = np.concatenate([gg, gb])
    err = np.abs(got.astype(np.float64) - want)
    print(f'{route} {rows} x {2 * n}: worst column at {np.max(err / bound):.4f} of its bound')
    assert np.all(err <= bound), (int(np.argmax(err / bound)), np.max(err / bound))
    assert intact, 'a guard element or the workspace tail was written'
    rc2, gg2, gb2, _ = _params_call(xd, rows, n)
    assert rc2 == 0 and np.array_equal(gg, gg2) and np.array_equal(gb, gb2), 'two calls differ'


@pytest.mark.parametrize('route,rows,n,slices,last', cc.COLSUM_CASES, ids=cc.colsum_ids())
def test_colsum_workspace_one_byte_short(cuda, route, rows, n, slices, last):
    """A host-side check: SRF_EWORKSPACE, and nothing is launched."""
    rc, gg, gb, intact = _params_call(torch.zeros((rows, 2 * n), device=cuda), rows, n, short=1)
    assert rc == SRF_EWORKSPACE
    assert np.all(gg == cc.SENTINEL) and np.all(gb == cc.SENTINEL) and intact


def _elementwise(name, got, ref):
    g, r = got.detach().cpu().double().numpy(), ref.detach().cpu().double().numpy()
    assert g.shape == r.shape, (name, g.shape, r.shape)
    if g.size == 0:
        return
    q = np.abs(g - r) / (1e-4 * (1 + np.abs(r)))
    print(f'{name}: max err {np.abs(g - r).max():.3e}, worst element at {q.max():.4f} of its tolerance')
    assert np.all(q <= 1), (name, q.max())


def _grad_close(name, got, want):
    g, w = got.detach().cpu().double(), want.detach().cpu().double()
    assert g.shape == w.shape, (name, g.shape, w.shape)
    if g.numel() == 0:
        return
    e, m = (g - w).abs().max().item(), w.abs().max().item()
    print(f'grad {name}: max err {e:.3e}, max|ref| {m:.3e}, at {e / (1e-3 * m + 1e-6):.4f} of its tolerance')
    assert e <= 1e-3 * m + 1e-6, (name, e, m)


@pytest.mark.parametrize('name', list(cc.PRIMARY_CASES))
def test_primary_caps_rows(cuda, name):
    from srf_amd import ops
    c, X, inp_len, P, drop, gz = cc.primary_inputs(name)
    gap, err = cc.maxout_gap(X, inp_len, P, drop)
    print(f'{name}: smallest |v1 - v2| {gap:.3e}, float32 error {err:.3e}')
    assert gap >= cc.MAXOUT_MARGIN * err, (gap, err)
    PH, PD, p = c['PH'], c['PD'], c['p']
    Pr = {k: v.clone().requires_grad_() for k, v in P.items()}
    Xr = torch.tensor(X, requires_grad=True)
    ref = tr.primary_caps(Xr, torch.tensor(inp_len), Pr, PH, PD, drop)
    (ref * torch.tensor(gz)).sum().backward()
    Pg = {k: v.float().to(cuda).requires_grad_() for k, v in P.items()}
    Xg = torch.tensor(X, dtype=torch.float32, device=cuda, requires_grad=True)
    z = ops.primary_caps(Xg, torch.tensor(inp_len, device=cuda), PH, PD, True, 0.2 if p > 0 else 0.0, p,
                         cc.PRIMARY_DROP_SEED, [Pg[k] for k in ops.CAPS_PARAMS])
    _elementwise('z', z, ref)
    (z * torch.tensor(gz, dtype=torch.float32, device=cuda)).sum().backward()
    for k, got, want in [('X', Xg.grad, Xr.grad)] + [(k, Pg[k].grad, Pr[k].grad) for k in ops.CAPS_PARAMS]:
        _grad_close(k, got, want)


@pytest.mark.parametrize('B,T,J,D,head,p', cc.CAPSNORM_CASES)
def test_capsnorm_and_head_rows(cuda, B, T, J, D, head, p):
    from srf_amd import ops
    v, params, drop, rng = cc.capsnorm_inputs(B, T, J, D, p)
    ts = [torch.tensor(v, requires_grad=True)] + [t.clone().requires_grad_() for t in params]
    tg = [t.detach().float().to(cuda).requires_grad_() for t in ts]
    if head:
        ref = tr.caps_head(*ts, drop)
        out = ops.CapsHead.apply(*tg, True, p, cc.CAPSNORM_SEED, cc.CAPSNORM_LAYER)
    else:
        ref = tr.capsnorm(ts[0], ts[1], ts[2], drop)
        out = ops.CapsNorm.apply(tg[0], tg[1], tg[2], True, p, cc.CAPSNORM_SEED, cc.CAPSNORM_LAYER)
    _elementwise('out', out, ref)
    w = torch.tensor(rng.standard_normal(ref.shape).astype(np.float32))
    (ref * w.double()).sum().backward()
    (out * w.to(cuda)).sum().backward()
    for i in range(5 if head else 3):
        _grad_close(('v', 'gamma_mid', 'beta_mid', 'gamma_out', 'beta_out')[i], tg[i].grad, ts[i].grad)


# ---------------------------------------------------------------- range entry points
class _RangeItem:
    """One layer's inputs, float64 reference restricted to frames [t0, t1), and
    sentinel-filled device buffers."""

    def __init__(self, dev, J, D, t0, t1, layer, rng_seed):
        B, T, n = cc.RANGE_B, cc.RANGE_T, J * D
        self.t0, self.t1, self.layer, self.n = t0, t1, layer, n
        v, params, drop, rng = cc.capsnorm_inputs(B, T, J, D, cc.RANGE_P, cc.RANGE_SEED, layer, rng_seed)
        self.ts = [torch.tensor(v, requires_grad=True)] + [t.clone().requires_grad_() for t in params[:2]]
        self.ref = tr.capsnorm(*self.ts, drop).reshape(B, T, n)
        w = torch.tensor(rng.standard_normal((B, T, n)).astype(np.float32))
        inside = torch.zeros(B, T, 1, dtype=torch.float64)
        inside[:, t0:t1] = 1
        (self.ref * w.double() * inside).sum().backward()   # a loss over the in-range frames only
        self.x, self.gamma, self.beta = (t.detach().float().to(dev).contiguous() for t in self.ts)
        self.g_y = w.to(dev)   # whole: the rows outside the range must not be read into anything
        full = lambda *s: torch.full(s, cc.SENTINEL, dtype=torch.float32, device=dev)
        self.y, self.stat, self.g_x, self.gpart = full(B, T, n), full(B * T, 4), full(B, T, n), full(B * T, 2 * n)

    def struct(self):
        from srf_amd import _lib
        r = _lib.CapsnormRange()
        r.t0, r.t1, r.layer = self.t0, self.t1, self.layer
        for k in ('x', 'gamma', 'beta', 'y', 'stat', 'g_y', 'g_x', 'gpart'):
            setattr(r, k, getattr(self, k).data_ptr())
        return r

    def check_fwd(self):
        B, T = cc.RANGE_B, cc.RANGE_T
        t0, t1 = self.t0, self.t1
        y, stat = self.y.cpu(), self.stat.cpu().reshape(B, T, 4)
        _elementwise(f'y of layer {self.layer}', y[:, t0:t1], self.ref[:, t0:t1])
        x64 = self.ts[0].detach().reshape(B, T, self.n)
        _elementwise('mean', stat[:, t0:t1, 0], x64.mean(-1)[:, t0:t1])
        _elementwise('rstd', stat[:, t0:t1, 1], torch.rsqrt(x64.var(-1, unbiased=False) + 1e-3)[:, t0:t1])
        for name, t in (('y', y), ('stat', stat)):
            assert torch.all(t[:, :t0] == cc.SENTINEL) and torch.all(t[:, t1:] == cc.SENTINEL), \
                f'{name}: a row outside [{t0}, {t1}) was written'

    def check_bwd(self):
        from srf_amd import _lib, ops
        B, T, n = cc.RANGE_B, cc.RANGE_T, self.n
        t0, t1 = self.t0, self.t1
        g_x = self.g_x.cpu()
        _grad_close(f'x of layer {self.layer}', g_x[:, t0:t1], self.ts[0].grad.reshape(B, T, n)[:, t0:t1])
        gp = self.gpart.reshape(B, T, 2 * n)
        for name, t in (('g_x', g_x), ('gpart', gp.cpu())):
            assert torch.all(t[:, :t0] == cc.SENTINEL) and torch.all(t[:, t1:] == cc.SENTINEL), \
                f'{name}: a row outside [{t0}, {t1}) was written'
        # in-range partial rows sit at the frame's own index: zero the others and sum all F
        gp[:, :t0] = 0
        gp[:, t1:] = 0
        L = _lib.lib()
        wb = L.srf_capsnorm_params_workspace(B * T, n)
        ws = torch.empty(wb, dtype=torch.uint8, device=self.x.device)
        g_gamma, g_beta = torch.empty_like(self.gamma), torch.empty_like(self.beta)
        _lib.check(L.srf_capsnorm_bwd_params(ops._ptr(self.gpart), B * T, n, ops._ptr(g_gamma), ops._ptr(g_beta),
                                             ops._ptr(ws), wb, ops._stream()), 'srf_capsnorm_bwd_params')
        torch.cuda.synchronize()
        _grad_close('gamma', g_gamma, self.ts[1].grad)
        _grad_close('beta', g_beta, self.ts[2].grad)
        if t0 == t1:
            assert torch.count_nonzero(g_gamma) == 0 and torch.count_nonzero(g_beta) == 0


@pytest.mark.parametrize('t0,t1', cc.RANGES)
@pytest.mark.parametrize('J,D', cc.RANGE_WIDTHS, ids=['wave256', 'block128'])
def test_capsnorm_range(cuda, J, D, t0, t1):
    """srf_capsnorm_fwd_range / _bwd_range (RowMap{T, t0, t1 - t0}): rows of [t0, t1) of
    every utterance meet the reference, with the dropout mask of the frame's global
    element index; every other row of y, stat, g_x and gpart keeps its sentinel."""
    from srf_amd import _lib, ops
    L = _lib.lib()
    it = _RangeItem(cuda, J, D, t0, t1, 2, 3)
    B, T, n = cc.RANGE_B, cc.RANGE_T, it.n
    _lib.check(L.srf_capsnorm_fwd_range(ops._ptr(it.x), B, T, t0, t1, n, ops._ptr(it.gamma), ops._ptr(it.beta), 1,
                                        cc.RANGE_P, cc.RANGE_SEED, it.layer, ops._ptr(it.y), ops._ptr(it.stat),
                                        ops._stream()), 'srf_capsnorm_fwd_range')
    torch.cuda.synchronize()
    it.check_fwd()
    _lib.check(L.srf_capsnorm_bwd_range(ops._ptr(it.x), B, T, t0, t1, n, ops._ptr(it.gamma), ops._ptr(it.beta), 1,
                                        cc.RANGE_P, cc.RANGE_SEED, it.layer, ops._ptr(it.stat), ops._ptr(it.g_y),
                                        ops._ptr(it.g_x), ops._ptr(it.gpart), ops._stream()),
               'srf_capsnorm_bwd_range')
    torch.cuda.synchronize()
    it.check_bwd()


@pytest.mark.parametrize('with_empty', [False, True], ids=['two', 'empty-first'])
@pytest.mark.parametrize('J,D', cc.RANGE_WIDTHS, ids=['wave256', 'block128'])
def test_capsnorm_range_n(cuda, J, D, with_empty):
    """One srf_capsnorm_{fwd,bwd}_range_n call with two items: layers 1 and 3 (their own
    dropout streams), ranges [2, 9) and [5, 7) (the grid is sized by the first; the
    second's surplus workgroups return early), separate buffers.  With an empty range
    in front, the host drops it and the others move up."""
    from srf_amd import _lib, ops
    L = _lib.lib()
    B, T, n = cc.RANGE_B, cc.RANGE_T, J * D
    items = [_RangeItem(cuda, J, D, t0, t1, layer, 20 + layer) for t0, t1, layer in cc.RANGE_N_ITEMS]
    structs = [it.struct() for it in items]
    if with_empty:
        e = _lib.CapsnormRange()
        e.t0, e.t1, e.layer = 4, 4, 0   # no buffers: an empty range is dropped before they are looked at
        structs.insert(0, e)
    arr = (_lib.CapsnormRange * len(structs))(*structs)
    _lib.check(L.srf_capsnorm_fwd_range_n(arr, len(structs), B, T, n, 1, cc.RANGE_P, cc.RANGE_SEED, ops._stream()),
               'srf_capsnorm_fwd_range_n')
    torch.cuda.synchronize()
    for it in items:
        it.check_fwd()
    _lib.check(L.srf_capsnorm_bwd_range_n(arr, len(structs), B, T, n, 1, cc.RANGE_P, cc.RANGE_SEED, ops._stream()),
               'srf_capsnorm_bwd_range_n')
    torch.cuda.synchronize()
    for it in items:
        it.check_bwd()
