"""The gW pass of the DR backward on split fp16 (route_gw16s_kernel; din = dout = 32,
2 or 3 iterations) at the shapes where its staging of the per-frame vectors (gs^r, Vc^r)
can go wrong: 16-byte loads along the rows, transposed through an LDS image that the
waves of one output capsule share.

Cases (B, T, N, D, lpad, rpad, J, iters, mask_first), with the plan gw2_plan gives each
(F = B T frames in 16-frame tiles, S frame splits of ft_per tiles, n_rt groups of four
output capsules, n_cc groups of four input capsules; a workgroup takes two of those):

  0  F = 9: one partial tile, zero fill past F.  S = 1, ft_per = 1; n_rt 2, n_cc 3.
  1  F = 34: three tiles, each a split of its own, the last with 2 frames; J = 6 is no
     multiple of 4 (a clamped idle wave); masked first capsule; n_cc = 3 is odd (the last
     workgroup has an idle half).  S = 3, ft_per = 1; n_rt 2.
  2  F = 48: whole tiles; in_n = 9, a last capsule group of one.  S = 3, ft_per = 1;
     n_rt 1, n_cc 3.
  3  R = 2: three vectors per image; an odd tile count for the two-tile unroll.
     S = 1, ft_per = 3; n_rt 2, n_cc 8.
  4  F = 183: several tiles per frame split, the last tile partial.  S = 2, ft_per = 6;
     n_rt 3, n_cc 10.
  5  J dout = 1024, the layer-6 row range.  S = 1, ft_per = 2; n_rt 8, n_cc 2.

Reference: float64 autograd of oracle.naive_mirror under a standard normal upstream
gradient, as test_route_dr_gxw_split_gpu.  Every element of g_W and g_bias is compared.
Conditions per case:
  (a) two runs of the same backward give bit-identical g_W and g_bias (the gW path has no
      atomics, so a missing wait or barrier in the staging shows here);
  (b) max|err| <= 1e-4 * max(1, max|ref|), and
      max|err| / max|ref| <= 4 * PARENT[case], with 4e-7 where the parent was below 1e-7.
PARENT holds max|err| / max|ref| of commit 7f79369 (4-byte loads of the vectors per lane)
on the same inputs, measured once on an MI355X with this file.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import naive_mirror as nm
from tests.test_route_dr_gpu import _mk, _run_gpu

pytestmark = pytest.mark.gpu

CASES = [
    # B, T, N, D, lpad, rpad, J, iters, mask_first
    (1, 9, 4, 32, 1, 1, 8, 3, False),
    (2, 17, 4, 32, 1, 1, 6, 3, True),
    (2, 24, 3, 32, 1, 1, 4, 3, False),
    (1, 35, 8, 32, 1, 2, 8, 2, True),
    (3, 61, 8, 32, 2, 2, 12, 3, False),
    (1, 20, 2, 32, 1, 1, 32, 3, False),
]
GRADS = ('g_W', 'g_bias')

# max|err| / max|ref| of the parent commit 7f79369: {case index: (g_W, g_bias)}
PARENT = {
    0: (2.719e-07, 1.344e-07),
    1: (2.672e-07, 1.332e-07),
    2: (2.840e-07, 2.166e-07),
    3: (2.718e-07, 1.920e-07),
    4: (2.854e-07, 1.990e-07),
    5: (2.785e-07, 1.881e-07),
}


@functools.lru_cache(maxsize=None)
def _reference(ci):
    """The case's inputs, the upstream gradient and the float64 g_W, g_bias."""
    case = CASES[ci]
    B, T, N, D, lp, rp, J, it, mf = case
    emb, W, bias = _mk(case, 2)
    ce, cW, cb = (torch.tensor(a, requires_grad=True) for a in (emb, W, bias))
    ep = torch.nn.functional.pad(ce, (0, 0, 0, 0, lp, rp))
    xw = torch.cat([ep[:, w:w + T] for w in range(lp + rp + 1)], dim=2)
    vr = nm.dynamic_routing(nm.pose_tiled(xw, cW, cb), it, mf)
    gv = np.random.default_rng(3).standard_normal(vr.shape)
    refs = [r.numpy() for r in torch.autograd.grad(vr, (cW, cb), torch.tensor(gv))]
    return emb, W, bias, gv, refs


def backward(ci, dev):
    """g_W and g_bias of one forward and backward on the device, as numpy arrays."""
    emb, W, bias, gv, _ = _reference(ci)
    _, tW, tb, v = _run_gpu(CASES[ci], emb, W, bias, dev)
    v.backward(torch.tensor(gv, dtype=torch.float32, device=dev))
    return tW.grad.cpu().numpy(), tb.grad.cpu().numpy()


@pytest.mark.parametrize('ci', range(len(CASES)))
def test_route_dr_gw_stage(cuda, ci):
    refs = _reference(ci)[4]
    first, second = backward(ci, cuda), backward(ci, cuda)
    res = []
    for name, got, ref in zip(GRADS, first, refs):
        err, mref = float(np.abs(got.astype(np.float64) - ref).max()), float(np.abs(ref).max())
        res.append((err, mref))
        print(f'{CASES[ci]} {name}: max|err| {err:.3e} max|ref| {mref:.3e} rel {err / mref:.3e} '
              f'parent {PARENT[ci][len(res) - 1]:.3e}')
    for name, a, b in zip(GRADS, first, second):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f'{name} differs between two runs'
    for name, (err, mref), par in zip(GRADS, res, PARENT[ci]):
        assert err <= 1e-4 * max(1.0, mref), (name, err, mref)
        lim = 4.0 * par if par >= 1e-7 else 4e-7
        assert err / mref <= lim, (name, err / mref, par)
