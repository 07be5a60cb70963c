"""The split-fp16 gx / gW passes of the DR backward (route_gux16_kernel,
route_gw16s_kernel; din = dout = 32) under upstream gradients that stress the
exponent of the fp16 hi / lo split.

The gx pass takes the exponent of a (capsule, frame) tile from a bound on max|gu| that
it knows before gu is formed (the triangle inequality over the five terms of gu), not
from the tile's own maximum, and the gW pass takes its per-layer exponent from the
maximum of those bounds.  The bound can sit up to log2 5 bits above the true maximum,
which may cost the split up to 2 bits; the inputs below are where that shows:

* ``normal``: standard normal gradient;
* ``skewed``: scaled by 2^u, u uniform in [-20, 4] per (utterance, frame, output
  capsule), so exponents inside one workgroup differ by 24 bits and one frame's bound
  must not leak into its neighbours;
* ``cancel``: minus the layer output plus 2^-10 noise on a third of the frames, where
  c^r gs^r and gL^r Vc^r nearly cancel and the bound is furthest above the maximum.

Reference: float64 autograd of oracle.naive_mirror, as test_route_dr_backward.
Conditions per case, input and gradient (all elements compared):
  max|err| <= 1e-4 * max(1, max|ref|), and
  max|err| / max|ref| <= 4 * PARENT[...], with 4e-7 where the parent was below 1e-7
  (there the float atomics of the gx flush dominate).
PARENT holds max|err| / max|ref| of commit 8bdb589 (the masking split with per-tile
maxima) on the same inputs, measured once on an MI355X.
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
    (1, 35, 8, 32, 1, 2, 8, 2, True),     # R = 2; a partial second frame tile; masked first capsule
    (2, 17, 4, 32, 1, 1, 6, 3, True),     # J no multiple of a workgroup's 4 capsules; utterance edges in a tile
    (3, 61, 8, 32, 2, 2, 12, 3, False),   # several output-capsule groups per workgroup; n-chunks
    (1, 9, 4, 32, 1, 1, 8, 4, False),     # R = 4: route_gux16_kernel<4>, the fp32 gW kernel behind it
]
KINDS = ('normal', 'skewed', 'cancel')
GRADS = ('g_emb', 'g_W', 'g_bias')

# max|err| / max|ref| of the parent commit 8bdb589: {(case index, kind): (g_emb, g_W, g_bias)}
PARENT = {
    (0, 'normal'): (2.291e-07, 2.718e-07, 1.790e-07),
    (0, 'skewed'): (2.324e-07, 3.680e-07, 2.344e-07),
    (0, 'cancel'): (2.212e-07, 3.342e-07, 1.877e-07),
    (1, 'normal'): (2.119e-07, 2.672e-07, 1.332e-07),
    (1, 'skewed'): (2.061e-07, 3.814e-07, 1.648e-07),
    (1, 'cancel'): (2.476e-07, 2.553e-07, 1.651e-07),
    (2, 'normal'): (2.978e-07, 2.854e-07, 1.867e-07),
    (2, 'skewed'): (2.299e-07, 3.068e-07, 2.284e-07),
    (2, 'cancel'): (2.647e-07, 3.110e-07, 2.029e-07),
    (3, 'normal'): (2.596e-07, 2.021e-07, 1.392e-07),
    (3, 'skewed'): (2.904e-07, 2.186e-07, 1.919e-07),
    (3, 'cancel'): (2.713e-07, 3.706e-07, 4.181e-07),
}


@functools.lru_cache(maxsize=None)
def _reference(ci):
    """The case's inputs, its float64 forward graph and the three upstream gradients."""
    case = CASES[ci]
    B, T, N, D, lp, rp, J, it, mf = case
    emb, W, bias = _mk(case, 2)
    ce, cW, cb = (torch.tensor(a, requires_grad=True) for a in (emb, W, bias))
    ep = torch.nn.functional.pad(ce, (0, 0, 0, 0, lp, rp))
    xw = torch.cat([ep[:, w:w + T] for w in range(lp + rp + 1)], dim=2)
    vr = nm.dynamic_routing(nm.pose_tiled(xw, cW, cb), it, mf)
    rng = np.random.default_rng(3)
    gvs = {'normal': rng.standard_normal(vr.shape)}
    gvs['skewed'] = rng.standard_normal(vr.shape) * np.exp2(rng.uniform(-20, 4, size=(B, T, J)))[..., None]
    g = rng.standard_normal(vr.shape)
    third = (np.arange(B * T).reshape(B, T) % 3) == 0
    g[third] = -vr.detach().numpy()[third] + 2.0 ** -10 * rng.standard_normal(vr.shape)[third]
    gvs['cancel'] = g
    refs = {}
    for kind, gv in gvs.items():
        gr = torch.autograd.grad(vr, (ce, cW, cb), torch.tensor(gv), retain_graph=True)
        refs[kind] = [r.numpy() for r in gr]
    return emb, W, bias, gvs, refs


def errors(ci, kind, dev):
    """(max|err|, max|ref|) of g_emb, g_W, g_bias for one case and upstream gradient."""
    emb, W, bias, gvs, refs = _reference(ci)
    te, tW, tb, v = _run_gpu(CASES[ci], emb, W, bias, dev)
    v.backward(torch.tensor(gvs[kind], dtype=torch.float32, device=dev))
    out = []
    for got, ref in zip((te.grad, tW.grad, tb.grad), refs[kind]):
        out.append((float(np.abs(got.cpu().double().numpy() - ref).max()), float(np.abs(ref).max())))
    return out


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('ci', range(len(CASES)))
def test_route_dr_gxw_split(cuda, ci, kind):
    res = errors(ci, kind, cuda)
    for name, (err, mref), par in zip(GRADS, res, PARENT[(ci, kind)]):
        print(f'{CASES[ci]} {kind} {name}: max|err| {err:.3e} max|ref| {mref:.3e} rel {err / mref:.3e} parent {par:.3e}')
    for name, (err, mref), par in zip(GRADS, res, PARENT[(ci, kind)]):
        assert err <= 1e-4 * max(1.0, mref), (name, err, mref)
        lim = 4.0 * par if par >= 1e-7 else 4e-7
        assert err / mref <= lim, (name, err / mref, par)
