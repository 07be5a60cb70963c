#!/usr/bin/env python
"""Time of the device edit alignment on one GPU (srf_edit_align, scoring.ErrorRate) next to
its yardstick, the CTC forced alignment's launch (srf_ctc_align at T' = 200, L = 90,
C = 63) measured in the same run, and the host route it replaces: the copy of the
hypotheses to the host plus the plain-Python alignment of tests/score_ref.py (context only).
Shapes: (H, R) = (90, 90) and (200, 200), B = 1 and 28, alphabet 62, 10 % random edits by
the generator of tests/score_ref.py.  After --warmup calls of each, --windows windows per
entry point, alternating, each of --reps back-to-back calls between two device events;
the figures are per call.  edit_launch_us and align_launch_us time the two C entry points
alone on buffers allocated once, update_state_us goes through ErrorRate.update_state.
One JSON line per configuration; no gate.

    python scripts/bench_score.py [--batch 1 28] [--sizes 90 200]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps   # microseconds per call


def stats(us):
    us = np.array(us)
    return {'median': round(float(np.median(us)), 2), 'min': round(float(us.min()), 2),
            'max': round(float(us.max()), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', nargs='+', type=int, default=[1, 28])
    ap.add_argument('--sizes', nargs='+', type=int, default=[90, 200])
    ap.add_argument('--alphabet', type=int, default=62)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--windows', type=int, default=10)
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_score.py needs a HIP device: times are measured, never estimated')
    from srf_amd import _lib, ops, scoring
    from tests import align_ref as ar
    from tests import score_ref as sr
    dev = torch.device('cuda:0')
    lib, p, st = _lib.lib(), ops._ptr, ops._stream()
    i32 = dict(dtype=torch.int32, device=dev)
    T, L, C = 200, 90, 63
    for B in args.batch:
        # the yardstick's operands, as scripts/bench_align.py builds them
        acases = [ar.case(b, T, C, L) for b in range(B)]
        x = torch.tensor(np.stack([c[0] for c in acases]), device=dev)
        alab = torch.tensor(np.array([c[1] for c in acases], dtype=np.int32), device=dev)
        alab_len, alens = torch.full((B,), L, **i32), torch.full((B,), T, **i32)
        aouts = [torch.empty((B, T), **i32), torch.empty((B, L), **i32), torch.empty((B, L), **i32),
                 torch.empty((B, L), device=dev), torch.empty(B, device=dev)]
        wa = lib.srf_ctc_align_workspace(B, T, C, L)
        wsa = torch.empty(wa, dtype=torch.uint8, device=dev)

        def align_launch():
            _lib.check(lib.srf_ctc_align(p(x), p(alab), p(alab_len), p(alens), B, T, C, L, C - 1,
                                         *[p(o) for o in aouts], p(wsa), wa, st), 'srf_ctc_align')

        for n in args.sizes:
            cases = [sr.case(b, n, n, args.alphabet) for b in range(B)]
            hyp = torch.tensor([c[0] for c in cases], **i32)
            ref = torch.tensor([c[1] for c in cases], **i32)
            hyp_len, ref_len = torch.full((B,), n, **i32), torch.full((B,), n, **i32)
            counts, h2r, r2h = torch.empty((B, 6), **i32), torch.empty((B, n), **i32), torch.empty((B, n), **i32)
            totals = torch.zeros(8, dtype=torch.int64, device=dev)
            we = lib.srf_edit_align_workspace(B, n, n)
            wse = torch.empty(we, dtype=torch.uint8, device=dev)
            er = scoring.ErrorRate(device=dev)

            def edit_launch():
                _lib.check(lib.srf_edit_align(p(hyp), p(hyp_len), n, p(ref), p(ref_len), n, B, None, 0, p(counts),
                                              p(h2r), p(r2h), p(totals), None, 0, p(wse), we, st), 'srf_edit_align')

            def update_state():
                er.update_state(hyp, hyp_len, ref, ref_len)

            for _ in range(args.warmup):
                for fn in (edit_launch, align_launch, update_state):
                    fn()
            k_edit, k_align, t_update = [], [], []
            for _ in range(args.windows):
                k_edit.append(window(edit_launch, args.reps))
                k_align.append(window(align_launch, args.reps))
                t_update.append(window(update_state, args.reps))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host_h, host_r = hyp.cpu().tolist(), ref.cpu().tolist()
            want = [sr.align(h, r) for h, r in zip(host_h, host_r)]
            host_ms = (time.perf_counter() - t0) * 1e3
            totals.zero_()
            edit_launch()
            got = counts.cpu().tolist()
            print(json.dumps({'B': B, 'H': n, 'R': n, 'alphabet': args.alphabet, 'windows': args.windows,
                              'reps': args.reps, 'edit_launch_us': stats(k_edit), 'update_state_us': stats(t_update),
                              'align_launch_us': stats(k_align), 'align_shape': [T, L, C],
                              'host_route_ms': round(host_ms, 2),
                              'counts_equal_reference': sum(got[b] == want[b]['counts'] for b in range(B)),
                              'maps_equal_reference': sum(h2r[b].cpu().tolist() == want[b]['hyp_to_ref']
                                                          for b in range(B)),
                              'totals_equal_reference': totals.cpu().tolist() == sr.totals(want)}), flush=True)


if __name__ == '__main__':
    main()
