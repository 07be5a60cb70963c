#!/usr/bin/env python
"""Time of the CTC forced alignment on one GPU (ctc.forced_align, srf_ctc_align) next to
its yardstick, the CTC loss's forward-only launch (ops.ctc_loss without a gradient) at the
same shape in the same run, and the float64 host reference of tests/align_ref.py.
Shapes: T' = 200, L = 90, C = 32 and 63, B = 1 and 28; logits and labels by the recipe
of tests/align_ref.py's case list.  After --warmup calls of each, --windows windows per
entry point, alternating, each of --reps back-to-back calls between two device events
(so the queue stays full and a window measures the launches, not the host); the figures
are per call.  Next to the two Python entry points the same windows time the two C entry
points alone, on buffers allocated once (align_launch_us, loss_fwd_launch_us).  One JSON
line per configuration; no gate.

    python scripts/bench_align.py [--batch 1 28] [--classes 32 63] [--frames 200] [--labels 90]
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
    ap.add_argument('--classes', nargs='+', type=int, default=[32, 63])
    ap.add_argument('--frames', type=int, default=200)
    ap.add_argument('--labels', type=int, default=90)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--windows', type=int, default=10)
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_align.py needs a HIP device: times are measured, never estimated')
    from srf_amd import _lib, ctc, ops
    from tests import align_ref as ar
    dev = torch.device('cuda:0')
    T, L = args.frames, args.labels
    for C in args.classes:
        for B in args.batch:
            cases = [ar.case(b, T, C, L) for b in range(B)]
            x = torch.tensor(np.stack([c[0] for c in cases]), device=dev)
            labels = torch.tensor(np.array([c[1] for c in cases], dtype=np.int32), device=dev)
            lab_len = torch.full((B,), L, dtype=torch.int32, device=dev)
            lens = torch.full((B,), T, dtype=torch.int32, device=dev)
            blank = C - 1

            def align():
                return ctc.forced_align(x, lens, labels, lab_len, blank_index=blank)

            def loss():
                with torch.no_grad():
                    return ops.ctc_loss(x, labels, lab_len, lens, blank)

            # the two launches alone, on buffers allocated once (no Python wrapper between them)
            lib, p, st = _lib.lib(), ops._ptr, ops._stream()
            i32 = dict(dtype=torch.int32, device=dev)
            outs = [torch.empty((B, T), **i32), torch.empty((B, L), **i32), torch.empty((B, L), **i32),
                    torch.empty((B, L), device=dev), torch.empty(B, device=dev)]
            wa = lib.srf_ctc_align_workspace(B, T, C, L)
            wsa = torch.empty(wa, dtype=torch.uint8, device=dev)
            wl = lib.srf_ctc_workspace(B, T, C, L)
            wsl, nll_raw = torch.empty(wl, dtype=torch.uint8, device=dev), torch.empty(B, device=dev)

            def align_launch():
                _lib.check(lib.srf_ctc_align(p(x), p(labels), p(lab_len), p(lens), B, T, C, L, blank,
                                             *[p(o) for o in outs], p(wsa), wa, st), 'srf_ctc_align')

            def loss_launch():
                _lib.check(lib.srf_ctc_loss(p(x), p(labels), p(lab_len), p(lens), B, T, C, L, blank, 1.0, p(nll_raw),
                                            None, p(wsl), wl, st), 'srf_ctc_loss')

            for _ in range(args.warmup):
                for fn in (align, loss, align_launch, loss_launch):
                    fn()
            t_align, t_loss, k_align, k_loss = [], [], [], []
            for _ in range(args.windows):
                t_align.append(window(align, args.reps))
                t_loss.append(window(loss, args.reps))
                k_align.append(window(align_launch, args.reps))
                k_loss.append(window(loss_launch, args.reps))
            t0 = time.perf_counter()
            ref = [ar.viterbi(ar.log_softmax(c[0]), c[1], c[2]) for c in cases]
            host_ms = (time.perf_counter() - t0) * 1e3
            al = align()
            score, nll = al.score.cpu().numpy(), loss().cpu().numpy()
            states = al.states.cpu().tolist()
            print(json.dumps({'B': B, 'frames': T, 'classes': C, 'labels': L, 'windows': args.windows,
                              'reps': args.reps, 'align_us': stats(t_align), 'loss_fwd_us': stats(t_loss),
                              'align_launch_us': stats(k_align), 'loss_fwd_launch_us': stats(k_loss),
                              'host_ref_ms': round(host_ms, 2),
                              'paths_equal_reference': sum(states[b] == ref[b][0] for b in range(B)),
                              'score_below_loglik': bool(np.all(score <= -nll + 1e-3))}), flush=True)


if __name__ == '__main__':
    main()
