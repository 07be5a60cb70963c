#!/usr/bin/env python
"""Time of the device word alignment on one GPU (srf_word_align, scoring.WordErrorRate)
next to its yardstick, the label alignment's launch (srf_edit_align) on the same label rows
measured in the same run.  Shapes: (H, R) = (90, 90) and (200, 200) labels, B = 1 and 28,
alphabet 30 with about 1 separator in 6 labels, 10 % random edits (the generator of
tests/words_ref.py).  After --warmup calls of each, --windows windows per entry point,
alternating, each of --reps back-to-back calls between two device events; the figures are
per call.  word_launch_us (both launches of srf_word_align, without the per-word tables
and maps, as WordErrorRate calls it), word_full_launch_us (with all of them) and
edit_launch_us time the C entry points alone on buffers allocated once, update_state_us
goes through WordErrorRate.update_state.  One JSON line per configuration; no gate.

    python scripts/bench_words.py [--batch 1 28] [--sizes 90 200]
"""
import argparse
import json
import os
import sys

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
    ap.add_argument('--alphabet', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--windows', type=int, default=10)
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_words.py needs a HIP device: times are measured, never estimated')
    from srf_amd import _lib, ops, scoring
    from tests import score_ref as sr
    from tests import words_ref as wr
    dev = torch.device('cuda:0')
    lib, p, st = _lib.lib(), ops._ptr, ops._stream()
    i32 = dict(dtype=torch.int32, device=dev)
    A = args.alphabet
    sep = wr.separator(A)
    for B in args.batch:
        for n in args.sizes:
            cases = [sr.case(b, n, n, 6 * A) for b in range(B)]
            hyp = torch.tensor(np.stack([wr.with_separators(c[0], A) for c in cases]), **i32)
            ref = torch.tensor(np.stack([wr.with_separators(c[1], A) for c in cases]), **i32)
            hyp_len, ref_len = torch.full((B,), n, **i32), torch.full((B,), n, **i32)
            W = (n + 1) // 2
            counts, wcounts = torch.empty((B, 6), **i32), torch.empty((B, 6), **i32)
            h2r, r2h = torch.empty((B, n), **i32), torch.empty((B, n), **i32)
            tables = [torch.empty((B, W), **i32) for _ in range(8)]
            totals = torch.zeros(8, dtype=torch.int64, device=dev)
            wtotals = torch.zeros(8, dtype=torch.int64, device=dev)
            we = lib.srf_edit_align_workspace(B, n, n)
            wse = torch.empty(we, dtype=torch.uint8, device=dev)
            ww = lib.srf_word_align_workspace(B, n, n)
            wsw = torch.empty(ww, dtype=torch.uint8, device=dev)
            wer = scoring.WordErrorRate(sep, device=dev)

            def edit_launch():
                _lib.check(lib.srf_edit_align(p(hyp), p(hyp_len), n, p(ref), p(ref_len), n, B, None, 0, p(counts),
                                              p(h2r), p(r2h), p(totals), None, 0, p(wse), we, st), 'srf_edit_align')

            def word_launch():
                _lib.check(lib.srf_word_align(p(hyp), p(hyp_len), n, p(ref), p(ref_len), n, B, None, 0, sep,
                                              p(wcounts), *[None] * 8, p(wtotals), p(wsw), ww, st), 'srf_word_align')

            def word_full_launch():
                _lib.check(lib.srf_word_align(p(hyp), p(hyp_len), n, p(ref), p(ref_len), n, B, None, 0, sep,
                                              p(wcounts), *[p(t) for t in tables], p(wtotals), p(wsw), ww, st),
                           'srf_word_align')

            def update_state():
                wer.update_state(hyp, hyp_len, ref, ref_len)

            fns = (word_launch, word_full_launch, edit_launch, update_state)
            for _ in range(args.warmup):
                for fn in fns:
                    fn()
            times = [[] for _ in fns]
            for _ in range(args.windows):
                for t, fn in zip(times, fns):
                    t.append(window(fn, args.reps))
            want = wr.align_batch(hyp.cpu().tolist(), [n] * B, ref.cpu().tolist(), [n] * B, sep)
            wtotals.zero_()
            word_full_launch()
            got = wcounts.cpu().tolist()
            maps = tables[6].cpu().tolist()
            print(json.dumps({'B': B, 'H': n, 'R': n, 'alphabet': A, 'windows': args.windows, 'reps': args.reps,
                              'word_launch_us': stats(times[0]), 'word_full_launch_us': stats(times[1]),
                              'edit_launch_us': stats(times[2]), 'update_state_us': stats(times[3]),
                              'reference_words': [w['counts'][4] for w in want][:4],
                              'counts_equal_reference': sum(got[b] == want[b]['counts'] for b in range(B)),
                              'maps_equal_reference': sum(maps[b] == want[b]['hyp_to_ref'] for b in range(B)),
                              'totals_equal_reference': wtotals.cpu().tolist() == wr.totals(want)}), flush=True)


if __name__ == '__main__':
    main()
