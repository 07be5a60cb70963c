#!/usr/bin/env python
"""Decode time of the CTC beam search on one GPU: the host decoder on device logits
(ctc.beam_search_decode, copy of the logits included) against the device decoder
(ctc.beam_search_decode_device), at the decode shape T' = 200, C = 63, beam 100 for
B = 1 and 28.  Random logits of scale 3 (the recipe of tests/beam_ref.py's case list).
Per configuration: --warmup calls, then --calls timed ones on the host clock, each from a synchronised idle device to
the hypotheses on the host; next to it the device time of the push launch alone (events).
One JSON line per configuration; no gate.

    python scripts/bench_beam.py [--batch 1 28] [--frames 200] [--classes 63] [--beam 100]
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


def case_logits(seed, T, C):
    return (np.random.default_rng(1000 + seed).standard_normal((T, C)) * 3).astype(np.float32)


def timed(fn, warmup, calls):
    out = []
    for i in range(warmup + calls):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append((time.perf_counter() - t) * 1e3)
    return np.array(out)


def stats(ms):
    return {'median': round(float(np.median(ms)), 4), 'min': round(float(ms.min()), 4),
            'max': round(float(ms.max()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', nargs='+', type=int, default=[1, 28])
    ap.add_argument('--frames', type=int, default=200)
    ap.add_argument('--classes', type=int, default=63)
    ap.add_argument('--beam', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--calls', type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_beam.py needs a HIP device: decode times are measured, never estimated')
    from srf_amd import ctc
    dev = torch.device('cuda:0')
    T, C, W = args.frames, args.classes, args.beam
    for B in args.batch:
        x = torch.tensor(np.stack([case_logits(b, T, C) for b in range(B)]), device=dev)
        lens = [T] * B
        host = timed(lambda: ctc.beam_search_decode(x, lens, C - 1, W), args.warmup, args.calls)
        device = timed(lambda: ctc.beam_search_decode_device(x, lens, C - 1, W), args.warmup, args.calls)
        state = ctc.BeamState(B, C, C - 1, W, T, dev)
        n_valid = torch.tensor(lens, device=dev, dtype=torch.int32)
        push = []
        for i in range(args.warmup + args.calls):
            state.reset()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            state.push(x, n_valid)
            e1.record()
            torch.cuda.synchronize()
            if i >= args.warmup:
                push.append(e0.elapsed_time(e1))
        push = np.array(push)
        same = ctc.beam_search_decode(x, lens, C - 1, W)[0] == ctc.beam_search_decode_device(x, lens, C - 1, W)[0]
        print(json.dumps({'B': B, 'frames': T, 'classes': C, 'beam': W, 'calls': args.calls,
                          'host_ms': stats(host), 'device_ms': stats(device), 'push_kernel_ms': stats(push),
                          'push_us_per_frame': round(float(np.median(push)) * 1e3 / T, 3),
                          'same_labellings': same}), flush=True)


if __name__ == '__main__':
    main()
