#!/usr/bin/env python
"""Time of the waveform front end on one GPU (srf_amd/fbank.py, csrc/fbank.hip).

Offline: ``Fbank`` on --batch utterances of --seconds of 16 kHz int16 audio (28 x 8 s by
default), the Python entry point and its two launches alone on buffers allocated once.
Streaming: one ``FbankStream.push`` of 64 frames' worth of samples (10 240) for 1 and 28
streams, next to its yardstick, one ``StreamingRouter.push`` of 64 feature frames at the
same number of streams (the C4 model by default), and the chunk's static and delta
launches alone.  Method of scripts/bench_align.py: after --warmup calls of each, --windows
windows per entry point, alternating, each of --reps back-to-back calls between two device
events (a streaming window is one session of --reps chunks after a reset); the figures
are per call.  One JSON line per configuration; no gate.

    python scripts/bench_fbank.py [--batch 28] [--seconds 8] [--streams 1 28] [--model c4_real]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

CHUNK_FRAMES = 64


def window(fn, reps, before=None):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if before is not None:
        before()
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


def rounds(entries, warmup, windows, reps):
    """entries: name -> (fn, before or None); alternating windows; name -> stats."""
    for fn, before in entries.values():
        if before is not None:
            before()
        for _ in range(warmup):
            fn()
    out = {k: [] for k in entries}
    for _ in range(windows):
        for k, (fn, before) in entries.items():
            out[k].append(window(fn, reps, before))
    return {k: stats(v) for k, v in out.items()}


def audio(B, n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((B, n), generator=g) * 3000.0).round().clamp(-32768, 32767).to(torch.int16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=28)
    ap.add_argument('--seconds', type=float, default=8.0)
    ap.add_argument('--streams', nargs='+', type=int, default=[1, 28])
    ap.add_argument('--model', default='c4_real')
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--windows', type=int, default=10)
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_fbank.py needs a HIP device: times are measured, never estimated')
    from srf_amd import fbank
    from srf_amd.sequence_router import SequenceRouter
    from srf_amd.streaming import StreamingRouter
    from tests.helpers import config_from_shape, load_eval_fixture
    dev = torch.device('cuda:0')
    cm = (np.zeros(fbank.N_FEAT, dtype=np.float32), np.ones(fbank.N_FEAT, dtype=np.float32))
    fe = fbank.Fbank(cmvn=cm, device=dev)

    # offline
    B, N = args.batch, int(args.seconds * 16000)
    x, n = audio(B, N, 1).to(dev), torch.full((B,), N, dtype=torch.int32, device=dev)
    T = fbank.n_frames(N)
    st = torch.empty((B, T, fbank.N_STATIC), device=dev)
    ft = torch.empty((B, T, fbank.N_FEAT), device=dev)
    nfr = torch.full((B,), T, dtype=torch.int32, device=dev)
    res = rounds({'fbank_us': (lambda: fe(x, n), None),
                  'static_launch_us': (lambda: fe._static(x, n, N, 0, N, 0, T, st, 0), None),
                  'deltas_launch_us': (lambda: fe._deltas(st, nfr, 0, T, 0, T, ft, 0), None)},
                 args.warmup, args.windows, args.reps)
    print(json.dumps({'mode': 'offline', 'B': B, 'seconds': args.seconds, 'frames': T, 'windows': args.windows,
                      'reps': args.reps, **res,
                      'audio_seconds_per_second': round(B * args.seconds / (res['fbank_us']['median'] * 1e-6))}),
          flush=True)

    # one streaming chunk next to the model's chunk step
    kw, sh = load_eval_fixture(args.model)[:2]
    model = SequenceRouter(config_from_shape(kw), None, sh.class_n, device=dev, seed=1)
    ns = CHUNK_FRAMES * fbank.FRAME_SHIFT
    for S in args.streams:
        chunk = audio(S, ns, 2 + S).to(dev)
        feats = torch.randn((S, CHUNK_FRAMES, sh.feat_dim), generator=torch.Generator().manual_seed(S)).to(dev)
        fs = fbank.FbankStream(fe, S, ns)
        router = StreamingRouter(model, S, max_chunk=CHUNK_FRAMES)
        buf = torch.zeros((S, ns + 399), device=dev)
        stb = torch.empty((S, CHUNK_FRAMES + 12, fbank.N_STATIC), device=dev)
        out = torch.empty((S, CHUNK_FRAMES, fbank.N_FEAT), device=dev)
        far = torch.full((S,), 1 << 30, dtype=torch.int32, device=dev)
        res = rounds({'fbank_chunk_us': (lambda: fs.push(chunk), fs.reset),
                      'model_chunk_us': (lambda: router.push(feats), router.reset),
                      'static_launch_us': (lambda: fe._static(buf, far, ns + 240, 0, ns + 240, 0, CHUNK_FRAMES,
                                                              stb, -4), None),
                      'deltas_launch_us': (lambda: fe._deltas(stb, far, -4, CHUNK_FRAMES + 4, 0, CHUNK_FRAMES, out,
                                                              0), None)},
                     args.warmup, args.windows, args.reps)
        frac = res['fbank_chunk_us']['median'] / res['model_chunk_us']['median']
        print(json.dumps({'mode': 'stream', 'streams': S, 'chunk_frames': CHUNK_FRAMES, 'chunk_samples': ns,
                          'model': args.model, 'windows': args.windows, 'reps': args.reps, **res,
                          'fbank_over_model_chunk': round(frac, 4)}), flush=True)


if __name__ == '__main__':
    main()
