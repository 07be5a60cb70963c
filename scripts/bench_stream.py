#!/usr/bin/env python
"""Chunk latency of chunked streaming inference (srf_amd/streaming.py) on one GPU.

For the C3 (SDR) and C4 (DR) models (the shape kwargs of the c3_real / c4_real
fixtures), B = 1 and 8 streams and chunks of 32 and 64 input frames (10 ms each): one
warm-up session, then sessions of --chunks chunks until at least --min-chunks are timed.
Every chunk is timed with device events around push() on an idle device (the host
synchronises after each chunk, as a live stream leaves the device idle between chunks)
and with the host clock around push() plus fetching the chunk's labels.  Next to it: the
offline forward of one session's audio, divided by the session's chunks.  One JSON line
per configuration; no gate.

    python scripts/bench_stream.py [--models c3_real c4_real] [--batch 1 8] [--chunk 32 64] [--beam W]

--beam W adds the device beam search (StreamingRouter(beam_width=W)) to every timed chunk.
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

FRAME_MS = 10.0   # one input frame of audio


def timed_session(s, feats, chunk):
    """One session over feats [B, T, F]: per chunk (device ms, host ms with the labels
    fetched), and the device ms of finish()."""
    dev_ms, host_ms, evs = [], [], []
    for pos in range(0, feats.shape[1], chunk):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        x = feats[:, pos:pos + chunk]
        torch.cuda.synchronize()
        t = time.perf_counter()
        e0.record()
        out = s.push(x)
        e1.record()
        out.labels
        host_ms.append((time.perf_counter() - t) * 1e3)
        evs.append((e0, e1))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    s.finish().labels
    e1.record()
    torch.cuda.synchronize()
    dev_ms = [a.elapsed_time(b) for a, b in evs]
    return dev_ms, host_ms, e0.elapsed_time(e1)


def offline_ms(model, feats, reps):
    lens = torch.full((feats.shape[0],), feats.shape[1], dtype=torch.int32, device=feats.device)
    out = []
    with torch.no_grad():
        for i in range(reps + 1):   # the first run warms up
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            model(feats, input_lengths=lens, training=False)
            e1.record()
            torch.cuda.synchronize()
            if i:
                out.append(e0.elapsed_time(e1))
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--models', nargs='+', default=['c3_real', 'c4_real'])
    ap.add_argument('--batch', nargs='+', type=int, default=[1, 8])
    ap.add_argument('--chunk', nargs='+', type=int, default=[32, 64])
    ap.add_argument('--chunks', type=int, default=50, help='chunks per session')
    ap.add_argument('--min-chunks', type=int, default=200, help='timed chunks per configuration, at least')
    ap.add_argument('--offline-reps', type=int, default=3)
    ap.add_argument('--beam', type=int, default=None, metavar='W',
                    help='also push every chunk through the device beam search of width W (in the timed chunk)')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_stream.py needs a HIP device: chunk times are measured, never estimated')
    from srf_amd.sequence_router import SequenceRouter
    from srf_amd.streaming import StreamingRouter
    from tests.helpers import config_from_shape, load_eval_fixture
    dev = torch.device('cuda:0')
    for name in args.models:
        kw, sh = load_eval_fixture(name)[:2]
        model = SequenceRouter(config_from_shape(kw), None, sh.class_n, device=dev, seed=1)
        for B in args.batch:
            for chunk in args.chunk:
                T = chunk * args.chunks
                feats = torch.randn((B, T, sh.feat_dim), generator=torch.Generator().manual_seed(B * T)).to(dev)
                s = StreamingRouter(model, B, max_chunk=chunk, beam_width=args.beam)
                timed_session(s, feats, chunk)   # warm-up: every shape the timed sessions use
                dev_ms, host_ms, fin = [], [], []
                while len(dev_ms) < args.min_chunks:
                    s.reset()
                    d, h, f = timed_session(s, feats, chunk)
                    # the first chunks of a session emit nothing yet (lookahead): they are
                    # chunk times all the same and stay in
                    dev_ms += d
                    host_ms += h
                    fin.append(f)
                off = offline_ms(model, feats, args.offline_reps)
                audio = chunk * FRAME_MS
                row = {
                    'model': name, 'B': B, 'beam': args.beam, 'chunk_frames': chunk, 'chunk_audio_ms': audio,
                    'timed_chunks': len(dev_ms),
                    'chunk_ms_median': round(float(np.median(dev_ms)), 4),
                    'chunk_ms_p95': round(float(np.percentile(dev_ms, 95)), 4),
                    'chunk_host_ms_median': round(float(np.median(host_ms)), 4),
                    'chunk_host_ms_p95': round(float(np.percentile(host_ms, 95)), 4),
                    'finish_ms_median': round(float(np.median(fin)), 4),
                    'real_time_factor_median': round(float(np.median(dev_ms)) / audio, 5),
                    'real_time_factor_p95_host': round(float(np.percentile(host_ms, 95)) / audio, 5),
                    'offline_ms': round(off, 4), 'offline_ms_per_chunk': round(off / args.chunks, 4),
                    'lookahead_frames': s.lookahead,
                }
                print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
