#!/usr/bin/env python
"""What endpointing costs (srf_amd/endpoint.py) on one GPU.

1. The chunk step of StreamingRouter with a beam, with and without endpoint=, by the method
   of scripts/bench_stream.py: one warm-up session, then sessions of --chunks chunks until
   --min-chunks are timed, device events around push() on an idle device.
2. The launches an endpointer adds, each alone on a chunk's worth of logits [B, n, C]: the
   endpoint kernel, the cut kernel (with the copy of the frames after the cut), and a push of
   no frames, which is what the second push is for every stream without a cut.
3. endpoints() offline on [B, T, C] against the same flags written with torch ops plus the
   host loop over them.

One JSON line per configuration; no gate.

    python scripts/bench_endpoint.py [--model c3_real] [--batch 1 28] [--chunk 32] [--beam 100]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'scripts'))


def event_ms(fn, reps):
    """Median device ms of fn() over reps runs on an idle device, after one warm-up."""
    out = []
    for i in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if i:
            out.append(e0.elapsed_time(e1))
    return float(np.median(out))


def torch_endpoints(logits, lengths, blank, rules):
    """The rule with the flags from torch ops and the machine on the host."""
    lp_blank = torch.log_softmax(logits, dim=-1)[:, :, blank]
    flags = torch.stack([lp_blank > math.log(rules.blank_threshold), logits.argmax(dim=-1) != blank], dim=-1)
    flags = flags.cpu().tolist()
    out = []
    for b, rows in enumerate(flags):
        n = sil = t = 0
        speech, cuts = False, []
        for is_sil, is_sp in rows[:lengths[b]]:
            n += 1
            sil = sil + 1 if is_sil else 0
            speech = speech or is_sp
            reason = (2 if speech and sil >= rules.silence_after_speech else 1 if sil >= rules.silence_only
                      else 3 if n >= rules.max_segment else 0)
            if reason:
                cuts.append((t - n + 1, t, reason))
                n, sil, speech = 0, 0, False
            t += 1
        out.append(cuts)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--model', default='c3_real')
    ap.add_argument('--batch', nargs='+', type=int, default=[1, 28])
    ap.add_argument('--chunk', type=int, default=32)
    ap.add_argument('--chunks', type=int, default=200, help='chunks per session')
    ap.add_argument('--min-chunks', type=int, default=400, help='timed chunks per configuration, at least')
    ap.add_argument('--beam', type=int, default=100)
    ap.add_argument('--rules', nargs=4, type=float, default=[125, 25, 500, 0.8],
                    metavar=('SILENCE_ONLY', 'SILENCE_AFTER_SPEECH', 'MAX_SEGMENT', 'BLANK_THRESHOLD'))
    ap.add_argument('--offline-frames', type=int, default=200)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--skip-steps', action='store_true', help='parts 2 and 3 only')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_endpoint.py needs a HIP device: times are measured, never estimated')
    from bench_stream import timed_session
    from srf_amd import ctc, endpoint, ops
    from srf_amd.sequence_router import SequenceRouter
    from srf_amd.streaming import StreamingRouter
    from tests.helpers import config_from_shape, load_eval_fixture
    dev = torch.device('cuda:0')
    rules = endpoint.EndpointRules(int(args.rules[0]), int(args.rules[1]), int(args.rules[2]), args.rules[3])
    kw, sh = load_eval_fixture(args.model)[:2]
    model = SequenceRouter(config_from_shape(kw), None, sh.class_n, device=dev, seed=1)
    C, blank, chunk = sh.class_n, sh.class_n - 1, args.chunk
    for B in args.batch:
        T = chunk * args.chunks
        feats = torch.randn((B, T, sh.feat_dim), generator=torch.Generator().manual_seed(B * T)).to(dev)
        if not args.skip_steps:
            for ep in (None, rules, None, rules):   # interleaved: two runs of each
                s = StreamingRouter(model, B, max_chunk=chunk, beam_width=args.beam, endpoint=ep,
                                    max_frames=None if ep is None else rules.max_segment + 64)
                timed_session(s, feats, chunk)
                dev_ms, host_ms = [], []
                while len(dev_ms) < args.min_chunks:
                    s.reset()
                    d, h, _ = timed_session(s, feats, chunk)
                    dev_ms += d
                    host_ms += h
                row = {'what': 'chunk_step', 'model': args.model, 'B': B, 'beam': args.beam, 'chunk_frames': chunk,
                       'endpoint': ep is not None, 'timed_chunks': len(dev_ms),
                       'chunk_ms_median': round(float(np.median(dev_ms)), 4),
                       'chunk_ms_p95': round(float(np.percentile(dev_ms, 95)), 4),
                       'chunk_host_ms_median': round(float(np.median(host_ms)), 4)}
                if ep is not None:
                    row['segments'] = [len(sb) for sb in s.segments][:4]
                print(json.dumps(row), flush=True)
        # the launches an endpointer adds, alone
        n = chunk // 4
        g = torch.Generator().manual_seed(7)
        x = (torch.randn((B, n, C), generator=g) * 3).to(dev)
        nv = torch.full((B,), n, dtype=torch.int32, device=dev)
        none = torch.full((B,), -1, dtype=torch.int32, device=dev)
        zero = torch.zeros(B, dtype=torch.int32, device=dev)
        e = endpoint.Endpointer(rules, B, C, blank, dev)
        state = ctc.BeamState(B, C, blank, args.beam, rules.max_segment + 64, dev, segmented=True)
        row = {'what': 'launches', 'B': B, 'n': n, 'C': C, 'beam': args.beam,
               'endpoint_ms': round(event_ms(lambda: e.push(x, nv), args.reps), 4),
               'cut_ms': round(event_ms(lambda: ops.ctc_beam_cut(state._state, state.shape, none, rules.max_segment,
                                                                 logits=x, n_valid=nv), args.reps), 4),
               'empty_push_ms': round(event_ms(lambda: state.push(x, zero), args.reps), 4),
               'push_cut_no_cut_ms': round(event_ms(lambda: (state.reset(), state.push_cut(x, nv, none)), args.reps), 4),
               'push_ms': round(event_ms(lambda: (state.reset(), state.push(x, nv)), args.reps), 4)}
        print(json.dumps(row), flush=True)
        # offline: one launch against torch ops plus the host loop
        To = args.offline_frames
        xo = (torch.randn((B, To, C), generator=g) * 3).to(dev)
        xo[:, :, blank] += 6.0 * (torch.rand((B, To, 1), generator=g) < 0.6).to(dev)[:, :, 0]
        lens = [To] * B
        small = endpoint.EndpointRules(12, 5, 40, 0.8)
        t = time.perf_counter()
        got = endpoint.endpoints(xo, lens, blank, small).lists()
        torch.cuda.synchronize()
        first = (time.perf_counter() - t) * 1e3
        host = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            want = torch_endpoints(xo, lens, blank, small)
            host.append((time.perf_counter() - t) * 1e3)
        ours = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            got = endpoint.endpoints(xo, lens, blank, small).lists()
            ours.append((time.perf_counter() - t) * 1e3)
        row = {'what': 'offline', 'B': B, 'T': To, 'C': C, 'cuts': sum(len(c) for c in got), 'equal': got == want,
               'device_ms': round(event_ms(lambda: endpoint.endpoints(xo, lens, blank, small), args.reps), 4),
               'with_lists_host_ms_median': round(float(np.median(ours)), 4),
               'torch_and_host_loop_ms_median': round(float(np.median(host)), 4), 'first_call_ms': round(first, 3)}
        print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
