#!/usr/bin/env python
"""Time of the sliding-window CMVN on one GPU (srf_amd/fbank.py SlidingCmvn, csrc/cmvn.hip).

Offline, on --batch utterances of --seconds (28 x 8 s, 800 frames, by default), window 600
with a prior: ``sc(feats, n)`` and its launch alone on buffers allocated once, the torch
restatement a user would otherwise write (fp64 ``cumsum`` and differences), and ``fe(samples,
n)`` with the sliding CMVN next to ``fe`` with a ``(mean, std)`` tuple.  Streaming, a chunk of
64 frames (10 240 samples) for 1 and 28 streams: ``FbankStream.push`` and
``StreamingRouter.push_audio`` (the C4 model by default), each with the sliding CMVN next to
the tuple one, and ``SlidingCmvnStream.push`` alone.  Method of scripts/bench_fbank.py: after
--warmup calls of each, --windows windows per entry point, alternating, each of --reps
back-to-back calls between two device events (a streaming window is one session of --reps
chunks after a reset); the figures are per call.  One JSON line per configuration; no gate.

    python scripts/bench_cmvn.py [--batch 28] [--seconds 8] [--streams 1 28] [--model c4_real]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

from scripts.bench_fbank import audio, rounds   # noqa: E402

CHUNK_FRAMES = 64


def torch_sliding(x, n_frames, W, mean_p, std_p, count_p):
    """The definition of DESIGN.md section 20 with torch ops: fp64 cumulative sums and their
    differences (whose error grows with the stream's length, unlike the kernel's)."""
    B, T, D = x.shape
    xd = x.double()
    c1 = torch.cat([xd.new_zeros((B, 1, D)), torch.cumsum(xd, 1)], 1)
    c2 = torch.cat([xd.new_zeros((B, 1, D)), torch.cumsum(xd * xd, 1)], 1)
    t = torch.arange(T, device=x.device)
    lo = (t - W + 1).clamp(min=0)
    n = (t - lo + 1).double()[None, :, None]
    c = (W - n).clamp(max=count_p)
    m = (c1[:, 1:] - c1[:, lo] + c * mean_p) / (n + c)
    q = (c2[:, 1:] - c2[:, lo] + c * (std_p * std_p + mean_p * mean_p)) / (n + c)
    y = (xd - m) / torch.sqrt((q - m * m).clamp(min=1e-10))
    return (y * (t[None, :, None] < n_frames[:, None, None])).float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=28)
    ap.add_argument('--seconds', type=float, default=8.0)
    ap.add_argument('--window', type=int, default=600)
    ap.add_argument('--streams', nargs='+', type=int, default=[1, 28])
    ap.add_argument('--model', default='c4_real')
    ap.add_argument('--offline-only', action='store_true')
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--windows', type=int, default=10)
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_cmvn.py needs a HIP device: times are measured, never estimated')
    from srf_amd import fbank
    from srf_amd.sequence_router import SequenceRouter
    from srf_amd.streaming import StreamingRouter
    from tests.helpers import config_from_shape, load_eval_fixture
    dev = torch.device('cuda:0')
    D = fbank.N_FEAT
    rng = np.random.default_rng(0)
    cm = (np.concatenate([rng.uniform(8, 16, 41), rng.uniform(-0.2, 0.2, 82)]).astype(np.float32),
          np.concatenate([rng.uniform(2, 5, 41), rng.uniform(0.4, 1.5, 82)]).astype(np.float32))
    sc = fbank.SlidingCmvn(window=args.window, prior=cm, device=dev)
    fe_tuple, fe_slide = fbank.Fbank(cmvn=cm, device=dev), fbank.Fbank(cmvn=sc, device=dev)

    # offline
    B, N = args.batch, int(args.seconds * 16000)
    x, n = audio(B, N, 1).to(dev), torch.full((B,), N, dtype=torch.int32, device=dev)
    T = fbank.n_frames(N)
    nfr = torch.full((B,), T, dtype=torch.int32, device=dev)
    raw = torch.from_numpy(cm[0] + cm[1] * rng.standard_normal((B, T, D)).astype(np.float32)).to(dev)
    out = torch.empty_like(raw)
    prior = (sc.mean, sc.std, sc.count)
    pm, ps = sc.mean[0], sc.std[0]
    diff = float((torch_sliding(raw, nfr, args.window, pm, ps, sc.prior_frames) - sc(raw, nfr)).abs().max())
    res = rounds({'cmvn_us': (lambda: sc(raw, nfr), None),
                  'cmvn_launch_us': (lambda: sc._launch(raw, nfr, 0, 0, T, prior, out, 0, None), None),
                  'torch_cumsum_us': (lambda: torch_sliding(raw, nfr, args.window, pm, ps, sc.prior_frames), None),
                  'fbank_sliding_us': (lambda: fe_slide(x, n), None),
                  'fbank_tuple_us': (lambda: fe_tuple(x, n), None)},
                 args.warmup, args.windows, args.reps)
    moved = 2 * B * T * D * 4
    print(json.dumps({'mode': 'offline', 'B': B, 'seconds': args.seconds, 'frames': T, 'window': args.window,
                      'tile': fbank.CMVN_TILE, 'lib': os.environ.get('SRF_LIB_PATH', 'default'),
                      'windows': args.windows, 'reps': args.reps, **res,
                      'bytes_in_plus_out': moved,
                      'launch_GBps_of_in_plus_out': round(moved / res['cmvn_launch_us']['median'] * 1e-3, 1),
                      'torch_minus_kernel_max_abs': diff}), flush=True)
    if args.offline_only:
        return

    # one streaming chunk, the sliding CMVN next to the tuple one
    kw, sh = load_eval_fixture(args.model)[:2]
    model = SequenceRouter(config_from_shape(kw), None, sh.class_n, device=dev, seed=1)
    ns = CHUNK_FRAMES * fbank.FRAME_SHIFT
    for S in args.streams:
        chunk = audio(S, ns, 2 + S).to(dev)
        feats = torch.randn((S, CHUNK_FRAMES, D), generator=torch.Generator().manual_seed(S)).to(dev)
        cs = fbank.SlidingCmvnStream(sc, S, CHUNK_FRAMES)
        fs_t, fs_s = fbank.FbankStream(fe_tuple, S, ns), fbank.FbankStream(fe_slide, S, ns)
        r_t = StreamingRouter(model, S, max_chunk=CHUNK_FRAMES + 8, frontend=fe_tuple)
        r_s = StreamingRouter(model, S, max_chunk=CHUNK_FRAMES + 8, frontend=fe_slide)
        res = rounds({'cmvn_chunk_us': (lambda: cs.push(feats), cs.reset),
                      'fbank_chunk_sliding_us': (lambda: fs_s.push(chunk), fs_s.reset),
                      'fbank_chunk_tuple_us': (lambda: fs_t.push(chunk), fs_t.reset),
                      'push_audio_sliding_us': (lambda: r_s.push_audio(chunk), r_s.reset),
                      'push_audio_tuple_us': (lambda: r_t.push_audio(chunk), r_t.reset)},
                     args.warmup, args.windows, args.reps)
        print(json.dumps({'mode': 'stream', 'streams': S, 'chunk_frames': CHUNK_FRAMES, 'chunk_samples': ns,
                          'window': args.window, 'model': args.model, 'windows': args.windows, 'reps': args.reps,
                          **res,
                          'fbank_chunk_added_us': round(res['fbank_chunk_sliding_us']['median']
                                                        - res['fbank_chunk_tuple_us']['median'], 2),
                          'push_audio_added_us': round(res['push_audio_sliding_us']['median']
                                                       - res['push_audio_tuple_us']['median'], 2)}), flush=True)


if __name__ == '__main__':
    main()
