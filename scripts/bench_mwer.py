#!/usr/bin/env python
"""Time of the device MWER path on one GPU next to its yardstick,
ctc_loss_and_grad at the same shape in the same run.  Shape: B = 28, T' = 200, C = 32,
beam 16, N = 4 and N = 8 hypotheses.  The logits follow a random reference of 45 labels
per utterance (each label two frames, two blank frames between; + 4 on the path's class
over unit noise), so the beam's hypotheses are about as long as the reference, as in
training.  Timed, per call:
  nbest_us       srf_ctc_beam_nbest on the pushed state
  mwer_us        mwer.mwer_loss_and_grad on that list and its errors
  addition_us    everything an MWER step adds to a CTC step: state, reset, push, N-best,
                 hypothesis_errors (label errors) and mwer_loss_and_grad
  beam_us        state, reset and push alone
  errors_us      hypothesis_errors alone
  ctc_us         ctc.ctc_loss_and_grad (the loss head of a plain step)
After --warmup calls of each, --windows windows per entry, alternating, each of --reps
back-to-back calls between two device events.  One JSON line per N; no gate.

    python scripts/bench_mwer.py [--n-best 4 8]
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


def inputs(B, T, C, L, dev):
    rng = np.random.default_rng(16)
    blank = C - 1
    x = rng.standard_normal((B, T, C)).astype(np.float32)
    ref = rng.integers(0, blank, size=(B, L))
    for b in range(B):
        path = np.full(T, blank)
        for k in range(L):
            path[4 * k:4 * k + 2] = ref[b, k]
        x[b, np.arange(T), path] += 4.0
    lens = np.full(B, T)
    lens[1::2] -= rng.integers(0, 20, size=len(lens[1::2]))   # ragged, as a cropped batch is
    return (torch.tensor(x, device=dev), torch.tensor(lens, dtype=torch.int32, device=dev),
            torch.tensor(ref, dtype=torch.int32, device=dev), torch.full((B,), L, dtype=torch.int32, device=dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=28)
    ap.add_argument('--frames', type=int, default=200)
    ap.add_argument('--classes', type=int, default=32)
    ap.add_argument('--beam', type=int, default=16)
    ap.add_argument('--n-best', nargs='+', type=int, default=[4, 8])
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--windows', type=int, default=10)
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_mwer.py needs a HIP device: times are measured, never estimated')
    from srf_amd import ctc, mwer, ops
    dev = torch.device('cuda:0')
    B, T, C, W, L = args.batch, args.frames, args.classes, args.beam, 45
    blank = C - 1
    x, lens, ref, ref_len = inputs(B, T, C, L, dev)
    scale = 1.0 / B
    for N in args.n_best:
        state = ctc.BeamState(B, C, blank, W, T, dev)
        state.push(x, lens)
        nbest = state.nbest(N)
        errors = mwer.hypothesis_errors(nbest, ref, ref_len)

        def nbest_call():
            ops.ctc_beam_nbest(state._state, state.shape, N, T)

        def mwer_call():
            mwer.mwer_loss_and_grad(x, lens, nbest, errors, blank, scale)

        def beam_call():
            s = ctc.BeamState(B, C, blank, W, T, dev)
            s.push(x, lens)
            return s

        def errors_call():
            mwer.hypothesis_errors(nbest, ref, ref_len)

        def addition():
            nb = beam_call().nbest(N)
            mwer.mwer_loss_and_grad(x, lens, nb, mwer.hypothesis_errors(nb, ref, ref_len), blank, scale)

        def ctc_call():
            ctc.ctc_loss_and_grad(ref, x, ref_len, lens, blank, scale)

        fns = {'nbest_us': nbest_call, 'mwer_us': mwer_call, 'beam_us': beam_call, 'errors_us': errors_call,
               'addition_us': addition, 'ctc_us': ctc_call}
        for _ in range(args.warmup):
            for fn in fns.values():
                fn()
        times = {k: [] for k in fns}
        for _ in range(args.windows):
            for k, fn in fns.items():
                times[k].append(window(fn, args.reps))
        loss, _, p_hat, _ = mwer.mwer_loss_and_grad(x, lens, nbest, errors, blank, scale)
        out = {'B': B, 'T': T, 'C': C, 'beam': W, 'N': N, 'ref_labels': L, 'windows': args.windows, 'reps': args.reps}
        out.update({k: stats(v) for k, v in times.items()})
        out.update({'mean_hyp_len': round(float(nbest.lengths.float().mean()), 1),
                    'mean_errors': round(float(errors.float().mean()), 2),
                    'mean_top_p': round(float(p_hat.max(dim=1).values.mean()), 3),
                    'mean_loss': round(float(loss.mean()), 4),
                    'workspace_MiB': round(ops._lib.lib().srf_mwer_workspace(B, T, C, N, T) / 2 ** 20, 1)})
        print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
