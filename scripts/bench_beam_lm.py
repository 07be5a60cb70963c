#!/usr/bin/env python
"""Per-frame time of the device CTC beam search with and without a fused language model,
from one process: the push launch (events) of ctc.BeamState with lm=None and with a
FusedLM, at the decode shape T' = 200, beam 100, B = 1 and 28, for C = 63 (trigram-shaped
automaton, 3 907 states, 1 MB per table) and C = 32 (4-gram-shaped, 30 784 states, 3.9 MB
per table: the size of a WSJ character 4-gram, read from L2).  Random logits of scale 3 (the
recipe of tests/beam_ref.py's case list), random bonuses: times do not depend on the values
beyond which candidates survive.  Per configuration: --warmup pushes, then --calls timed
ones, fused and unfused alternating.  One JSON line per configuration; no gate.

    python scripts/bench_beam_lm.py [--batch 1 28] [--frames 200] [--classes 63 32] [--beam 100]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)


def case_logits(seed, T, C):
    return (np.random.default_rng(1000 + seed).standard_normal((T, C)) * 3).astype(np.float32)


def full_automaton(C, order, seed=0):
    """Every context of up to order - 1 labels is a state (blank C - 1): bonus = 0.5 * a
    random log-distribution + 0.3, next = the context extended and cut to order - 1."""
    assert order >= 2
    L, keep = C - 1, order - 1
    offset = np.cumsum([0] + [L ** k for k in range(keep + 1)])   # first state of each context length
    S = int(offset[-1])
    nxt = np.zeros((S, C), np.int32)
    c = np.arange(L)
    for k in range(keep + 1):
        idx = np.arange(L ** k)[:, None]
        if k < keep:
            to = offset[k + 1] + idx * L + c[None, :]
        else:   # the oldest label leaves the context
            to = offset[k] + (idx % L ** (keep - 1)) * L + c[None, :]
        nxt[offset[k]:offset[k + 1], :L] = to
        nxt[offset[k]:offset[k + 1], L] = offset[k] + idx[:, 0]
    score = np.random.default_rng(seed).standard_normal((S, C)) * 2
    score[:, :L] -= np.log(np.exp(score[:, :L]).sum(axis=1, keepdims=True))
    return (0.5 * score + 0.3).astype(np.float32), nxt


def stats(ms):
    return {'median': round(float(np.median(ms)), 4), 'min': round(float(ms.min()), 4),
            'max': round(float(ms.max()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', nargs='+', type=int, default=[1, 28])
    ap.add_argument('--frames', type=int, default=200)
    ap.add_argument('--classes', nargs='+', type=int, default=[63, 32])
    ap.add_argument('--beam', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--calls', type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_beam_lm.py needs a HIP device: decode times are measured, never estimated')
    from srf_amd import ctc
    from srf_amd.lm import FusedLM
    dev = torch.device('cuda:0')
    T, W = args.frames, args.beam
    for C in args.classes:
        order = 4 if C <= 33 else 3
        lm = FusedLM.from_tables(*full_automaton(C, order), blank=C - 1, device=dev)
        for B in args.batch:
            x = torch.tensor(np.stack([case_logits(b, T, C) for b in range(B)]), device=dev)
            n_valid = torch.tensor([T] * B, device=dev, dtype=torch.int32)
            states = {'unfused': ctc.BeamState(B, C, C - 1, W, T, dev),
                      'fused': ctc.BeamState(B, C, C - 1, W, T, dev, lm=lm)}
            push = {k: [] for k in states}
            for i in range(args.warmup + args.calls):
                for name, state in states.items():
                    state.reset()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    state.push(x, n_valid)
                    e1.record()
                    torch.cuda.synchronize()
                    if i >= args.warmup:
                        push[name].append(e0.elapsed_time(e1))
            push = {k: np.array(v) for k, v in push.items()}
            fused, unfused = (float(np.median(push[k])) for k in ('fused', 'unfused'))
            hyp_f, hyp_u = states['fused'].best()[0], states['unfused'].best()[0]
            print(json.dumps({'B': B, 'frames': T, 'classes': C, 'beam': W, 'lm_order': order,
                              'lm_states': lm.n_states, 'table_mb': round(lm.n_states * C * 4 / 2 ** 20, 2),
                              'calls': args.calls, 'push_unfused_ms': stats(push['unfused']),
                              'push_fused_ms': stats(push['fused']),
                              'unfused_us_per_frame': round(unfused * 1e3 / T, 3),
                              'fused_us_per_frame': round(fused * 1e3 / T, 3),
                              'fused_over_unfused': round(fused / unfused, 4),
                              'labellings_differ': sum(a != b for a, b in zip(hyp_f, hyp_u))}), flush=True)


if __name__ == '__main__':
    main()
