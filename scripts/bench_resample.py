#!/usr/bin/env python
"""Time of the device resampler on one GPU (srf_amd/resample.py, csrc/resample.hip).

Offline: ``Resampler`` on --batch utterances of --seconds of int16 audio (28 x 8 s by
default) at 48, 44.1 and 8 kHz and through the speed bank (14 400 / 16 000 / 17 600 Hz, rows
in turn), the Python entry point and its launch alone on buffers allocated once.  Next to
each, in the same session: the ``Fbank`` call on the resampled audio (the resampler's share
of the front end), and the same filter as ``torch.nn.functional.conv1d`` on the device --
what a user would write without the kernel: weight [ou, 1, K] with every phase's taps at
its own offset first[p] - first[0] (K = first[ou - 1] - first[0] + taps), stride iu, the
phases interleaved afterwards; the bank as one such call per rate on its rows.  Streaming:
one ``ResampleStream.push`` of 640 ms of 48 kHz audio for 1 and 28 streams next to the
``FbankStream.push`` of the 16 kHz samples it releases.  Method of scripts/bench_fbank.py:
after --warmup calls of each, --windows windows per entry point, alternating, each of --reps
back-to-back calls between two device events; the figures are per call.  ``traffic_GBps`` is
(bytes in + bytes out) / time of the launch alone, to be read beside the 6.3 TB/s that HBM
sustains.  One JSON line per configuration; no gate.

    python scripts/bench_resample.py [--batch 28] [--seconds 8] [--streams 1 28]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'scripts'))

from bench_fbank import audio, rounds  # noqa: E402

CHUNK_MS = 640


def conv_form(rs, entry, dev):
    """x [B, N] float32 -> [B, ceil(N ou / iu)]: the filter of bank entry ``entry`` as one conv1d."""
    f = rs.filters[entry]
    iu, ou, taps, first = f['iu'], f['ou'], f['taps'], f['first']
    K = int(first[-1] - first[0]) + taps
    w = torch.zeros((ou, 1, K))
    for p in range(ou):
        w[p, 0, int(first[p] - first[0]):int(first[p] - first[0]) + taps] = torch.from_numpy(f['w'][p])
    w, left = w.to(dev), int(-first[0])

    def run(x):
        B, N = x.shape
        M = (N * ou + iu - 1) // iu
        units = (M + ou - 1) // ou
        right = max(0, (units - 1) * iu + K - left - N)
        y = F.conv1d(F.pad(x[:, None, :], (left, right)), w, stride=iu)     # [B, ou, units]
        return y.transpose(1, 2).reshape(B, -1)[:, :M]
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=28)
    ap.add_argument('--seconds', type=float, default=8.0)
    ap.add_argument('--streams', nargs='+', type=int, default=[1, 28])
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--windows', type=int, default=10)
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_resample.py needs a HIP device: times are measured, never estimated')
    from srf_amd import fbank, resample
    dev = torch.device('cuda:0')
    fe = fbank.Fbank(device=dev)
    B = args.batch

    for name, rates in [('48000', [48000]), ('44100', [44100]), ('8000', [8000]), ('speed', [14400, 16000, 17600])]:
        rs = resample.Resampler(rates if len(rates) > 1 else rates[0], device=dev)
        N = int(args.seconds * (rates[0] if len(rates) == 1 else 16000))
        x, n = audio(B, N, 1).to(dev), torch.full((B,), N, dtype=torch.int32, device=dev)
        choice = None if len(rates) == 1 else torch.arange(B) % len(rates)
        choice_dev = None if choice is None else choice.to(device=dev, dtype=torch.int32)
        y, n16 = rs(x, n, choice)
        M = y.shape[1]
        xf = x.float()
        convs = [conv_form(rs, e, dev) for e in range(len(rates))]
        rows = [torch.arange(B)] if choice is None else [(choice == e).nonzero()[:, 0].to(dev) for e in range(len(rates))]
        if choice is None:
            conv = lambda: convs[0](xf)   # noqa: E731
            got = convs[0](xf)
            agree = float((got[:, 64:-64] - y[:, 64:-64]).abs().max())
        else:
            conv = lambda: [c(xf[r]) for c, r in zip(convs, rows)]   # noqa: E731
            agree = max(float((c(xf[r])[:, 64:m - 64] - y[r][:, 64:m - 64]).abs().max())
                        for c, r, m in zip(convs, rows, [int(n16[int(r[0])]) for r in rows]))
        res = rounds({'resample_us': (lambda: rs(x, n, choice), None),
                      'launch_us': (lambda: rs._launch(x, n, choice_dev, N, 0, N, 0, M, y, 0), None),
                      'fbank_us': (lambda: fe(y, n16), None),
                      'conv1d_us': (conv, None)},
                     args.warmup, args.windows, args.reps)
        nbytes = x.numel() * x.element_size() + int(n16.sum()) * 4
        print(json.dumps({'mode': 'offline', 'rates_in': rates, 'B': B, 'seconds': args.seconds, 'samples': N,
                          'outputs': M, 'taps': [f['taps'] for f in rs.filters], 'windows': args.windows,
                          'reps': args.reps, **res, 'conv1d_max_abs_diff': agree,
                          'launch_over_conv1d': round(res['launch_us']['median'] / res['conv1d_us']['median'], 4),
                          'resample_over_frontend': round(res['resample_us']['median'] /
                                                          (res['resample_us']['median'] + res['fbank_us']['median']), 4),
                          'bytes': nbytes, 'traffic_GBps': round(nbytes / res['launch_us']['median'] * 1e-3, 1)}),
              flush=True)

    rs = resample.Resampler(48000, device=dev)
    ns = 48 * CHUNK_MS
    for S in args.streams:
        chunk = audio(S, ns, 2 + S).to(dev)
        st = resample.ResampleStream(rs, S, ns)
        m = st.push(chunk).shape[1]
        chunk16 = audio(S, m, 3 + S).to(dev)
        fs = fbank.FbankStream(fe, S, m)
        res = rounds({'resample_chunk_us': (lambda: st.push(chunk), st.reset),
                      'fbank_chunk_us': (lambda: fs.push(chunk16), fs.reset)},
                     args.warmup, args.windows, args.reps)
        print(json.dumps({'mode': 'stream', 'streams': S, 'rate_in': 48000, 'chunk_ms': CHUNK_MS, 'chunk_samples': ns,
                          'first_chunk_outputs': m, 'windows': args.windows, 'reps': args.reps, **res}), flush=True)


if __name__ == '__main__':
    main()
