"""srf_ctc_beam_nbest (ctc.BeamState.nbest) against the float64 beam of tests/mwer_ref.py.

Adjacent totals among the top N + 1 prefixes lie closer than fp32 can order (the float64
gaps go down to 2e-5 on these shapes), so the order itself is not compared.  Checked:
row 0 is best() bit for bit; rows are distinct and log_prob does not increase; n_hyp;
every returned prefix is in the float64 beam with its total within 1e-4 (1 + |want|) (the
tolerance of tests/test_ctc_beam_device_gpu.py); every float64 prefix that leads the
device's last returned score by more than twice that tolerance is returned; any chunking
of the frames gives the same bits; nothing is written past a row's count, and a row longer
than max_len is flagged with count = -1.  N <= W / 2 except in the last case, so rounding
at the beam's edge cannot move the top N.
"""
import functools

import numpy as np
import pytest
import torch

from srf_amd import ctc, ops
from tests import mwer_ref

pytestmark = pytest.mark.gpu

CASES = [(12, 6, 8, 4), (40, 8, 16, 4), (50, 32, 32, 8), (30, 63, 100, 8), (9, 128, 128, 64)]   # (T, C, W, N)
SEEDS = (0, 1, 2)
SCALES = (1.0, 3.0)
POISON = -77


@functools.lru_cache(maxsize=None)
def _batch(T, C, W):
    """Six utterances (seed x scale) of ragged lengths and one without a frame; the
    float64 beam of each, computed once."""
    rows, lens = [], []
    for k, (seed, scale) in enumerate((s, a) for s in SEEDS for a in SCALES):
        rows.append((np.random.default_rng(7000 + seed).standard_normal((T, C)) * scale).astype(np.float32))
        lens.append(T - (k % 3) * max(1, T // 6))
    rows.append(np.zeros((T, C), np.float32))
    lens.append(0)
    x = np.stack(rows)
    beams = [mwer_ref.beam_nbest(x[b, :lens[b]], C - 1, W) for b in range(len(lens))]
    return x, lens, beams


def _tol(v):
    return 1e-4 * (1 + abs(v))


def _pushed(x, lens, C, W, chunk, dev):
    B, T, _ = x.shape
    state = ctc.BeamState(B, C, C - 1, W, T, dev)
    xt = torch.tensor(x, device=dev)
    lt = torch.tensor(lens, dtype=torch.int32, device=dev)
    for t0 in range(0, T, chunk):
        state.push(xt[:, t0:t0 + chunk].contiguous(), (lt - t0).clamp(min=0))
    return state


@pytest.mark.parametrize('T,C,W,N', CASES)
def test_nbest_against_float64_beam(cuda, T, C, W, N):
    x, lens, beams = _batch(T, C, W)
    B = len(lens)
    state = _pushed(x, lens, C, W, T, cuda)
    nb = state.nbest(N)
    assert tuple(nb.labels.shape) == (B, N, T) and tuple(nb.lengths.shape) == (B, N)
    # 1. row 0 is best(), bit for bit
    bl, bc, bp = state.best_device()
    assert torch.equal(nb.lengths[:, 0], bc)
    assert torch.equal(nb.log_prob[:, 0].contiguous().view(torch.int32), bp.view(torch.int32))
    for b in range(B):
        n = int(bc[b])
        assert torch.equal(nb.labels[b, 0, :n], bl[b, :n])
    lists = nb.lists()
    count = nb.count.cpu().tolist()
    lengths = nb.lengths.cpu().tolist()
    logp = nb.log_prob.cpu().double().numpy()
    for b in range(B):
        want = dict(beams[b])
        got = lists[b]
        # 3. n_hyp; the rows past it
        assert count[b] == min(N, len(beams[b])) == len(got), (b, count[b], len(beams[b]))
        assert all(v == 0 for v in lengths[b][count[b]:]) and (logp[b, count[b]:] == -np.inf).all()
        # 2. distinct, not increasing
        prefixes = [tuple(p) for p, _ in got]
        assert len(set(prefixes)) == len(prefixes), b
        scores = [v for _, v in got]
        assert all(a >= c for a, c in zip(scores, scores[1:])), (b, scores)
        # 4. every returned prefix is in the float64 beam, with its total
        for p, v in zip(prefixes, scores):
            assert p in want, (b, p)
            assert abs(v - want[p]) <= _tol(want[p]), (b, p, v, want[p])
        # 5. every float64 prefix clearly above the last returned score is returned
        if count[b] == N:
            for p, v in beams[b]:
                if v > scores[-1] + 2 * _tol(v):
                    assert p in prefixes, (b, p, v, scores[-1])
    # the utterance without a frame holds the empty prefix alone
    assert count[-1] == 1 and lists[-1][0][0] == [] and lists[-1][0][1] == 0.0


@pytest.mark.parametrize('T,C,W,N', CASES[:3])
def test_chunking_gives_the_same_bits(cuda, T, C, W, N):
    x, lens, _ = _batch(T, C, W)
    ref = None
    for chunk in (T, 7, 1):
        nb = _pushed(x, lens, C, W, chunk, cuda).nbest(N)
        mask = torch.arange(T, device=cuda)[None, None, :] < nb.lengths[:, :, None]
        got = (torch.where(mask, nb.labels, torch.zeros_like(nb.labels)), nb.lengths, nb.log_prob.view(torch.int32),
               nb.count)
        if ref is None:
            ref = got
        for a, c in zip(ref, got):
            assert torch.equal(a, c), chunk


def test_padding_is_left_alone_and_long_rows_are_flagged(cuda):
    T, C, W, N = CASES[1]
    x, lens, _ = _batch(T, C, W)
    B = len(lens)
    state = _pushed(x, lens, C, W, T, cuda)
    labels = torch.full((B, N, T), POISON, dtype=torch.int32, device=cuda)
    out, lengths, logp, count = ops.ctc_beam_nbest(state._state, state.shape, N, T, labels=labels)
    assert out is labels
    mask = torch.arange(T, device=cuda)[None, None, :] < lengths[:, :, None]
    assert bool((labels[~mask] == POISON).all()) and bool((labels[mask] != POISON).all())
    # between pushes the state is not changed: the same call again, the same bits
    again = ops.ctc_beam_nbest(state._state, state.shape, N, T)
    assert torch.equal(again[1], lengths) and torch.equal(again[2].view(torch.int32), logp.view(torch.int32))
    # max_len one short of the longest row: that row (and every row as long) gets -1
    longest = int(lengths.max())
    assert longest >= 2
    short = torch.full((B, N, longest - 1), POISON, dtype=torch.int32, device=cuda)
    _, len2, logp2, count2 = ops.ctc_beam_nbest(state._state, state.shape, N, longest - 1, labels=short)
    assert torch.equal(count2, count) and torch.equal(logp2.view(torch.int32), logp.view(torch.int32))
    too_long = lengths > longest - 1
    assert bool(too_long.any()) and bool((len2[too_long] == -1).all()) and torch.equal(len2[~too_long],
                                                                                      lengths[~too_long])
    assert bool((short[too_long] == POISON).all())
    keep = ~too_long[:, :, None] & (torch.arange(longest - 1, device=cuda)[None, None, :] < lengths[:, :, None])
    assert torch.equal(short[keep], labels[:, :, :longest - 1][keep])
    with pytest.raises(ValueError, match='beam_width'):
        state.nbest(W + 1)
    with pytest.raises(ValueError, match='max_len'):
        state.nbest(N, max_len=0)
