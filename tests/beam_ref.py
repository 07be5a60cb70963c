"""Float64 restatement of the CTC prefix beam search (srf_ctc_beam_search on the host,
srf_ctc_beam_* on the device), with prefixes as tuples, and the case list on which the
device decoder is compared with the host decoder.

Ties are broken as the host decoder breaks them, by first creation, stated the way the
device kernel states it: walking the beam in slot order, slot k creates the prefix itself
(key k C) and then its extensions by ascending class (key k C + 1 + rank of the class
among the non-blank ones); a prefix reached twice keeps the smaller key; the beam_width
candidates that come first by (total descending, key ascending) survive, in that order.
"""
import math

import numpy as np

NEG_INF = -math.inf

# (T, C, W): random logits of scale 3 (seeds 0 .. 7), blank = C - 1.  On all 56 cases the
# float64 restatement and the fp32 host decoder return the same labelling
# (tests/test_ctc_beam_device_cpu.py), so rounding does not decide the answer.
CASES = [(40, 8, 4), (40, 8, 16), (60, 32, 16), (50, 63, 100), (64, 33, 100), (50, 63, 128), (30, 128, 128)]
SEEDS = range(8)
# (T, C, W) decoded on all-zero logits: every extension of a prefix ties with its
# siblings, so which prefixes stay is decided by the order of creation alone
TIE_CASES = [(3, 4, 2), (4, 5, 3), (5, 3, 4), (12, 20, 50), (9, 128, 128)]
# Flat logits (scale 1, seeds 5000 .. 5039, blank = C - 1) at a narrow beam: prefixes
# leave the beam while a child of theirs stays and are made again a frame later, when
# their extension has to merge with that child again (the host's persistent node map does
# this; beam_search counts the events in stats['readopted']).  A decoder that identifies
# a parent by anything that does not survive its absence from the beam splits the
# probability there and returns another labelling on seeds 36 and 38.
READOPT_CASE = (40, 8, 16)
READOPT_SEEDS = range(40)


def case_logits(seed, T, C):
    return (np.random.default_rng(1000 + seed).standard_normal((T, C)) * 3).astype(np.float32)


def readopt_logits(seed):
    T, C, _ = READOPT_CASE
    return np.random.default_rng(5000 + seed).standard_normal((T, C)).astype(np.float32)


def beam_search(logits, blank, beam_width, stats=None):
    """logits [T, C] -> (labels, log probability, gap): the most probable prefix after
    the last frame, and how far the second most probable one lies below it (inf if
    there is none).

    The beam holds distinct prefixes, so the extension of slot p by class c is a prefix
    that some other candidate also is only if a beam entry n is that very prefix,
    n = prefix(p) + (c,): then the two are one candidate, with both contributions and the
    smaller key.  Everything else is a candidate of its own, so a frame is array work.

    stats (a dict) gets 'readopted': how often an entry merged with the extension of a
    parent that was not in the beam one frame earlier although the entry itself was."""
    x = np.asarray(logits, dtype=np.float64)
    T, C = x.shape
    lse = np.logaddexp   # max + log1p(exp(-|a - b|)), -inf as the neutral element
    rank = np.cumsum(np.arange(C) != blank)   # key of extension c of slot k: k C + rank[c]
    prefixes, pb, pnb = [()], np.array([0.0]), np.array([NEG_INF])   # in rank order
    before, readopted = set(), 0   # the beam one frame earlier
    for t in range(T):
        mx = x[t].max()
        lp = x[t] - (mx + math.log(np.exp(x[t] - mx).sum()))
        n = len(prefixes)
        slot = {p: k for k, p in enumerate(prefixes)}
        last = np.array([p[-1] if p else -1 for p in prefixes])
        tot = lse(pb, pnb)
        # extensions [slot, class]: -inf source probabilities and the blank create none
        prev = np.repeat(tot[:, None], C, axis=1)
        has = last >= 0
        prev[has, last[has]] = pb[has]
        ext = prev + lp[None, :]
        made = prev > NEG_INF
        made[:, blank] = False
        ext_key = np.arange(n)[:, None] * C + rank[None, :]
        # the prefixes themselves
        npb = tot + lp[blank]
        npnb = np.where(has, pnb + lp[np.maximum(last, 0)], NEG_INF)
        own_key = np.arange(n) * C
        for k, p in enumerate(prefixes):
            par = slot.get(p[:-1]) if p else None
            if par is not None and made[par, last[k]]:
                npnb[k] = lse(npnb[k], ext[par, last[k]])
                own_key[k] = min(own_key[k], ext_key[par, last[k]])
                made[par, last[k]] = False
                readopted += p in before and p[:-1] not in before
        before = set(prefixes)
        ks, cs = np.nonzero(made)
        totals = np.concatenate([lse(npb, npnb), ext[ks, cs]])
        keys = np.concatenate([own_key, ext_key[ks, cs]])
        assert len(set(keys.tolist())) == len(keys)
        order = np.lexsort((keys, -totals))[:beam_width]   # total descending, then key ascending
        new_prefixes, new_pb, new_pnb = [], [], []
        for i in order:
            if i < n:
                new_prefixes.append(prefixes[i])
                new_pb.append(npb[i])
                new_pnb.append(npnb[i])
            else:
                new_prefixes.append(prefixes[ks[i - n]] + (int(cs[i - n]),))
                new_pb.append(NEG_INF)
                new_pnb.append(ext[ks[i - n], cs[i - n]])
        prefixes, pb, pnb = new_prefixes, np.array(new_pb), np.array(new_pnb)
    if stats is not None:
        stats['readopted'] = stats.get('readopted', 0) + readopted
    tots = lse(pb, pnb)
    gap = float(tots[0] - tots[1]) if len(tots) > 1 else math.inf
    return list(prefixes[0]), float(tots[0]), gap
