"""Float64 restatement of the CTC prefix beam search with a fused language model
(srf_ctc_beam_search_lm on the host, srf_ctc_beam_lm_* on the device), with prefixes as
tuples, in the style of tests/beam_ref.py, whose case lists, key order and count of
re-adopted parents it shares; and the automaton the tests fuse.

The one change to beam_ref.beam_search: extending a prefix whose automaton state is s by
class c adds bonus[s][c], also where an entry folds its parent's extension in (with the
parent's state).  State and accumulated bonus are functions of the prefix alone.
"""
import itertools
import math

import numpy as np

NEG_INF = -math.inf


def case_automaton(C):
    """(bonus [S, C] float32, next [S, C] int32) for C classes, blank C - 1: an n-gram-shaped
    automaton of order 3 if C <= 33, else 2.  States are the tuples of the last order - 1
    labels (shorter at the start), numbered breadth-first from () in ascending class order;
    scores default_rng(77 + C).standard_normal((S, C)) * 2, log-softmaxed over the non-blank
    classes; bonus = float32(0.5 * score + 0.3), the blank's column 0.  S = 57, 993, 1057,
    63, 128 for C = 8, 32, 33, 63, 128."""
    blank, keep = C - 1, (3 if C <= 33 else 2) - 1
    index, queue = {(): 0}, [()]
    for h in queue:   # grows while it is walked: breadth-first
        for c in range(C - 1):
            n = (h + (c,))[-keep:]
            if n not in index:
                index[n] = len(index)
                queue.append(n)
    S = len(queue)
    nxt = np.zeros((S, C), np.int32)
    for h, s in index.items():
        nxt[s, blank] = s
        for c in range(C - 1):
            nxt[s, c] = index[(h + (c,))[-keep:]]
    score = np.random.default_rng(77 + C).standard_normal((S, C)) * 2
    lab = score[:, :blank]
    mx = lab.max(axis=1, keepdims=True)
    score[:, :blank] = lab - (mx + np.log(np.exp(lab - mx).sum(axis=1, keepdims=True)))
    bonus = (0.5 * score + 0.3).astype(np.float32)
    bonus[:, blank] = 0.0
    return bonus, nxt


def random_automaton(seed, S, C):
    """Any automaton: normal bonuses of scale 1, next uniform in [0, S)."""
    rng = np.random.default_rng(seed)
    bonus = rng.standard_normal((S, C)).astype(np.float32)
    bonus[:, C - 1] = 0.0
    return bonus, rng.integers(0, S, (S, C)).astype(np.int32)


def sequence_bonus(labels, bonus, nxt):
    """Sum of the bonuses of a label sequence from state 0, in float64."""
    s, acc = 0, 0.0
    for c in labels:
        acc += float(bonus[s, c])
        s = int(nxt[s, c])
    return acc


def beam_search(logits, blank, beam_width, bonus, nxt, stats=None):
    """logits [T, C] -> (labels, fused score, gap, lm score): the best prefix after the last
    frame by log p_ctc + bonuses, how far the second best lies below it (inf if there is
    none), and the best prefix's sum of bonuses.  stats as in beam_ref.beam_search."""
    x = np.asarray(logits, dtype=np.float64)
    bonus = np.asarray(bonus, dtype=np.float64)
    T, C = x.shape
    lse = np.logaddexp
    rank = np.cumsum(np.arange(C) != blank)
    prefixes, pb, pnb = [()], np.array([0.0]), np.array([NEG_INF])
    state, acc = [0], [0.0]
    before, readopted = set(), 0
    for t in range(T):
        mx = x[t].max()
        lp = x[t] - (mx + math.log(np.exp(x[t] - mx).sum()))
        n = len(prefixes)
        slot = {p: k for k, p in enumerate(prefixes)}
        last = np.array([p[-1] if p else -1 for p in prefixes])
        tot = lse(pb, pnb)
        prev = np.repeat(tot[:, None], C, axis=1)
        has = last >= 0
        prev[has, last[has]] = pb[has]
        ext = (prev + lp[None, :]) + bonus[state]
        made = prev > NEG_INF
        made[:, blank] = False
        ext_key = np.arange(n)[:, None] * C + rank[None, :]
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
        order = np.lexsort((keys, -totals))[:beam_width]
        new = []
        for i in order:
            if i < n:
                new.append((prefixes[i], npb[i], npnb[i], state[i], acc[i]))
            else:
                k, c = ks[i - n], int(cs[i - n])
                new.append((prefixes[k] + (c,), NEG_INF, ext[k, c], int(nxt[state[k], c]),
                            acc[k] + bonus[state[k], c]))
        prefixes, pb, pnb, state, acc = (list(v) for v in zip(*new))
        pb, pnb = np.array(pb), np.array(pnb)
    if stats is not None:
        stats['readopted'] = stats.get('readopted', 0) + readopted
    tots = lse(pb, pnb)
    gap = float(tots[0] - tots[1]) if len(tots) > 1 else math.inf
    return list(prefixes[0]), float(tots[0]), gap, float(acc[0])


def exhaustive(logp, blank, bonus, nxt):
    """(labels, score): the labelling with the largest log p_ctc + bonuses among all
    labellings of at most T labels, log p_ctc by torch's float64 CTC forward."""
    import torch
    T, C = logp.shape
    lp = torch.tensor(logp, dtype=torch.float64).unsqueeze(1)
    best, best_v = None, -np.inf
    for n in range(T + 1):
        for lab in itertools.product([c for c in range(C) if c != blank], repeat=n):
            tgt = torch.tensor([list(lab) if lab else [0]], dtype=torch.long)
            nll = torch.nn.functional.ctc_loss(lp, tgt, torch.tensor([T]), torch.tensor([n]), blank=blank,
                                               reduction='none', zero_infinity=False)
            v = -float(nll[0]) + sequence_bonus(lab, bonus, nxt)
            if v > best_v:
                best, best_v = list(lab), v
    return best, best_v
