"""Float64 restatement of the MWER loss (srf_mwer_loss, include/srf.h) and of the N-best
output of the CTC prefix beam search (srf_ctc_beam_nbest), for the tests.

Per utterance with log-softmax lp [T, C], hypotheses y_0 .. y_{n-1} and integer errors e_i:
    ll_i = log P_CTC(y_i | x)   (the full sum over alignments; -inf if infeasible or T = 0)
    p_i = exp(ll_i - LSE_k ll_k),  ebar = sum(e) / n,  loss = sum_i p_i (e_i - ebar)
    w_i = p_i (e_i - ebar - loss),  grad = grad_scale * sum_i w_i occ_i
    occ_i[t, c] = exp(LSE_{s: ext_i[s] = c}(alpha_i[t, s] + beta_i[t, s]) - lp[t, c] - ll_i)
alpha and beta both include the emission at t.  ``torch_mwer`` states the same loss with
torch.nn.functional.ctc_loss and autograd in a given dtype: an independent oracle in
float64, and in float32 the measure of what fp32 arithmetic costs on given inputs.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

NEG_INF = -math.inf


def log_softmax(x):
    x = np.asarray(x, dtype=np.float64)
    mx = x.max(axis=-1, keepdims=True)
    return x - (mx + np.log(np.exp(x - mx).sum(axis=-1, keepdims=True)))


def _lse(*terms):
    with np.errstate(invalid='ignore', divide='ignore'):
        st = np.stack(terms)
        m = st.max(axis=0)
        ms = np.where(np.isfinite(m), m, 0.0)
        return ms + np.log(np.exp(st - ms).sum(axis=0))


def _shift(a, k):
    """out[s] = a[s - k], -inf where s - k falls outside."""
    out = np.full(len(a), NEG_INF)
    if k > 0:
        out[k:] = a[:len(a) - k] if k < len(a) else []
    else:
        out[:len(a) + k] = a[-k:] if -k < len(a) else []
    return out


def ctc_alpha_beta(lp, labels, blank):
    """(alpha [T, S], beta [T, S], ll) of one hypothesis on lp [T, C], S = 2 L + 1."""
    T = lp.shape[0]
    L = len(labels)
    S = 2 * L + 1
    ext = np.full(S, blank, dtype=np.int64)
    ext[1::2] = labels
    skip = np.zeros(S, dtype=bool)          # s may be entered from s - 2
    skip[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
    alpha = np.full((T, S), NEG_INF)
    beta = np.full((T, S), NEG_INF)
    if T == 0:
        return alpha, beta, NEG_INF
    alpha[0, :2] = lp[0, ext[:2]]
    for t in range(1, T):
        a = alpha[t - 1]
        a1 = _shift(a, 1)
        a2 = np.where(skip, _shift(a, 2), NEG_INF)
        alpha[t] = _lse(a, a1, a2) + lp[t, ext]
    beta[T - 1, max(S - 2, 0):] = lp[T - 1, ext[max(S - 2, 0):]]
    skip_from = np.zeros(S, dtype=bool)     # s may move to s + 2
    skip_from[:max(S - 2, 0)] = skip[2:]
    for t in range(T - 2, -1, -1):
        b = beta[t + 1]
        b1 = _shift(b, -1)
        b2 = np.where(skip_from, _shift(b, -2), NEG_INF)
        beta[t] = _lse(b, b1, b2) + lp[t, ext]
    ll = float(_lse(*[np.array(v) for v in alpha[T - 1, max(S - 2, 0):]]))
    return alpha, beta, ll


def occupancy(lp, labels, blank):
    """(occ [T, C], ll): the posterior probability of emitting class c at frame t."""
    T, C = lp.shape
    alpha, beta, ll = ctc_alpha_beta(lp, labels, blank)
    occ = np.zeros((T, C))
    if ll == NEG_INF:
        return occ, ll
    ext = np.full(2 * len(labels) + 1, blank, dtype=np.int64)
    ext[1::2] = labels
    with np.errstate(invalid='ignore'):
        post = np.exp(alpha + beta - lp[:, ext] - ll)   # [T, S]; -inf + -inf stays -inf, exp gives 0
    post = np.nan_to_num(post, nan=0.0)
    for s, c in enumerate(ext):
        occ[:, c] += post[:, s]
    return occ, ll


def weights(ll, errs):
    """(p, ebar, loss, w) from the log-probabilities and integer errors of one list."""
    ll = np.asarray(ll, dtype=np.float64)
    e = np.asarray(errs, dtype=np.float64)
    n = len(ll)
    p = np.zeros(n)
    if n == 0 or not np.isfinite(ll).any():
        return p, (float(e.mean()) if n else 0.0), 0.0, np.zeros(n)
    m = ll.max()
    z = np.exp(ll - m)
    p = z / z.sum()
    ebar = e.sum() / n
    d = (n * e - e.sum()) / n
    loss = float((p * d).sum())
    return p, float(ebar), loss, p * (d - loss)


def mwer(logits, hyps, errs, blank, grad_scale=1.0):
    """One utterance: logits [T, C] (its valid frames only), hyps a list of label lists.
    Returns a dict: ll [n], p [n], ebar, loss, w [n], grad [T, C]."""
    lp = log_softmax(logits)
    occs, ll = [], []
    for y in hyps:
        o, l = occupancy(lp, list(y), blank)
        occs.append(o)
        ll.append(l)
    p, ebar, loss, w = weights(ll, errs)
    grad = np.zeros(lp.shape)
    for wi, o in zip(w, occs):
        if wi != 0.0:
            grad += wi * o
    return {'ll': np.array(ll), 'p': p, 'ebar': ebar, 'loss': loss, 'w': w, 'grad': grad_scale * grad}


def mwer_batch(logits, lens, hyps, errs, blank, grad_scale=1.0):
    """logits [B, Tmax, C], lens [B], hyps[b] a list of n_b label lists, errs[b] its errors.
    Returns per-utterance dicts as ``mwer``, grad padded with zeros to [Tmax, C]."""
    logits = np.asarray(logits, dtype=np.float64)
    out = []
    for b in range(logits.shape[0]):
        T = max(0, min(int(lens[b]), logits.shape[1]))
        r = mwer(logits[b, :T], hyps[b], errs[b], blank, grad_scale)
        g = np.zeros(logits.shape[1:])
        g[:T] = r['grad']
        r['grad'] = g
        out.append(r)
    return out


def torch_mwer(logits, lens, hyps, errs, blank, dtype, grad_scale=1.0):
    """The same loss from torch.nn.functional.ctc_loss and autograd on the CPU in ``dtype``:
    (ll list of [n_b], p list of [n_b], loss [B], grad [B, Tmax, C]) as float64 numpy.
    Infeasible hypotheses: ctc_loss returns +inf, i.e. ll = -inf, masked out of the softmax
    as zero_infinity does for the loss.  Utterances with T = 0 or no hypothesis give 0."""
    x = torch.tensor(np.asarray(logits), dtype=dtype, requires_grad=True)
    B, Tmax, C = x.shape
    lls, ps, losses = [], [], []
    total = torch.zeros((), dtype=dtype)
    for b in range(B):
        T = max(0, min(int(lens[b]), Tmax))
        n = len(hyps[b])
        if T == 0 or n == 0:
            lls.append(np.full(n, NEG_INF))
            ps.append(np.zeros(n))
            losses.append(0.0)
            continue
        lp = F.log_softmax(x[b, :T], dim=-1)[:, None, :].expand(T, n, C)
        Lmax = max([len(y) for y in hyps[b]] + [1])
        tgt = torch.tensor([list(y) + [0] * (Lmax - len(y)) for y in hyps[b]], dtype=torch.long)
        tl = torch.tensor([len(y) for y in hyps[b]], dtype=torch.long)
        il = torch.full((n,), T, dtype=torch.long)
        with torch.no_grad():
            ok = torch.isfinite(F.ctc_loss(lp.detach(), tgt, il, tl, blank=blank, reduction='none'))
        # zero_infinity: an infeasible row gets loss 0 and a zero gradient (not inf and nan)
        nll = F.ctc_loss(lp, tgt, il, tl, blank=blank, reduction='none', zero_infinity=True)
        if not bool(ok.any()):
            lls.append(np.full(n, NEG_INF))
            ps.append(np.zeros(n))
            losses.append(0.0)
            continue
        ll = torch.where(ok, -nll, torch.full_like(nll, NEG_INF))
        p = torch.softmax(ll, dim=0)
        e = torch.tensor(errs[b], dtype=dtype)
        d = (n * e - e.sum()) / n
        loss = (p * d).sum()
        total = total + loss
        lls.append(ll.detach().double().numpy())
        ps.append(p.detach().double().numpy())
        losses.append(float(loss.detach().double()))
    if not total.requires_grad:
        return lls, ps, np.array(losses), np.zeros(tuple(x.shape))
    (total * grad_scale).backward()
    return lls, ps, np.array(losses), x.grad.double().numpy()


# ---- inputs of tests/test_mwer_gpu.py ------------------------------------------------
# (B, N, T, C, Lmax, lo, hi, scale, seed): N hypotheses of lo .. hi labels per utterance
# (edits of one random row, so that their probabilities are comparable; lo = hi: only
# substitutions, every row has exactly that many labels), logits of the given scale.
# mwer.hip chooses a hypothesis's recursion by its own S = 2 L + 1: <= 128, <= 256, <= 512
# (wave-resident, 2 / 4 / 8 states per lane) and > 512 (the block loop).  One case per
# class, one on either side of each boundary, and N = 32.
KERNEL_CASES = [
    (3, 4, 12, 6, 12, 2, 6, 1.0, 0),            # the smallest class
    (2, 3, 40, 33, 40, 33, 38, 1.0, 3),         # S = 67 .. 77: states cross a 64-lane group
    (2, 2, 80, 8, 80, 66, 72, 0.5, 33),          # S = 133 .. 145: the second class
    (1, 2, 140, 5, 140, 130, 136, 0.5, 1),      # S = 261 .. 273: the third class
    (1, 2, 260, 4, 260, 256, 256, 0.5, 1),      # S = 513: the block loop
    (2, 32, 10, 5, 10, 2, 5, 1.0, 0),           # N = 32
    (1, 2, 70, 4, 64, 63, 63, 0.5, 0),          # S = 127, the last of the first class
    (1, 2, 70, 4, 64, 64, 64, 0.5, 0),          # S = 129, the first of the second
    (1, 2, 134, 4, 128, 127, 127, 0.5, 3),      # S = 255
    (1, 2, 134, 4, 128, 128, 128, 0.5, 2),      # S = 257
    (1, 2, 262, 4, 256, 255, 255, 0.5, 1),      # S = 511
    (1, 2, 262, 4, 256, 256, 256, 0.5, 1),      # S = 513
]
POISON_LABEL = 0x7f7f7f7f


def _repeats(y):
    return sum(1 for a, b in zip(y, y[1:]) if a == b)


def kernel_case(index):
    """The inputs of KERNEL_CASES[index], a dict: logits [B, T, C] float32 (NaN past an
    utterance's length), lens [B], hyps[b] the list of N label lists, errs[b] their errors
    (0 .. 6), blank = C - 1.  Lengths are ragged (utterance 0 is full, the others shorter),
    every hypothesis is feasible, rows hold repeated labels where the frames allow, and
    hypothesis N - 1 of utterance 0 is empty when N >= 3."""
    B, N, T, C, Lmax, lo, hi, scale, seed = KERNEL_CASES[index]
    rng = np.random.default_rng(9000 + 100 * index + seed)
    blank = C - 1
    logits = (rng.standard_normal((B, T, C)) * scale).astype(np.float32)
    lens, hyps, errs = [], [], []
    for b in range(B):
        Tb = T if b == 0 else T - int(rng.integers(1, max(2, T // 8)))
        hi_b = min(hi, Tb - 2)
        lens.append(Tb)
        logits[b, Tb:] = np.nan
        base = rng.integers(0, blank, size=int(rng.integers(min(lo, hi_b), hi_b + 1))).tolist()
        rows = []
        for i in range(N):
            y = list(base)
            for _ in range(int(rng.integers(1, 4)) if i else 0):
                k = int(rng.integers(0, len(y)))
                kind = int(rng.integers(0, 3)) if lo < hi else 0
                if kind == 0:
                    y[k] = int(rng.integers(0, blank))
                elif kind == 1 and len(y) > 1:
                    del y[k]
                elif len(y) < min(Lmax, hi_b):
                    y.insert(k, y[k])             # a repeated label
            # keep it feasible: a repeat needs a blank between, i.e. one more frame
            k = 1
            while len(y) + _repeats(y) > Tb and k < len(y):
                if y[k] == y[k - 1]:
                    y[k] = (y[k] + 1) % blank if blank > 1 else y[k]
                k += 1
            assert len(y) <= Lmax and len(y) + _repeats(y) <= Tb, (index, b, i)
            rows.append(y)
        if b == 0 and N >= 3:
            rows[N - 1] = []
        hyps.append(rows)
        e = rng.integers(0, 7, size=N).tolist()
        while len(set(e)) < 2:   # equal errors are the exact-zero case, tested on its own
            e = rng.integers(0, 7, size=N).tolist()
        errs.append(e)
    return {'logits': logits, 'lens': lens, 'hyps': hyps, 'errs': errs, 'blank': blank, 'Lmax': Lmax}


def dense_hyps(hyps, N, Lmax):
    """(hyp [B, N, Lmax] int32 with POISON_LABEL past each length, hyp_len [B, N], n_hyp [B])."""
    B = len(hyps)
    hyp = np.full((B, N, Lmax), POISON_LABEL, dtype=np.int32)
    hyp_len = np.zeros((B, N), dtype=np.int32)
    for b, rows in enumerate(hyps):
        for i, y in enumerate(rows):
            hyp[b, i, :len(y)] = y
            hyp_len[b, i] = len(y)
    return hyp, hyp_len, np.array([len(r) for r in hyps], dtype=np.int32)


def measure_fp32_error():
    """Largest absolute error of the float32 CPU evaluation (torch_mwer) against the
    float64 restatement (mwer_batch) over all of KERNEL_CASES, per quantity: the figures
    from which tests/test_mwer_gpu.py's tolerances come (4 x each)."""
    worst = {'ll_rel': 0.0, 'p': 0.0, 'loss': 0.0, 'grad': 0.0, 'min_second_p': 1.0}
    for k in range(len(KERNEL_CASES)):
        c = kernel_case(k)
        want = mwer_batch(c['logits'], c['lens'], c['hyps'], c['errs'], c['blank'])
        lls, ps, loss, grad = torch_mwer(c['logits'], c['lens'], c['hyps'], c['errs'], c['blank'], torch.float32)
        for b, r in enumerate(want):
            worst['ll_rel'] = max(worst['ll_rel'], float(np.max(np.abs(lls[b] - r['ll']) / (1 + np.abs(r['ll'])))))
            worst['p'] = max(worst['p'], float(np.abs(ps[b] - r['p']).max()))
            worst['loss'] = max(worst['loss'], abs(float(loss[b]) - r['loss']))
            worst['grad'] = max(worst['grad'], float(np.abs(grad[b] - r['grad']).max()))
            worst['min_second_p'] = min(worst['min_second_p'], float(np.sort(r['p'])[-2]))
    return worst


def beam_nbest(logits, blank, beam_width):
    """The whole beam after the last frame of logits [T, C], in rank order, as a list of
    (prefix tuple, total log probability): the algorithm of tests/beam_ref.py (ties by
    first creation; keys as the device kernel states them), restated to return every entry."""
    x = np.asarray(logits, dtype=np.float64)
    T, C = x.shape
    lse = np.logaddexp
    rank = np.cumsum(np.arange(C) != blank)
    prefixes, pb, pnb = [()], np.array([0.0]), np.array([NEG_INF])
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
        ext = prev + lp[None, :]
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
        ks, cs = np.nonzero(made)
        totals = np.concatenate([lse(npb, npnb), ext[ks, cs]])
        keys = np.concatenate([own_key, ext_key[ks, cs]])
        order = np.lexsort((keys, -totals))[:beam_width]
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
    tots = lse(pb, pnb)
    return [(tuple(p), float(v)) for p, v in zip(prefixes, tots)]
