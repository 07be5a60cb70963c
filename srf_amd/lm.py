"""Language models for shallow fusion in the CTC prefix beam search.

The beam search takes a deterministic automaton over the classes as two tables,
``bonus [S][C]`` (what extending a prefix in state s by class c adds to its score) and
``next [S][C]`` (the state after it); state 0 belongs to the empty prefix.  This module
builds them on the host, in numpy:

  * ``NGramLM.from_arpa`` reads a backoff n-gram from an ARPA file,
  * ``NGramLM.from_sequences`` estimates one from label sequences (interpolated
    Witten-Bell), so that a model can be made from the training transcripts alone,
  * ``lm.automaton()`` unfolds the backoff structure into ``(logp, next)``,
  * ``lm.fuse(alpha, beta, blank, device)`` gives the ``FusedLM`` that
    ``ctc.BeamState``, ``StreamingRouter`` and ``process_test_step`` take:
    ``bonus = alpha * logp + beta`` with the blank's column 0,
  * ``FusedLM.from_tables`` wraps any automaton.

Contexts are tuples of class indices, oldest first; ``BOS`` (-1) stands for the start of
the utterance and occurs only at the front of a context.
"""
import math
import os

import numpy as np

BOS = -1
_LN10 = math.log(10.0)


class FusedLM:
    """The tables of a fused language model: ``bonus`` [S, C] float32 and ``next`` [S, C]
    int32 on ``device``, their host copies ``bonus_host`` / ``next_host`` (numpy, for the
    host decoder), ``n_states``, ``n_classes`` and ``blank``."""

    def __init__(self, bonus, next_state, blank, device):
        import torch
        self.bonus_host, self.next_host = bonus, next_state
        self.n_states, self.n_classes = bonus.shape
        self.blank = int(blank)
        self.bonus = torch.from_numpy(bonus).to(device)
        self.next = torch.from_numpy(next_state).to(device)

    @classmethod
    def from_tables(cls, bonus, next, blank, device='cuda'):
        """Any automaton.  Checked on the host: both tables [S, C] with S >= 1, C >= 2 and
        S * C < 2^31, 0 <= blank < C, every bonus finite, every next in [0, S).
        ValueError otherwise, before anything reaches a kernel.  The blank's column of
        ``bonus`` is stored as 0."""
        bonus, nxt = np.asarray(bonus), np.asarray(next)
        if bonus.ndim != 2 or nxt.shape != bonus.shape:
            raise ValueError(f'bonus and next must both be [n_states, n_classes], got {bonus.shape} and {nxt.shape}')
        S, C = bonus.shape
        if S < 1 or C < 2 or S * C >= 2 ** 31:
            raise ValueError(f'need n_states >= 1, n_classes >= 2 and n_states * n_classes < 2^31, got {S} x {C}')
        if not 0 <= int(blank) < C:
            raise ValueError(f'blank index {blank} outside [0, {C})')
        if not np.issubdtype(nxt.dtype, np.integer):
            raise ValueError(f'next must hold integers, got {nxt.dtype}')
        with np.errstate(over='ignore'):   # a value too large for float32 becomes inf and is refused below
            bonus = np.array(bonus, dtype=np.float32)   # a copy
        bonus[:, int(blank)] = 0.0
        if not np.isfinite(bonus).all():
            raise ValueError('the bonus table holds a value that is not finite (as float32)')
        if nxt.min() < 0 or nxt.max() >= S:
            raise ValueError(f'next holds a state outside [0, {S})')
        return cls(np.ascontiguousarray(bonus), np.ascontiguousarray(nxt, dtype=np.int32), blank, device)

    def sequence_bonus(self, labels):
        """The sum of the bonuses of ``labels`` from state 0, added in label order in
        float32 as the decoders add them."""
        s, acc = 0, np.float32(0.0)
        for c in labels:
            acc = np.float32(acc + self.bonus_host[s, c])
            s = int(self.next_host[s, c])
        return float(acc)


class NGramLM:
    """A backoff n-gram over class indices: ``probs`` maps an n-gram (a tuple, the
    predicted class last) to its natural-log probability, ``backoffs`` a context to its
    natural-log backoff weight (0 where absent).  log p(c | h) is probs[h + (c,)] if
    listed, else backoffs[h] + log p(c | h[1:]); a class without a unigram scores
    ``missing_logp``."""

    def __init__(self, order, n_classes, probs, backoffs, missing_logp=-30.0):
        if int(order) < 1 or int(n_classes) < 2:
            raise ValueError(f'need order >= 1 and n_classes >= 2, got {order} and {n_classes}')
        self.order, self.n_classes = int(order), int(n_classes)
        self.probs, self.backoffs, self.missing_logp = dict(probs), dict(backoffs), float(missing_logp)
        for gram in self.probs:
            if not 1 <= len(gram) <= self.order or not 0 <= gram[-1] < self.n_classes:
                raise ValueError(f'n-gram {gram} does not fit order {self.order} and {self.n_classes} classes')

    # ------------------------------------------------------------------ sources
    @classmethod
    def from_arpa(cls, path_or_text, symbols, n_classes=None, missing_logp=-30.0):
        """Read an ARPA file (a path, or the text itself).  ``symbols`` maps a token to its
        class index; ``n_classes`` defaults to the largest index + 2 (the blank last).
        The file's log10 values become natural logs.  ``<s>`` gives the start context;
        entries with ``</s>`` or ``<unk>`` (and a ``<s>`` that is predicted) are read and
        ignored; any other unknown token is a ValueError."""
        text = path_or_text
        if '\\data\\' not in text and os.path.exists(text):
            with open(text) as fh:
                text = fh.read()
        if n_classes is None:
            n_classes = max(symbols.values()) + 2
        probs, backoffs, order, n = {}, {}, 0, 0
        for line in text.splitlines():
            line = line.strip()
            if not line or line.startswith('ngram ') or line == '\\data\\':
                continue
            if line == '\\end\\':
                break
            if line.startswith('\\') and line.endswith('-grams:'):
                n = int(line[1:-len('-grams:')])
                order = max(order, n)
                continue
            if n == 0:
                continue   # header text before \data\
            f = line.split()
            if len(f) not in (n + 1, n + 2):
                raise ValueError(f'ARPA line does not hold a {n}-gram: {line!r}')
            tokens = f[1:n + 1]
            if '</s>' in tokens or '<unk>' in tokens or '<s>' in tokens[1:]:
                continue
            try:
                gram = tuple(BOS if tok == '<s>' else int(symbols[tok]) for tok in tokens)
            except KeyError as e:
                raise ValueError(f'ARPA token {e.args[0]!r} is not among the symbols') from None
            if gram[-1] != BOS:
                probs[gram] = float(f[0]) * _LN10
            if len(f) == n + 2:
                backoffs[gram] = float(f[n + 1]) * _LN10
        if order < 1:
            raise ValueError('no n-gram section found: not an ARPA file')
        return cls(order, n_classes, probs, backoffs, missing_logp)

    @classmethod
    def from_sequences(cls, label_lists, order, n_classes, blank, missing_logp=-30.0):
        """Estimate from label sequences with interpolated Witten-Bell smoothing:
        p(c | h) = (n(h, c) + t(h) p(c | h[1:])) / (n(h) + t(h)), t(h) the number of
        distinct classes seen after h, the unigrams interpolated with the uniform
        distribution over the non-blank classes.  Every sequence starts in the context
        (BOS,).  Stored in backoff form (seen n-grams listed, the weight t / (n + t) on
        their context), which is the same distribution: rows over the non-blank classes
        sum to 1."""
        order, n_classes, blank = int(order), int(n_classes), int(blank)
        if not 0 <= blank < n_classes:
            raise ValueError(f'blank index {blank} outside [0, {n_classes})')
        counts = [dict() for _ in range(order)]   # [context length]: context -> {class: count}
        for seq in label_lists:
            seq = [int(c) for c in seq]
            if any(not 0 <= c < n_classes or c == blank for c in seq):
                raise ValueError(f'a label lies outside [0, {n_classes}) or is the blank')
            hist = [BOS] + seq
            for i in range(1, len(hist)):
                for k in range(min(order - 1, i) + 1):
                    ctx = tuple(hist[i - k:i])
                    row = counts[k].setdefault(ctx, {})
                    row[hist[i]] = row.get(hist[i], 0) + 1
        uniform = 1.0 / (n_classes - 1)
        p = {}      # n-gram -> probability, shorter contexts first

        def lower(ctx, c):   # p(c | ctx) for a context of any kind, through the backoff form
            while True:
                if ctx + (c,) in p:
                    return p[ctx + (c,)]
                if not ctx:
                    return uniform   # unreachable: every non-blank unigram is listed
                row = counts[len(ctx)].get(ctx)
                if row:
                    n, t = sum(row.values()), len(row)
                    return t / (n + t) * lower(ctx[1:], c)
                ctx = ctx[1:]

        probs, backoffs = {}, {}
        row = counts[0].get((), {})
        n, t = sum(row.values()), len(row)
        for c in range(n_classes):
            if c != blank:
                p[(c,)] = (row.get(c, 0) + t * uniform) / (n + t) if n else uniform
        for k in range(1, order):
            for ctx, row in counts[k].items():
                n, t = sum(row.values()), len(row)
                for c, cnt in row.items():
                    p[ctx + (c,)] = (cnt + t * lower(ctx[1:], c)) / (n + t)
                backoffs[ctx] = math.log(t / (n + t))
        for gram, v in p.items():
            probs[gram] = math.log(v)
        return cls(order, n_classes, probs, backoffs, missing_logp)

    # ------------------------------------------------------------------ queries
    def logp(self, context, c):
        """log p(c | context) by recursive backoff; the context is cut to order - 1."""
        h = tuple(context)[-(self.order - 1):] if self.order > 1 else ()
        total = 0.0
        while True:
            v = self.probs.get(h + (c,))
            if v is not None:
                return total + v
            if not h:
                return total + self.missing_logp
            total += self.backoffs.get(h, 0.0)
            h = h[1:]

    def contexts(self):
        """The contexts the model lists: every context of a listed n-gram and every listed
        n-gram of length < order (it may carry a backoff weight), and the empty one.
        Any other context scores exactly as its longest suffix among these does."""
        out = {()}
        for gram in self.probs:
            out.add(gram[:-1])
            if len(gram) < self.order:
                out.add(gram)
        for ctx in self.backoffs:
            if len(ctx) < self.order:
                out.add(ctx)
        return out

    def automaton(self):
        """(logp [S, C] float64, next [S, C] int32): the states are the listed contexts,
        state 0 the start (the longest listed suffix of (BOS,)), the others by length and
        then in ascending order.  Row s holds log p(c | context of s) with the backoff
        weights folded in, so a lookup never backs off at decode time; next[s, c] is the
        longest listed suffix of the context extended by c (at most order - 1 long)."""
        listed = self.contexts()

        def reduce(ctx):
            ctx = ctx[-(self.order - 1):] if self.order > 1 else ()
            while ctx not in listed:
                ctx = ctx[1:]
            return ctx

        start = reduce((BOS,))
        states = [start] + sorted(listed - {start}, key=lambda h: (len(h), h))
        index = {h: s for s, h in enumerate(states)}
        C = self.n_classes
        rows = {}

        def row(h):   # log p(. | h) for all classes, from the row of the shorter context
            if h not in rows:
                r = np.full(C, self.missing_logp) if not h else self.backoffs.get(h, 0.0) + row(h[1:])
                r = r.copy()
                rows[h] = r
            return rows[h]

        by_context = {}
        for gram, v in self.probs.items():
            by_context.setdefault(gram[:-1], []).append((gram[-1], v))
        for h in sorted(states, key=len):   # shorter contexts first: the recursion stays shallow
            r = row(h)
            for c, v in by_context.get(h, ()):
                r[c] = v
        logp = np.stack([rows[h] for h in states])
        nxt = np.zeros((len(states), C), np.int32)
        for s, h in enumerate(states):
            for c in range(C):
                nxt[s, c] = index[reduce(h + (c,))]
        return logp, nxt

    def fuse(self, alpha, beta, blank, device='cuda'):
        """The ``FusedLM`` with bonus = alpha * log p_lm + beta (``alpha`` the model's
        weight, ``beta`` the bonus per label, i.e. the length penalty), the blank's
        column 0.  ValueError for a blank outside the classes or a table that is not
        finite."""
        logp, nxt = self.automaton()
        if not 0 <= int(blank) < self.n_classes:
            raise ValueError(f'blank index {blank} outside [0, {self.n_classes})')
        if not (math.isfinite(alpha) and math.isfinite(beta)):
            raise ValueError(f'alpha and beta must be finite, got {alpha} and {beta}')
        return FusedLM.from_tables(float(alpha) * logp + float(beta), nxt, blank, device)
