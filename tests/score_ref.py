"""Plain-Python restatement of srf_edit_align's definition (include/srf.h): fold, distance
table, backtrace with the tie rule (diagonal, then deletion, then insertion), the two
position maps, the totals and the confusion matrix; and the case generator of the scoring
tests: a reference drawn from an alphabet of A labels, a hypothesis that is the reference
with random deletions, substitutions and insertions."""
import numpy as np

DIAG_DEL_INS = ('diag', 'del', 'ins')   # the definition's preference
INS_DEL_DIAG = ('ins', 'del', 'diag')   # the opposite one, for the tie-rule condition on the cases


def fold_seq(seq, fold):
    """(folded labels, original positions) of the labels the fold keeps."""
    lab, pos = [], []
    for p, x in enumerate(seq):
        x = int(x)
        if fold is not None:
            if not 0 <= x < len(fold) or fold[x] < 0:
                continue
            x = int(fold[x])
        lab.append(x)
        pos.append(p)
    return lab, pos


def table(h, r):
    H, R = len(h), len(r)
    D = [[0] * (R + 1) for _ in range(H + 1)]
    for i in range(H + 1):
        D[i][0] = i
    for j in range(R + 1):
        D[0][j] = j
    for i in range(1, H + 1):
        for j in range(1, R + 1):
            D[i][j] = min(D[i - 1][j - 1] + (h[i - 1] != r[j - 1]), D[i][j - 1] + 1, D[i - 1][j] + 1)
    return D


def distance_two_rows(h, r):
    """The distance alone, by an independent two-row sweep without a backtrace."""
    prev = list(range(len(r) + 1))
    for i in range(1, len(h) + 1):
        cur = [i] + [0] * len(r)
        for j in range(1, len(r) + 1):
            cur[j] = min(prev[j - 1] + (h[i - 1] != r[j - 1]), cur[j - 1] + 1, prev[j] + 1)
        prev = cur
    return prev[len(r)]


def backtrace(h, r, D, prefer=DIAG_DEL_INS):
    """From (H, R), the first step of ``prefer`` that is consistent with D.  Returns the
    steps in forward order: ('diag', i, j) pairs h[i] with r[j], ('del', -1, j), ('ins', i, -1)."""
    i, j, steps = len(h), len(r), []
    while i > 0 or j > 0:
        ok = {'diag': i > 0 and j > 0 and D[i][j] == D[i - 1][j - 1] + (h[i - 1] != r[j - 1]),
              'del': j > 0 and D[i][j] == D[i][j - 1] + 1,
              'ins': i > 0 and D[i][j] == D[i - 1][j] + 1}
        step = next(s for s in prefer if ok[s])
        if step == 'diag':
            i, j = i - 1, j - 1
            steps.append(('diag', i, j))
        elif step == 'del':
            j -= 1
            steps.append(('del', -1, j))
        else:
            i -= 1
            steps.append(('ins', i, -1))
    return steps[::-1]


def sdi(h, r, prefer=DIAG_DEL_INS):
    """(substitutions, deletions, insertions) of the backtrace under ``prefer``."""
    steps = backtrace(h, r, table(h, r), prefer)
    return (sum(1 for s, i, j in steps if s == 'diag' and h[i] != r[j]), sum(1 for s, _, _ in steps if s == 'del'),
            sum(1 for s, _, _ in steps if s == 'ins'))


def align(hyp, ref, fold=None, hmax=None, rmax=None):
    """One utterance: dict with counts [6], hyp_to_ref [hmax], ref_to_hyp [rmax] (positions
    before the fold, -1 inserted / deleted, -2 dropped or past the length), ops (kind,
    hyp position, ref position) and pairs (reference class, hypothesis class; None for the
    side a deletion / an insertion lacks)."""
    hmax = len(hyp) if hmax is None else hmax
    rmax = len(ref) if rmax is None else rmax
    h, hpos = fold_seq(hyp, fold)
    r, rpos = fold_seq(ref, fold)
    D = table(h, r)
    h2r, r2h = [-2] * hmax, [-2] * rmax
    ops, pairs, n_sub, n_del, n_ins = [], [], 0, 0, 0
    for s, i, j in backtrace(h, r, D):
        if s == 'diag':
            h2r[hpos[i]], r2h[rpos[j]] = rpos[j], hpos[i]
            n_sub += h[i] != r[j]
            ops.append(('cor' if h[i] == r[j] else 'sub', hpos[i], rpos[j]))
            pairs.append((r[j], h[i]))
        elif s == 'del':
            r2h[rpos[j]] = -1
            n_del += 1
            ops.append(('del', -1, rpos[j]))
            pairs.append((r[j], None))
        else:
            h2r[hpos[i]] = -1
            n_ins += 1
            ops.append(('ins', hpos[i], -1))
            pairs.append((None, h[i]))
    return {'counts': [D[len(h)][len(r)], n_sub, n_del, n_ins, len(r), len(h)], 'hyp_to_ref': h2r, 'ref_to_hyp': r2h,
            'ops': ops, 'pairs': pairs}


def align_batch(hyp, hyp_len, ref, ref_len, fold=None):
    """Dense [B][max] rows with lengths (clamped as the kernel clamps them)."""
    hmax = len(hyp[0]) if len(hyp) else 0
    rmax = len(ref[0]) if len(ref) else 0
    out = []
    for b in range(len(hyp)):
        nh, nr = max(0, min(int(hyp_len[b]), hmax)), max(0, min(int(ref_len[b]), rmax))
        out.append(align(list(hyp[b][:nh]), list(ref[b][:nr]), fold, hmax, rmax))
    return out


def totals(results):
    t = [0] * 8
    for res in results:
        for q in range(6):
            t[q] += res['counts'][q]
        t[6] += 1
        t[7] += res['counts'][0] > 0
    return t


def confusion(results, K):
    """[K + 1][K + 1]: row the reference class, column the hypothesis class, column K the
    deletions, row K the insertions; a pair with a class outside [0, K) is left out."""
    M = np.zeros((K + 1, K + 1), dtype=np.int64)
    for res in results:
        for rc, hc in res['pairs']:
            if (rc is not None and not 0 <= rc < K) or (hc is not None and not 0 <= hc < K):
                continue
            M[K if rc is None else rc, K if hc is None else hc] += 1
    return M


def error_rate(t):
    return {'substitutions': t[1], 'deletions': t[2], 'insertions': t[3], 'reference_labels': t[4],
            'hypothesis_labels': t[5], 'utterances': t[6], 'error_rate': (t[1] + t[2] + t[3]) / t[4] if t[4] else 0.0,
            'utterance_error_rate': t[7] / t[6] if t[6] else 0.0}


def case(seed, H, R, A, edits=0.10):
    """(hyp, ref): a reference of R labels from [0, A) and the reference with random
    deletions, substitutions and insertions (``edits`` of the positions each way), cut or
    filled with random labels to exactly H labels."""
    rng = np.random.default_rng(7000 + seed)
    ref = [int(v) for v in rng.integers(0, A, R)]
    hyp = []
    for x in ref:
        u = rng.random()
        if u < edits / 3:
            continue                                   # deletion
        if u < 2 * edits / 3:
            x = int(rng.integers(0, A))                # substitution (may draw the same label)
        hyp.append(x)
        if rng.random() < edits / 3:
            hyp.append(int(rng.integers(0, A)))        # insertion
    hyp = hyp[:H] + [int(v) for v in rng.integers(0, A, max(0, H - len(hyp)))]
    return hyp, ref


# (H, R) capacities of the device tests: empty and tiny sequences; the flush of the 16-step
# history word; the 64-lane boundary feed; the size-class switch; the workload's size;
# back-pointers spilling to the workspace; the workgroup-loop fallback.
SHAPES = [(0, 0), (0, 5), (5, 0), (1, 1), (7, 9), (15, 17), (16, 16), (17, 15), (63, 64), (64, 65), (65, 63),
          (128, 129), (129, 128), (256, 257), (200, 200), (300, 512), (512, 300), (40, 513), (513, 40), (600, 700)]
ALPHABETS = (4, 62)
_REFERENCE = {}


def reference(H, R, A):
    """The ragged batch of a shape and alphabet with its alignments, computed once per
    process and shared: (hyp, hyp_len, ref, ref_len, results).  Callers leave it unchanged."""
    key = (H, R, A)
    if key not in _REFERENCE:
        hyp, hyp_len, ref, ref_len = ragged_batch(SHAPES.index((H, R)), H, R, A)
        _REFERENCE[key] = (hyp, hyp_len, ref, ref_len, align_batch(hyp, hyp_len, ref, ref_len))
    return _REFERENCE[key]


def ragged_batch(seed, H, R, A, B=8):
    """B utterances in dense rows [B][H] / [B][R]: utterance 0 at the maximum (H, R),
    utterance 1 of length 0 on both sides, the others ragged; the padding is poison
    (-7 in the hypotheses, 10^9 in the references).  Returns (hyp, hyp_len, ref, ref_len)."""
    rng = np.random.default_rng(9000 + seed)
    hyp = np.full((B, H), -7, dtype=np.int64)
    ref = np.full((B, R), 10 ** 9, dtype=np.int64)
    hyp_len, ref_len = [], []
    for b in range(B):
        nh, nr = (H, R) if b == 0 else (0, 0) if b == 1 else (int(rng.integers(0, H + 1)), int(rng.integers(0, R + 1)))
        if b >= 4 and R > 0 and H > 0:   # near-diagonal pairs, as a hypothesis of its reference is
            nr = min(R, max(0, nh + int(rng.integers(-2, 3))))
        h, r = case(1000 * seed + b, nh, nr, A)
        hyp[b, :nh], ref[b, :nr] = h, r
        hyp_len.append(nh)
        ref_len.append(nr)
    return hyp, hyp_len, ref, ref_len
