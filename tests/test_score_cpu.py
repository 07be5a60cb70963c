"""The scoring reference (tests/score_ref.py) pinned on the host, the conditions its case
list must meet for tests/test_score_gpu.py to mean something, the label fold, and the
argument checks of srf_edit_align and its wrappers.  Needs no GPU.  Each test prints its
figures before it asserts."""
import ctypes
import json
import os

import pytest
import torch

from tests import score_ref as sr

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def test_worked_examples():
    a = sr.align([1, 2, 3], [1, 3])
    assert a['counts'] == [1, 0, 0, 1, 2, 3] and a['ops'] == [('cor', 0, 0), ('ins', 1, -1), ('cor', 2, 1)]
    a = sr.align([1, 2], [2, 1])
    assert a['counts'] == [2, 2, 0, 0, 2, 2] and [o[0] for o in a['ops']] == ['sub', 'sub']
    a = sr.align([1, 1, 2], [1, 2])
    assert a['counts'] == [1, 0, 0, 1, 2, 3] and a['hyp_to_ref'] == [-1, 0, 1] and a['ops'][0] == ('ins', 0, -1)
    a = sr.align([1, 2], [1, 1, 2])
    assert a['counts'] == [1, 0, 1, 0, 3, 2] and a['ref_to_hyp'] == [-1, 0, 1] and a['ops'][0] == ('del', -1, 0)
    a = sr.align([], [4, 5])
    assert a['counts'] == [2, 0, 2, 0, 2, 0] and a['ref_to_hyp'] == [-1, -1] and a['hyp_to_ref'] == []
    assert sr.align([], [])['counts'] == [0] * 6


def test_fold_and_padding_in_the_reference():
    fold = [0, -1, 1, 1]
    a = sr.align([0, 1, 3, 9, -4], [0, 2, 1], fold, hmax=7, rmax=4)
    assert a['counts'] == [0, 0, 0, 0, 2, 2]
    assert a['hyp_to_ref'] == [0, -2, 1, -2, -2, -2, -2] and a['ref_to_hyp'] == [0, 2, -2, -2]
    assert a['ops'] == [('cor', 0, 0), ('cor', 2, 1)]
    assert sr.align([1, 1], [1], [-1, -1])['counts'] == [0] * 6


def _check_invariants(res, hyp, ref):
    d, s, dl, ins, R, H = res['counts']
    cor = sum(1 for o in res['ops'] if o[0] == 'cor')
    assert s + dl + ins == d
    assert cor + s + dl == R and cor + s + ins == H
    assert d == sr.distance_two_rows(hyp, ref)
    h2r, r2h = res['hyp_to_ref'], res['ref_to_hyp']
    for i, j in enumerate(h2r):
        if j >= 0:
            assert r2h[j] == i
    for j, i in enumerate(r2h):
        if i >= 0:
            assert h2r[i] == j
    for m in (h2r, r2h):
        pos = [v for v in m if v >= 0]
        assert all(x < y for x, y in zip(pos[:-1], pos[1:]))


@pytest.mark.parametrize('H,R', sr.SHAPES)
def test_invariants_on_every_case(H, R):
    for A in sr.ALPHABETS:
        hyp, hyp_len, ref, ref_len, results = sr.reference(H, R, A)
        assert hyp_len[0] == H and ref_len[0] == R and hyp_len[1] == 0 and ref_len[1] == 0
        for b, res in enumerate(results):
            _check_invariants(res, list(hyp[b][:hyp_len[b]]), list(ref[b][:ref_len[b]]))
        print(f'(H, R) = {(H, R)} A = {A}: distances {[r["counts"][0] for r in results]}')


def test_small_alphabet_cases_test_the_tie_rule():
    """A condition on the inputs: under the opposite preference (insertion, deletion,
    diagonal) at least 5 % of the A = 4 utterances give different (S, D, I)."""
    n = differ = 0
    for H, R in sr.SHAPES:
        hyp, hyp_len, ref, ref_len, results = sr.reference(H, R, 4)
        for b, res in enumerate(results):
            h, r = list(hyp[b][:hyp_len[b]]), list(ref[b][:ref_len[b]])
            if not h or not r:
                continue
            n += 1
            other = sr.sdi(h, r, sr.INS_DEL_DIAG)
            assert sum(other) == res['counts'][0]   # another optimal path, the same distance
            differ += tuple(res['counts'][1:4]) != other
    print(f'{differ} of {n} A = 4 utterances change (S, D, I) under the opposite preference')
    assert differ >= 0.05 * n


def _fixture():
    with open(os.path.join(GOLD, 'timit_fold.json')) as fh:
        return json.load(fh)


def test_fold_table_on_the_timit_fixture():
    from srf_amd import scoring
    fx = _fixture()
    vocab, mapping = fx['vocab'], fx['fold']
    assert len(vocab) == 62 and len(mapping) == 61
    table, names = scoring.fold_table(vocab, mapping, device='cpu')
    assert table.dtype == torch.int32 and table.dim() == 1
    table = table.tolist()
    assert len(names) == 39 and len(table) == 62
    assert sorted(set(t for t in table if t >= 0)) == list(range(39))
    assert table[vocab.index('q')] == -1
    assert table[0] == -1 and vocab[0] not in mapping          # the padding symbol
    assert table[vocab.index('ao')] == table[vocab.index('aa')] == names.index('aa')
    assert names[0] == 'aa' and names[table[vocab.index('bcl')]] == 'sil'
    assert all(names[table[i]] == mapping[v] for i, v in enumerate(vocab) if table[i] >= 0)
    # numbered by first appearance in vocab order
    firsts = [table[i] for i in range(62) if table[i] >= 0 and table[i] not in table[:i]]
    assert firsts == list(range(39))


def test_signatures_hold_both_names():
    from srf_amd import _lib
    assert 'srf_edit_align' in _lib._SIGNATURES and 'srf_edit_align_workspace' in _lib._SIGNATURES
    assert len(_lib._SIGNATURES['srf_edit_align'][1]) == 18


def test_entry_points_refuse_bad_arguments_without_gpu():
    from srf_amd import _lib
    L = _lib.lib()
    assert L.srf_edit_align_workspace(1, 0, 0) >= 16
    assert L.srf_edit_align_workspace(28, 200, 200) >= 16
    assert L.srf_edit_align_workspace(2, 600, 700) >= 2 * 150 * 700
    assert L.srf_edit_align_workspace(1, 8192, 8192) >= 2048 * 8192
    fake = ctypes.c_void_p(4096)   # never dereferenced: every call below is refused before a launch
    for B, H, R in ((0, 4, 4), (-1, 4, 4), (1, -1, 4), (1, 4, -1), (1, 8193, 4), (1, 4, 8193)):
        assert L.srf_edit_align_workspace(B, H, R) == 0, (B, H, R)
        assert b'bad shape' in L.srf_last_error()
        assert L.srf_edit_align(fake, fake, H, fake, fake, R, B, None, 0, fake, None, None, None, None, 0, fake, 1 << 30,
                                None) == -1, (B, H, R)
        assert b'bad shape' in L.srf_last_error()

    def call(hyp=fake, hyp_len=fake, ref=fake, ref_len=fake, fold=None, n_fold=0, counts=fake, confusion=None, K=0,
             ws=fake, wb=1 << 30):
        return L.srf_edit_align(hyp, hyp_len, 4, ref, ref_len, 4, 1, fold, n_fold, counts, None, None, None, confusion,
                                K, ws, wb, None)
    for kw in (dict(hyp=None), dict(hyp_len=None), dict(ref=None), dict(ref_len=None), dict(counts=None),
               dict(ws=None)):
        assert call(**kw) == -1, kw
        assert b'null' in L.srf_last_error(), (kw, L.srf_last_error())
    assert call(n_fold=3) == -1 and b'n_fold' in L.srf_last_error()
    assert call(fold=fake, n_fold=-1) == -1 and b'n_fold' in L.srf_last_error()
    assert call(confusion=fake, K=0) == -1 and b'K = 0' in L.srf_last_error()
    assert call(ws=ctypes.c_void_p(4100)) == -1 and b'aligned' in L.srf_last_error()
    assert call(wb=8) == -4 and b'workspace too small' in L.srf_last_error()


def test_wrappers_refuse_host_tensors_and_shape_mismatches():
    from srf_amd import scoring
    hyp = torch.zeros((2, 3), dtype=torch.int32)
    with pytest.raises(ValueError, match='device tensor'):
        scoring.edit_align(hyp, [3, 3], [[0], [1]], None)
    with pytest.raises(ValueError, match='device tensor'):
        scoring.edit_align([[0], [1]], None, hyp, torch.tensor([3, 3]))
    with pytest.raises(ValueError, match='without lengths'):
        scoring.edit_align([[0], [1]], [1, 1], [[0], [1]], None)
    with pytest.raises(ValueError, match='expected 2'):
        scoring.edit_align([[0], [1]], None, [[0]], None)
    with pytest.raises(ValueError, match='holds 0 utterances'):
        scoring.edit_align([], None, [], None)
    with pytest.raises(ValueError, match='takes 8192'):
        scoring.edit_align([[0] * 8193], None, [[0]], None)
    er = scoring.ErrorRate(device='cpu')
    with pytest.raises(ValueError, match='device tensor'):
        er.update_state(hyp, torch.tensor([3, 3]), hyp, torch.tensor([3, 3]))
    with pytest.raises(ValueError, match='HIP device'):
        er.update_state([[0]], None, [[0]], None)
    with pytest.raises(ValueError, match='n_classes'):
        scoring.ErrorRate(n_classes=-1, device='cpu')
    with pytest.raises(ValueError, match='n_classes'):
        er.confusion()
    with pytest.raises(ValueError, match='fold'):
        scoring.ErrorRate(fold=[[0, 1]], device='cpu')
    assert er.result() == sr.error_rate([0] * 8)
    er.reduce()   # no process group: nothing happens
    if torch.cuda.is_available():
        dev = torch.device('cuda:0')
        with pytest.raises(ValueError, match='lengths'):
            scoring.edit_align(hyp.to(dev), None, [[0], [1]], None)
        with pytest.raises(ValueError, match='shape'):
            scoring.edit_align(hyp.to(dev), [3, 3, 3], [[0], [1]], None)
        with pytest.raises(ValueError, match='expected 2'):
            scoring.edit_align(hyp.to(dev), [3, 3], [[0]], None)
        with pytest.raises(ValueError, match='device tensor'):
            scoring.edit_align(hyp.to(dev)[0], [3], [[0]], None)


def test_ops_view_refuses_host_tensors():
    from srf_amd import ops
    z = torch.zeros((1, 2), dtype=torch.int32)
    n = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError, match='int32 device tensor'):
        ops.edit_align(z, n, z, n)
    with pytest.raises(ValueError, match=r'\[B, Hmax\]'):
        ops.edit_align(z[0], n, z, n)
