"""The host side of chunked streaming inference that needs no GPU
(srf_amd/streaming.py): the schedule arithmetic -- how many output frames of each stage
are final after a push -- and the validation of ``ended``."""
import pytest

from srf_amd import streaming

SHAPES = [(1, 0), (2, 2), (3, 4), (6, 2)]   # (routing layers, rpad)
PATTERNS = [[96], [12] * 8, [4] * 24, [4, 20, 8, 4, 36, 24], [64, 4, 4, 64, 32]]


@pytest.mark.parametrize('L,rpad', SHAPES)
@pytest.mark.parametrize('pushes', PATTERNS, ids=lambda p: '-'.join(map(str, p[:6])))
def test_schedule_emits_all_but_the_lookahead(L, rpad, pushes):
    """After pushes totalling P input frames, max(0, P/4 - 2 - L*rpad) output frames are
    emitted; every stage lags the one below by its own lookahead and never runs ahead of
    it; finish() completes every stage at T/4."""
    rows = streaming.stream_schedule(pushes, L, rpad)
    assert len(rows) == len(pushes) + 1
    total, prev = 0, [0] * (L + 2)
    for n, row in zip(pushes, rows):
        total += n
        assert len(row) == L + 2
        assert row[-1] == max(0, total // 4 - 2 - L * rpad)
        assert row[0] == max(0, total // 4 - 1)        # CNN-FE: inputs 4o .. 4o + 6
        assert row[1] == max(0, total // 4 - 2)        # primary capsules: CNN-FE frame o + 1
        for l in range(L):
            assert row[l + 2] == max(0, row[l + 1] - rpad)
        assert all(a >= b for a, b in zip(row, prev))  # final frames stay final
        assert all(a - b <= n // 4 for a, b in zip(row, prev))
        prev = row
    assert rows[-1] == [total // 4] * (L + 2)
    assert all(a - b <= 2 + L * rpad for a, b in zip(rows[-1], prev))   # what finish() still owes


def test_schedule_refuses_partial_output_frames():
    with pytest.raises(ValueError):
        streaming.frames_final(10, 2, 2)
    assert streaming.frames_final(0, 2, 2) == [0, 0, 0, 0]
    assert streaming.frames_final(0, 2, 2, finished=True) == [0, 0, 0, 0]


def test_ended_validation():
    """A length is declared once, with the chunk it lies in: P_before <= len <=
    P_before + n.  Later raises (frames were emitted unmasked), so does a repeat."""
    lens = [None, None, None]
    lens = streaming.check_ended(lens, None, 0, 12)
    assert lens == [None, None, None]
    lens = streaming.check_ended(lens, [-1, 12, -1], 0, 12)        # the chunk's last frame ends it
    assert lens == [None, 12, None]
    lens = streaming.check_ended(lens, [12, -1, -1], 12, 12)       # ends exactly at the chunk's start
    assert lens == [12, 12, None]
    with pytest.raises(ValueError, match='already declared'):     # repeated, even with the same value
        streaming.check_ended(lens, [-1, 12, -1], 12, 12)
    with pytest.raises(ValueError, match='before this chunk'):    # late: its end lay in an earlier chunk
        streaming.check_ended(lens, [-1, -1, 11], 12, 12)
    with pytest.raises(ValueError, match='beyond this chunk'):
        streaming.check_ended(lens, [-1, -1, 25], 12, 12)
    with pytest.raises(ValueError, match='length or -1'):
        streaming.check_ended(lens, [-1, -1, -2], 12, 12)
    with pytest.raises(ValueError, match='entries'):
        streaming.check_ended(lens, [-1, -1], 12, 12)
    assert lens == [12, 12, None]                                  # a refused call changes nothing
    assert streaming.check_ended(lens, [-1, -1, 24], 12, 12) == [12, 12, 24]
