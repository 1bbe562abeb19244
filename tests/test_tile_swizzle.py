"""The swizzled S_k^{-1} tile layout of the one-shot four-wave kernel (CPU test).

solve_phases.h::tile_at<true> puts element (i, c) of a 32 x 32 tile of doubles at

    i * 32 + (c & 16) + 2 * (((c & 15) >> 1) ^ (i & 7)) + (c & 1)

restated here.  A lane (i, h) keeps row i, columns [16 h, 16 h + 16) in registers and moves them
with eight 16-byte LDS accesses, step s taking column pair s of its half.  What the kernel relies
on, and what this test holds the map to:

* it is a bijection of the tile, and of every row onto itself (so whole-tile zeroing and the
  F_k product's row reads need nothing else);
* the columns (2 k, 2 k + 1) stay adjacent and 16-byte aligned (one ds_read_b128 per pair), and
  each 16-column half stays within itself (the two half-waves keep their halves);
* banks: a row is 256 bytes, the whole of LDS's 64 four-byte banks, so a 16-byte chunk's
  position in its row is its bank quad.  In every step s the lanes of a half whose rows are in
  one group of eight (i / 8) touch eight distinct chunk positions -- row-major, all 32 lanes
  touch one.
"""
import numpy as np

S = 32


def tile_at(i, c):
    return i * S + (c & 16) + 2 * (((c & 15) >> 1) ^ (i & 7)) + (c & 1)


def row_major(i, c):
    return i * S + c


def _chunks(at, s, h):
    """16-byte chunk position within the row (the bank quad) that lane (i, h) touches in step s."""
    return np.array([(at(i, 16 * h + 2 * s) % S) // 2 for i in range(S)])


def test_map_is_a_bijection_of_the_tile_and_of_each_row():
    pos = np.array([[tile_at(i, c) for c in range(S)] for i in range(S)])
    assert sorted(pos.ravel().tolist()) == list(range(S * S))
    for i in range(S):
        assert sorted(pos[i].tolist()) == list(range(i * S, (i + 1) * S))


def test_pairs_stay_adjacent_and_halves_closed():
    for i in range(S):
        for k in range(S // 2):
            a, b = tile_at(i, 2 * k), tile_at(i, 2 * k + 1)
            assert b == a + 1 and a % 2 == 0, (i, k, a, b)
        for c in range(S):
            assert (tile_at(i, c) - i * S) // 16 == c // 16, (i, c)


def test_each_step_spreads_a_row_group_over_the_eight_chunks():
    for h in range(2):
        for s in range(8):
            q = _chunks(tile_at, s, h)
            assert np.all((q >= 8 * h) & (q < 8 * h + 8))
            for g in range(4):
                assert len(set(q[8 * g:8 * g + 8].tolist())) == 8, (h, s, g, q)
    # and a lane's eight steps cover its half's eight chunks once each
    for h in range(2):
        for i in range(S):
            assert sorted((tile_at(i, 16 * h + 2 * s) % S) // 2 for s in range(8)) == list(range(8 * h, 8 * h + 8))


def test_row_major_is_what_the_swizzle_replaces():
    """The layout the other kernels keep: every lane of a step on one chunk (the 16-way conflict)."""
    for h in range(2):
        for s in range(8):
            assert len(set(_chunks(row_major, s, h).tolist())) == 1
