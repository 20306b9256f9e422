"""Dense-majority stitching (CPU): stitch_dense over dense_majority must give
the string stitch_contig gives on the same vote table. dense_majority is also
the reference the GPU consensus kernel is tested against."""

import numpy as np
import pytest

from roko_amd import config as C
from roko_amd.inference import (
    NO_VOTE, SLOTS_PER_POS, accumulate_votes, dense_majority, stitch_contig,
    stitch_dense,
)

DRAFT = "".join("ACGT"[i % 4] for i in range(57))  # not a multiple of anything


def _table(rows):
    """rows: {(pos, ins): [count per class]} -> sorted (keys, counts)."""
    items = sorted(rows.items())
    keys = np.array([p << 3 | i for (p, i), _ in items], dtype=np.int64)
    counts = np.array([c for _, c in items], dtype=np.int64).reshape(
        len(items), C.NUM_CLASSES)
    return keys, counts


def _same(draft, keys, counts):
    maj = dense_majority(keys, counts, len(draft))
    assert maj.dtype == np.uint8 and len(maj) == len(draft) * SLOTS_PER_POS
    got = stitch_dense(draft, maj)
    assert got == stitch_contig(draft, keys, counts)
    return got, maj


def test_leading_insertion_only_columns_are_dropped():
    keys, counts = _table({
        (10, 1): [0, 3, 0, 0, 0], (10, 2): [0, 0, 2, 0, 0],  # no (10, 0)
        (11, 0): [3, 0, 0, 0, 0], (11, 1): [0, 0, 0, 2, 1],
        (12, 0): [0, 0, 3, 0, 0],
    })
    got, _ = _same(DRAFT, keys, counts)
    assert got == DRAFT[:11] + "ATG" + DRAFT[13:]


def test_insertion_only_table_returns_draft():
    keys, counts = _table({(5, 1): [1, 0, 0, 0, 0], (5, 3): [0, 1, 0, 0, 0]})
    got, _ = _same(DRAFT, keys, counts)
    assert got == DRAFT


def test_all_gap_majorities_delete_the_span():
    keys, counts = _table({(p, 0): [0, 1, 0, 0, 2] for p in range(20, 26)})
    got, _ = _same(DRAFT, keys, counts)
    assert got == DRAFT[:20] + DRAFT[26:]


def test_tie_goes_to_smallest_class():
    keys, counts = _table({
        (7, 0): [0, 2, 0, 2, 0],   # classes 1 and 3 tie -> 1 ('C')
        (8, 0): [0, 0, 0, 1, 1],   # 3 and GAP tie -> 3 ('T')
        (9, 0): [1, 1, 1, 1, 1],   # all tie -> 0 ('A')
    })
    got, maj = _same(DRAFT, keys, counts)
    assert maj[7 * SLOTS_PER_POS] == 1
    assert got == DRAFT[:7] + "CTA" + DRAFT[10:]


def test_votes_only_in_the_middle_keep_draft_ends():
    keys, counts = _table({
        (30, 0): [0, 0, 3, 0, 0], (30, 1): [0, 0, 0, 0, 3],
        (31, 0): [0, 0, 0, 0, 3], (32, 0): [0, 3, 0, 0, 0],
        (32, 3): [2, 0, 0, 0, 0],
    })
    got, maj = _same(DRAFT, keys, counts)
    assert got == DRAFT[:30] + "GCA" + DRAFT[33:]
    assert (maj[: 30 * SLOTS_PER_POS] == NO_VOTE).all()
    assert (maj[33 * SLOTS_PER_POS:] == NO_VOTE).all()


def test_first_and_last_base_voted():
    n = len(DRAFT)
    keys, counts = _table({(0, 0): [0, 0, 0, 3, 0], (n - 1, 0): [0, 0, 3, 0, 0],
                           (n - 1, 3): [0, 1, 0, 0, 0]})
    got, _ = _same(DRAFT, keys, counts)
    assert got == "TGC"  # only the voted columns survive between the ends


def test_empty_table_returns_draft():
    keys = np.empty(0, dtype=np.int64)
    counts = np.empty((0, C.NUM_CLASSES), dtype=np.int64)
    got, maj = _same(DRAFT, keys, counts)
    assert got == DRAFT and (maj == NO_VOTE).all()


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_random_tables_from_accumulate_votes(seed):
    """Contig of 200, 40 windows at random positions with random classes —
    overlapping windows give real ties and mixed majorities."""
    rng = np.random.default_rng(seed)
    contig_len, n_win = 200, 40
    draft = "".join("ACGT"[int(b)] for b in rng.integers(0, 4, contig_len))
    lo = int(rng.integers(0, 60))  # leave unvoted draft at both ends
    positions = np.empty((n_win, C.WINDOW_COLS, 2), dtype=np.int32)
    for w in range(n_win):
        # a window: consecutive (pos, ins) columns from a random start
        p = int(rng.integers(lo, contig_len - 40))
        cols = []
        while len(cols) < C.WINDOW_COLS:
            n_ins = int(rng.integers(0, C.MAX_INS + 1)) if rng.random() < 0.3 else 0
            cols.extend((p, i) for i in range(n_ins + 1))
            p = min(p + 1, contig_len - 1)
        positions[w] = np.array(cols[: C.WINDOW_COLS], dtype=np.int32)
    preds = rng.integers(0, C.NUM_CLASSES, (n_win, C.WINDOW_COLS)).astype(np.uint8)
    keys, counts = accumulate_votes(positions, preds)
    assert (counts.max(axis=1)[:, None] == counts).sum(axis=1).max() > 1  # ties
    _same(draft, keys, counts)
