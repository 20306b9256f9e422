"""Quality-gated stitch: the polished sequence with only the edits the model
is sure of, and with uncovered draft bases kept on request. This module is
the contract (numpy, no GPU) and the CPU route of `polish` and `infer`; the
device route (ops/hip/stitch.hip, DeviceVotes.stitch) computes the same two
strings and tests compare them for exact equality.

Two parameters: `min_qual` (0..60), the smallest quality at which an edit is
applied, and `keep_uncovered`, whether a draft base inside the stitch window
that no model window covered stays (the reference stitch drops it).

Inputs are those of edits.py: the draft and the dense arrays `maj` and
`qual`, slot = pos * SLOTS_PER_POS + ins. The stitch window is that of
`inference.stitch_dense`: s0 the first voted ins == 0 slot, first = s0 // 4,
last = (last voted slot) // 4. Positions outside first..last emit the draft
base as it is at Q0. Inside, slot (p, i) with d = draft[p] uppercased and
q = qual[s] emits:

  i == 0, majority base b == d                  b, q
  i == 0, majority base b != d   q >= min_qual  b, q
                                 q <  min_qual  draft[p] as it is, Q0
  i == 0, majority GAP           q >= min_qual  nothing
                                 q <  min_qual  draft[p] as it is, Q0
  i == 0, not voted              keep_uncovered draft[p] as it is, Q0
                                 otherwise      nothing
  i  > 0, majority base b        q >= min_qual  b, q
                                 q <  min_qual  nothing
  i  > 0, GAP or not voted                      nothing

A rejected call leaves the draft base at Q0, the existing meaning of "copied
through unpolished". An uncovered deletion has no quality: `min_qual` does
not touch it, `keep_uncovered` decides it.

With both parameters at their defaults the result is
`quality.stitch_dense_qual(draft, maj, qual)`. With e = dense_edits(draft,
maj, qual), `apply_edits(draft, e[applied(e, Q, K)])` equals the sequence of
`stitch_filtered(draft, maj, qual, Q, K)` up to case.
"""

from __future__ import annotations

from typing import Tuple

import numpy as np

from . import config as C
from .edits import draft_bytes_upper, is_uncovered
from .inference import NO_VOTE, SLOTS_PER_POS, _BASE_BYTES, dense_majority
from .quality import (PHRED_OFFSET, Q_MAX, dense_quality, unpolished_quality)


def check_filter(min_qual: int, keep_uncovered: bool) -> Tuple[int, bool]:
    """(min_qual, keep_uncovered) validated: min_qual an integer in 0..Q_MAX."""
    if isinstance(min_qual, bool) or int(min_qual) != min_qual \
            or not 0 <= int(min_qual) <= Q_MAX:
        raise ValueError(f"min_qual must be an integer in 0..{Q_MAX}, "
                         f"got {min_qual!r}")
    return int(min_qual), bool(keep_uncovered)


def is_default(min_qual: int, keep_uncovered: bool) -> bool:
    return min_qual == 0 and not keep_uncovered


def filter_header(min_qual: int, keep_uncovered: bool) -> str:
    """The VCF header line that names a filter not at its defaults."""
    return (f"##roko_filter=min_qual={int(min_qual)};"
            f"keep_uncovered={int(bool(keep_uncovered))}")


def stitch_filtered(draft: str, maj: np.ndarray, qual: np.ndarray,
                    min_qual: int = 0,
                    keep_uncovered: bool = False) -> Tuple[str, str]:
    """(sequence, Phred+33 quality string) of one contig under the filter
    (the table in the module docstring)."""
    min_qual, keep_uncovered = check_filter(min_qual, keep_uncovered)
    n = len(draft)
    maj = np.asarray(maj, dtype=np.uint8)
    qual = np.asarray(qual, dtype=np.uint8)
    if maj.shape != (n * SLOTS_PER_POS,) or qual.shape != maj.shape:
        raise ValueError("maj and qual must hold SLOTS_PER_POS slots per "
                         "draft base")
    m = maj.reshape(n, SLOTS_PER_POS)
    voted = m != NO_VOTE
    on_pos = np.flatnonzero(voted[:, 0])
    if len(on_pos) == 0:
        return draft, unpolished_quality(draft)
    first = int(on_pos[0])
    last = int(np.flatnonzero(voted.any(axis=1))[-1])
    m = m[first:last + 1]
    q = qual.reshape(n, SLOTS_PER_POS)[first:last + 1]
    raw = np.frombuffer(draft.encode("ascii"), dtype=np.uint8)[first:last + 1]
    d = draft_bytes_upper(draft)[first:last + 1]

    is_base = m < C.LABEL_GAP
    called = _BASE_BYTES[np.minimum(m, C.LABEL_GAP)]
    sure = q >= min_qual  # read only where the slot is voted
    seq = np.zeros(m.shape, dtype=np.uint8)  # 0: the slot emits nothing
    ql = np.zeros(m.shape, dtype=np.uint8)
    # ins == 0
    same = is_base[:, 0] & (called[:, 0] == d)
    sub = is_base[:, 0] & ~same
    dele = m[:, 0] == C.LABEL_GAP
    call = same | (sub & sure[:, 0])
    keep_draft = ((sub | dele) & ~sure[:, 0])
    if keep_uncovered:
        keep_draft |= ~voted[first:last + 1, 0]
    seq[:, 0] = np.where(call, called[:, 0], np.where(keep_draft, raw, 0))
    ql[:, 0] = np.where(call, q[:, 0], 0)
    # ins > 0
    ins = is_base[:, 1:] & sure[:, 1:]
    seq[:, 1:] = np.where(ins, called[:, 1:], 0)
    ql[:, 1:] = np.where(ins, q[:, 1:], 0)

    emitted = seq.reshape(-1) != 0
    mid_q = ql.reshape(-1)[emitted]
    if len(mid_q) and mid_q.max() > Q_MAX:
        raise ValueError("a voted slot carries no quality (NO_QUAL)")
    mid = seq.reshape(-1)[emitted].tobytes().decode("ascii")
    mid_q = (mid_q + np.uint8(PHRED_OFFSET)).astype(np.uint8).tobytes() \
        .decode("ascii")
    tail = draft[last + 1:]
    return (draft[:first] + mid + tail,
            unpolished_quality(draft[:first]) + mid_q
            + unpolished_quality(tail))


def applied(edits: np.ndarray, min_qual: int = 0,
            keep_uncovered: bool = False) -> np.ndarray:
    """Mask of the `edits` (edits.EDIT_DTYPE) the filter applies: an
    uncovered deletion unless `keep_uncovered`, any other edit when its
    quality is at least `min_qual`."""
    min_qual, keep_uncovered = check_filter(min_qual, keep_uncovered)
    return np.where(is_uncovered(edits), not keep_uncovered,
                    edits["qual"] >= min_qual)


def applied_edits(edits: np.ndarray, min_qual: int = 0,
                  keep_uncovered: bool = False) -> np.ndarray:
    """The edits the filter applies: what a filtered VCF lists."""
    if is_default(min_qual, keep_uncovered):
        return edits
    return edits[applied(edits, min_qual, keep_uncovered)]


def vcf_header(min_qual: int, keep_uncovered: bool) -> Tuple[str, ...]:
    """Extra VCF header lines: the filter, only when it is not the default."""
    if is_default(min_qual, keep_uncovered):
        return ()
    return (filter_header(min_qual, keep_uncovered),)


def stitch_tables_filtered(draft: str, counts_table, sums_table,
                           min_qual: int = 0,
                           keep_uncovered: bool = False) -> Tuple[str, str]:
    """Host-route filtered stitch: (keys, counts) and (keys, sums) of one
    contig through the dense forms (as quality.stitch_tables)."""
    keys, counts = counts_table
    skeys, sums = sums_table
    if not np.array_equal(keys, skeys):
        raise ValueError("count and quality tables disagree on their keys")
    return stitch_filtered(
        draft, dense_majority(keys, counts, len(draft)),
        dense_quality(keys, counts, sums, len(draft)), min_qual,
        keep_uncovered)
