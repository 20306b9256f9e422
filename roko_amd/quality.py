"""Per-base quality of the polished consensus: the reference implementation
of the quality contract (numpy, no GPU) and the CPU route of `polish` and
`infer`. The device route (ops/hip/head.hip, ops/hip/votes.hip) computes the
same integers; tests compare the two for exact equality.

Per-vote units. One (window, column) with logits z[0..4]: m = max z,
t_j = exp(z_j - m), and for every class k the probability that the column is
NOT k is e_k = (sum_{j != k} t_j) / (sum_j t_j). The sum over the others is
taken directly, never as 1 - p_k, so a dominant class does not lose its small
e_k to cancellation. u_k = min(255, floor(4 * (-10 log10 e_k) + 0.5)), and
255 when e_k = 0: one unit is a quarter Phred, a vote spans Q0 to Q63.75.

Table. Per column slot and class the sum S_k of u_k over the votes the slot
received (on the device: 12-bit fields of one 64-bit word per slot).

Per-slot quality. With c the majority class (ties to the smallest id) and n
the slot's total votes, Q = min(60, S_c // (4 n)): the mean Phred of the
called class over ALL windows that saw the column, so a dissenting window
contributes about 0 and pulls the mean down. Slots without votes get NO_QUAL.

Stitching. The quality string follows the emitted sequence one to one: a
voted slot whose majority is GAP emits neither base nor quality, and draft
bases copied through unpolished (prefix, suffix, contigs without windows) get
Q0. A deleted base therefore carries no quality anywhere.
"""

from __future__ import annotations

from collections import defaultdict
from typing import Dict, List, Tuple

import numpy as np

from . import config as C
from .inference import (NO_VOTE, SLOTS_PER_POS, _BASE_BYTES, _KEY_SHIFT,
                        VoteTable, accumulate_votes, dense_majority,
                        merge_votes)

UNITS_PER_Q = 4
UNIT_MAX = 255
Q_MAX = 60
NO_QUAL = 0xFF
PHRED_OFFSET = 33  # FASTQ encoding


def phred_units(logits) -> np.ndarray:
    """(..., NUM_CLASSES) logits -> uint8 (..., NUM_CLASSES) quarter-Phred
    units of every class, computed in float64."""
    z = np.asarray(logits, dtype=np.float64)
    t = np.exp(z - z.max(axis=-1, keepdims=True))
    total = t.sum(axis=-1)
    units = np.empty(z.shape, dtype=np.uint8)
    with np.errstate(divide="ignore"):
        for k in range(z.shape[-1]):
            others = np.zeros(z.shape[:-1], dtype=np.float64)
            for j in range(z.shape[-1]):
                if j != k:
                    others = others + t[..., j]
            e = others / total
            u = np.floor(UNITS_PER_Q * (-10.0 * np.log10(e)) + 0.5)
            u = np.where(e > 0, np.clip(u, 0, UNIT_MAX), UNIT_MAX)
            units[..., k] = u.astype(np.uint8)
    return units


def accumulate_quality(positions: np.ndarray,
                       units: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """Group (N, W, 2) positions + (N, W, NUM_CLASSES) units into per-column
    unit sums. Returns (unique keys sorted, sums int64 (K, NUM_CLASSES)):
    the keys and order of `accumulate_votes` on the same positions."""
    pos = positions.reshape(-1, 2).astype(np.int64)
    keys = (pos[:, 0] << _KEY_SHIFT) | pos[:, 1]
    out_keys, inv = np.unique(keys, return_inverse=True)
    inv = inv.reshape(-1)
    u = units.reshape(-1, C.NUM_CLASSES)
    # float64 weights hold these small integer sums exactly
    sums = np.stack([np.bincount(inv, weights=u[:, k],
                                 minlength=len(out_keys))
                     for k in range(C.NUM_CLASSES)], axis=1).astype(np.int64)
    return out_keys, sums.reshape(len(out_keys), C.NUM_CLASSES)


def dense_quality(keys: np.ndarray, counts: np.ndarray, sums: np.ndarray,
                  contig_len: int) -> np.ndarray:
    """(keys, counts, sums) -> dense uint8 quality array of contig_len *
    SLOTS_PER_POS slots (slot order of `dense_majority`): Q of the majority
    class per voted slot, NO_QUAL elsewhere. The CPU reference of the
    quality half of the consensus kernel (ops/hip/votes.hip)."""
    qual = np.full(contig_len * SLOTS_PER_POS, NO_QUAL, dtype=np.uint8)
    if len(keys):
        keys = np.asarray(keys, dtype=np.int64)
        counts = np.asarray(counts, dtype=np.int64)
        sums = np.asarray(sums, dtype=np.int64)
        slot = (keys >> _KEY_SHIFT) * SLOTS_PER_POS \
            + (keys & ((1 << _KEY_SHIFT) - 1))
        maj = counts.argmax(axis=1)
        n = counts.sum(axis=1)
        s = sums[np.arange(len(keys)), maj]
        q = np.minimum(Q_MAX, s // (UNITS_PER_Q * np.maximum(n, 1)))
        qual[slot] = np.where(n > 0, q, NO_QUAL).astype(np.uint8)
    return qual


def stitch_dense_qual(draft: str, maj: np.ndarray,
                      qual: np.ndarray) -> Tuple[str, str]:
    """`inference.stitch_dense` with the quality string (Phred+33) of the
    sequence it returns: the sequence is stitch_dense(draft, maj) always."""
    unpolished = chr(PHRED_OFFSET)
    voted = np.flatnonzero(maj != NO_VOTE)
    if len(voted) == 0:
        return draft, unpolished * len(draft)
    on_pos = np.flatnonzero(voted % SLOTS_PER_POS == 0)
    if len(on_pos) == 0:
        return draft, unpolished * len(draft)
    voted = voted[on_pos[0]:]
    m = maj[voted]
    keep = m != C.LABEL_GAP
    mid = _BASE_BYTES[m[keep]].tobytes().decode("ascii")
    q = qual[voted][keep]
    if len(q) and q.max() > Q_MAX:
        raise ValueError("a voted slot carries no quality (NO_QUAL)")
    mid_q = (q + np.uint8(PHRED_OFFSET)).astype(np.uint8).tobytes() \
        .decode("ascii")
    first = int(voted[0]) // SLOTS_PER_POS
    last = int(voted[-1]) // SLOTS_PER_POS
    tail = draft[last + 1:]
    return (draft[:first] + mid + tail,
            unpolished * first + mid_q + unpolished * len(tail))


def unpolished_quality(seq: str) -> str:
    """Quality string of a contig copied through from the draft."""
    return chr(PHRED_OFFSET) * len(seq)


def stitch_tables(draft: str, counts_table, sums_table) -> Tuple[str, str]:
    """Host-route stitch: (keys, counts) and (keys, sums) of one contig ->
    (sequence, quality string) through the dense forms."""
    keys, counts = counts_table
    skeys, sums = sums_table
    if not np.array_equal(keys, skeys):
        raise ValueError("count and quality tables disagree on their keys")
    return stitch_dense_qual(
        draft, dense_majority(keys, counts, len(draft)),
        dense_quality(keys, counts, sums, len(draft)))


class StreamingQualityVotes:
    """`inference.StreamingVotes` with the quality sums beside the counts, in
    the same bounded memory: windows are buffered per contig and folded into
    per-contig (keys, counts) and (keys, sums) tables every `chunk_windows`."""

    def __init__(self, chunk_windows: int = 4096):
        self.chunk = chunk_windows
        self.tables: VoteTable = {}
        self.sums: VoteTable = {}
        self._pos: Dict[str, List[np.ndarray]] = defaultdict(list)
        self._pred: Dict[str, List[np.ndarray]] = defaultdict(list)
        self._unit: Dict[str, List[np.ndarray]] = defaultdict(list)

    def add(self, contig: str, positions: np.ndarray, preds: np.ndarray,
            units: np.ndarray) -> None:
        """One window: positions (W, 2), preds (W,), units (W, 5)."""
        self._pos[contig].append(positions)
        self._pred[contig].append(preds)
        self._unit[contig].append(units)
        if len(self._pos[contig]) >= self.chunk:
            self._flush(contig)

    def _flush(self, contig: str) -> None:
        if not self._pos[contig]:
            return
        pos = np.stack(self._pos[contig])
        t = accumulate_votes(pos, np.stack(self._pred[contig]))
        s = accumulate_quality(pos, np.stack(self._unit[contig]))
        for buf in (self._pos, self._pred, self._unit):
            buf[contig].clear()
        for tabs, new in ((self.tables, t), (self.sums, s)):
            prev = tabs.get(contig)
            tabs[contig] = new if prev is None else merge_votes([prev, new])

    def buffered(self, contig: str) -> int:
        return len(self._pos[contig])

    def finalize(self) -> Tuple[VoteTable, VoteTable]:
        for contig in list(self._pos):
            self._flush(contig)
        return self.tables, self.sums
