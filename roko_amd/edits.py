"""What the polisher changed: the edits between a draft and its polished
form, and their VCF. This module is the contract (numpy, no GPU) and the CPU
route of `polish` and `infer`; the device route (ops/hip/edits.hip,
DeviceVotes.edits) computes the same array and tests compare the two for
exact equality.

Inputs are the draft, the dense majority array `maj` (inference.dense_majority
/ DeviceVotes.consensus, NO_VOTE = 0xFF) and the dense quality array `qual`
(quality.dense_quality, NO_QUAL = 0xFF), slot = pos * SLOTS_PER_POS + ins.

Stitch window, exactly as `inference.stitch_dense`: s0 is the first voted
slot with ins == 0 (none: no edits), first = s0 // 4, last = (last voted
slot) // 4; only slots s0 .. last * 4 + 3 are considered, so voted
insertion-only slots before s0 are ignored as the stitch ignores them.

One slot (p, i) with d = draft[p] uppercased yields at most one edit:

  i == 0, not voted            uncovered deletion  ref d, alt *, qual NO_QUAL
  i == 0, majority GAP         deletion            ref d, alt *, qual[s]
  i == 0, majority base b != d substitution        ref d, alt b, qual[s]
  i  > 0, majority a base b    insertion           ref *, alt b, qual[s]
  i  > 0, GAP or not voted     nothing

A draft N (or any non-ACGT letter) against a called base is a substitution;
a lowercase draft letter equal to the call after uppercasing is not an edit.
`apply_edits(draft, dense_edits(draft, maj, qual)).upper()` equals
`stitch_dense(draft, maj).upper()`: case is the only thing the stitch changes
that is not an edit.

An uncovered deletion is the stitch dropping a draft base inside the window
that no model window covered; it is an edit like any other here, and the VCF
flags it NOCOV.
"""

from __future__ import annotations

import os
from typing import Iterable, List, Sequence, Tuple

import numpy as np

from . import config as C
from .inference import NO_VOTE, SLOTS_PER_POS, _BASE_BYTES
from .quality import NO_QUAL

EDIT_DTYPE = np.dtype([("pos", "<i8"), ("ins", "u1"), ("ref", "u1"),
                       ("alt", "u1"), ("qual", "u1")])
GAP_BYTE = ord("*")

#: one VCF data line: (contig, 1-based POS, REF, ALT, QUAL, INFO)
VcfRecord = Tuple[str, int, str, str, int, str]


def draft_bytes_upper(draft: str) -> np.ndarray:
    """The draft as uint8 ASCII with a-z uppercased (what the device kernel
    does to the byte it loads); other bytes stay as they are."""
    d = np.frombuffer(bytearray(draft, "ascii"), dtype=np.uint8)
    lower = (d >= ord("a")) & (d <= ord("z"))
    d[lower] -= 32
    return d


def dense_edits(draft: str, maj: np.ndarray, qual: np.ndarray) -> np.ndarray:
    """The edits of one contig, ascending in slot order (EDIT_DTYPE; ref and
    alt are ASCII, '*' for gap)."""
    n = len(draft)
    maj = np.asarray(maj, dtype=np.uint8)
    qual = np.asarray(qual, dtype=np.uint8)
    if maj.shape != (n * SLOTS_PER_POS,) or qual.shape != maj.shape:
        raise ValueError("maj and qual must hold SLOTS_PER_POS slots per "
                         "draft base")
    out = np.empty(0, dtype=EDIT_DTYPE)
    m = maj.reshape(n, SLOTS_PER_POS)
    voted = m != NO_VOTE
    on_pos = np.flatnonzero(voted[:, 0])
    if len(on_pos) == 0:
        return out
    first = int(on_pos[0])
    last = int(np.flatnonzero(voted.any(axis=1))[-1])
    d = draft_bytes_upper(draft)
    in_window = np.zeros(n, dtype=bool)
    in_window[first:last + 1] = True
    is_base = m < C.LABEL_GAP
    called = _BASE_BYTES[np.minimum(m, C.LABEL_GAP)]  # '*' for GAP / no vote
    edit = is_base & in_window[:, None]
    edit[:, 0] = in_window & (~is_base[:, 0] | (called[:, 0] != d))
    slots = np.flatnonzero(edit.reshape(-1))
    if len(slots) == 0:
        return out
    pos, ins = slots // SLOTS_PER_POS, slots % SLOTS_PER_POS
    out = np.empty(len(slots), dtype=EDIT_DTYPE)
    out["pos"] = pos
    out["ins"] = ins
    out["ref"] = np.where(ins == 0, d[pos], GAP_BYTE)
    out["alt"] = called.reshape(-1)[slots]
    out["qual"] = np.where(maj[slots] != NO_VOTE, qual[slots], NO_QUAL)
    return out


def table_edits(draft: str, counts_table, sums_table) -> np.ndarray:
    """Host-route edits: (keys, counts) and (keys, sums) of one contig
    through the dense forms (as quality.stitch_tables)."""
    from .inference import dense_majority
    from .quality import dense_quality

    keys, counts = counts_table
    skeys, sums = sums_table
    if not np.array_equal(keys, skeys):
        raise ValueError("count and quality tables disagree on their keys")
    return dense_edits(draft, dense_majority(keys, counts, len(draft)),
                       dense_quality(keys, counts, sums, len(draft)))


def apply_edits(draft: str, edits: np.ndarray) -> str:
    """Replay `edits` on `draft`: substituted and inserted bases come out
    uppercase, everything else keeps the draft's case."""
    n = len(draft)
    grid = np.zeros((n, SLOTS_PER_POS), dtype=np.uint8)
    grid[:, 0] = np.frombuffer(draft.encode("ascii"), dtype=np.uint8)
    alt = np.where(edits["alt"] == GAP_BYTE, 0, edits["alt"]).astype(np.uint8)
    grid[edits["pos"], edits["ins"]] = alt
    flat = grid.reshape(-1)
    return flat[flat != 0].tobytes().decode("ascii")


def is_uncovered(edits: np.ndarray) -> np.ndarray:
    """Mask of the uncovered deletions among `edits`."""
    return (edits["ins"] == 0) & (edits["alt"] == GAP_BYTE) \
        & (edits["qual"] == NO_QUAL)


def vcf_records(contig: str, draft: str, edits: np.ndarray) -> List[VcfRecord]:
    """One VCF record per cluster of `edits`: a maximal run in which each
    edit sits at the previous edit's draft position or the next one (an
    insertion at (p, i) belongs to p). REF is the draft over the cluster's
    span, uppercased; ALT is what the polished sequence holds for it. When
    the lengths differ and the two do not start with the same letter, the
    unedited draft base before the span is prepended to both (after it, for
    a span starting at position 0). QUAL is the smallest edit quality of the
    cluster (an uncovered deletion counts 0); INFO is NE=<edits> and the flag
    NOCOV if any of them is an uncovered deletion. A cluster whose edits
    leave its span as it was gives no record."""
    if len(edits) == 0:
        return []
    pos = edits["pos"].astype(np.int64)
    starts = np.concatenate([[0], np.flatnonzero(np.diff(pos) > 1) + 1])
    ends = np.concatenate([starts[1:], [len(edits)]]).tolist()
    q0 = np.where(edits["qual"] == NO_QUAL, 0, edits["qual"])
    qmin = np.minimum.reduceat(q0, starts).tolist()
    nocov = np.add.reduceat(is_uncovered(edits).astype(np.int64), starts) \
        .tolist()
    starts = starts.tolist()
    # plain lists and strings from here on: most clusters hold one edit, and
    # per-cluster numpy calls would cost more than the work they do
    pos_l, on_pos = pos.tolist(), (edits["ins"] == 0).tolist()
    alt_l = edits["alt"].tobytes().decode("ascii")
    out: List[VcfRecord] = []
    for k, (lo, hi) in enumerate(zip(starts, ends)):
        a, b = pos_l[lo], pos_l[hi - 1]
        ref = draft[a:b + 1].upper()
        pieces, cur = [], 0  # cur: first base of ref not yet emitted
        for e in range(lo, hi):
            p = pos_l[e] - a
            if on_pos[e]:  # base p is replaced, or dropped
                pieces.append(ref[cur:p])
                if alt_l[e] != "*":
                    pieces.append(alt_l[e])
            else:          # base p, if still to come, then the inserted base
                pieces.append(ref[cur:p + 1])
                pieces.append(alt_l[e])
            cur = p + 1
        pieces.append(ref[cur:])
        alt = "".join(pieces)
        vpos = a + 1
        if ref == alt:
            # the cluster's edits cancel (a base deleted and the same base
            # inserted beside it): the sequence does not change, and a VCF
            # record may not have ALT equal to REF
            continue
        if len(ref) != len(alt) and (not alt or ref[0] != alt[0]):
            if a > 0:
                anchor = draft[a - 1].upper()
                ref, alt, vpos = anchor + ref, anchor + alt, a
            elif b + 1 < len(draft):
                anchor = draft[b + 1].upper()
                ref, alt = ref + anchor, alt + anchor
        info = f"NE={hi - lo};NOCOV" if nocov[k] else f"NE={hi - lo}"
        # a whole contig deleted has no base left to anchor on: VCF's '*'
        out.append((contig, vpos, ref, alt or "*", qmin[k], info))
    return out


VCF_HEADER = (
    "##fileformat=VCFv4.2",
    "##source=roko_amd.polish",
)
VCF_INFO = (
    '##INFO=<ID=NE,Number=1,Type=Integer,Description="Polishing edits '
    '(substituted, deleted or inserted bases) merged into this record">',
    '##INFO=<ID=NOCOV,Number=0,Type=Flag,Description="At least one deleted '
    'draft base was dropped because no model window covered it">',
)
VCF_COLUMNS = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"


def write_vcf(path: str, contig_lens: Sequence[Tuple[str, int]],
              records: Iterable[VcfRecord],
              extra_header: Sequence[str] = ()) -> int:
    """Write VCF 4.2: one ##contig line per (name, length) of `contig_lens`
    in the given order, then `records` as they come. `extra_header` lines
    (stitch.filter_header) follow ##source. Returns the number of records.
    Creates parent dirs."""
    d = os.path.dirname(os.path.abspath(path))
    os.makedirs(d, exist_ok=True)
    n = 0
    with open(path, "w") as fh:
        for line in tuple(VCF_HEADER) + tuple(extra_header):
            fh.write(line + "\n")
        for name, length in contig_lens:
            fh.write(f"##contig=<ID={name},length={length}>\n")
        for line in VCF_INFO:
            fh.write(line + "\n")
        fh.write(VCF_COLUMNS + "\n")
        for contig, pos, ref, alt, qual, info in records:
            fh.write(f"{contig}\t{pos}\t.\t{ref}\t{alt}\t{qual}\t.\t{info}\n")
            n += 1
    return n


def contig_vcf_records(refs: Sequence[Tuple[str, str]],
                       edits: dict) -> List[VcfRecord]:
    """Records of every contig of `refs` ((name, draft) pairs, in order)
    that has an entry in `edits`."""
    out: List[VcfRecord] = []
    for name, draft in refs:
        e = edits.get(name)
        if e is not None and len(e):
            out.extend(vcf_records(name, draft, e))
    return out
