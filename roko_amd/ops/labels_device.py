"""Truth labels of feature windows on the GPU (kernels: ops/hip/windows.hip,
truth_scan and label_windows).

The label of a window column (pos, slot) is the truth alignment's base at
that column. `labels.get_pos_and_labels` builds a dict of every column of an
alignment and `features._generate_train` looks 90 of them up per window; here
the same answer comes from a CIGAR lookup per column, the one the device
window builder does per cell:

  slot 0     the op that covers pos is M/=/X: the query base there (A C G T
             -> 0..3, anything else LABEL_UNKNOWN); D or N: LABEL_GAP
  slot s > 0 the s-th query base of the run of consecutive I ops behind the
             op that covers pos, if pos is that op's last reference position
             (whatever the op: M/=/X, D or N) and the run has s bases;
             LABEL_GAP otherwise (the host's "un-labeled insertion slot")
  keep       0 if any of the window's 90 labels is LABEL_UNKNOWN

Columns are labelled only inside the alignment's label span [lo, hi): the
region clipped by the alignment's (filter_aligns-adjusted) start and end.

`pack_truth` puts a contig's truth alignments into the arrays of a read pack
(`_pileup.region_reads`), `TruthPack` uploads and scans them once per contig,
`label_windows_reference` is the vectorised numpy twin of the kernel (the CPU
oracle, and the place to read the rule), and `label_span` gives the span the
windows of an alignment are built over, from its two ends.

Alignments the kernels do not take carry refusal bits (`TRUTH_ERR_*`): a
zero-length op, or an S/H/P op between aligned ops. The host route handles
both; callers send such regions there.
"""

from __future__ import annotations

import copy
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .. import config as C
from ..labels import TruthAlign, filter_aligns

TRUTH_ERR_ZERO_OP = 1  # a zero-length CIGAR op
TRUTH_ERR_CLIP = 2     # S/H/P between aligned ops, or an op code above 8
LABEL_ERR_RANGE = 4    # a window column outside the label span

_SEQ_CODES = "=ACMGRSVTWYHKDBN"  # BAM's 4-bit base alphabet
_CODE_OF = np.full(256, 15, dtype=np.uint8)
for _i, _c in enumerate(_SEQ_CODES):
    _CODE_OF[ord(_c)] = _i
    _CODE_OF[ord(_c.lower())] = _i
#: 4-bit code -> label (ops/hip/windows.hip read_base)
_LABEL_OF = np.full(16, C.LABEL_UNKNOWN, dtype=np.uint8)
_LABEL_OF[[1, 2, 4, 8]] = [0, 1, 2, 3]

_REF_OPS = (0, 2, 3, 7, 8)    # M D N = X consume the reference
_QUERY_OPS = (0, 1, 4, 7, 8)  # M I S = X consume the query
_MATCH_OPS = (0, 7, 8)
_CLIP_OPS = (4, 5, 6)         # S H P
_OP_INS = 1

_FIELDS = (("ref_start", np.int32), ("ref_end", np.int32),
           ("cigar_off", np.uint32), ("seq_off", np.uint32),
           ("cigar", np.uint32), ("seq4", np.uint8))


# ---------------------------------------------------------------------------
# pack

def pack_truth(aligns: Sequence[TruthAlign]) -> dict:
    """TruthAlign records -> the arrays of a read pack: reference bounds,
    CIGAR words, 4-bit bases (two a byte, first base in the high nibble),
    and the offsets of every alignment into the two flat arrays."""
    n = len(aligns)
    ref_start = np.zeros(n, dtype=np.int32)
    ref_end = np.zeros(n, dtype=np.int32)
    cigar_off = np.zeros(n + 1, dtype=np.uint32)
    seq_off = np.zeros(n + 1, dtype=np.uint32)
    cigars, seqs = [], []
    c_at = s_at = 0
    for i, a in enumerate(aligns):
        cig = np.ascontiguousarray(a.cigar, dtype=np.uint32)
        if len(cig) == 0:
            raise ValueError(f"truth alignment {a.qname!r} has no CIGAR ops")
        op, ln = cig & 0xF, (cig >> 4).astype(np.int64)
        end = int(a.pos) + int(ln[np.isin(op, _REF_OPS)].sum())
        if a.pos < 0 or end >= 1 << 31:
            raise ValueError(f"truth alignment {a.qname!r} out of range")
        ref_start[i], ref_end[i] = a.pos, end
        codes = _CODE_OF[np.frombuffer(a.seq.encode("ascii"), dtype=np.uint8)]
        if len(codes) & 1:
            codes = np.append(codes, np.uint8(0))
        seq4 = (codes[0::2] << 4) | codes[1::2]
        cigars.append(cig)
        seqs.append(seq4)
        c_at += len(cig)
        s_at += len(seq4)
        if c_at >= 1 << 31 or s_at >= 1 << 31:
            raise ValueError("truth pack too large")
        cigar_off[i + 1], seq_off[i + 1] = c_at, s_at
    return {
        "ref_start": ref_start,
        "ref_end": ref_end,
        "cigar_off": cigar_off,
        "seq_off": seq_off,
        "cigar": (np.concatenate(cigars) if cigars
                  else np.zeros(0, dtype=np.uint32)),
        "seq4": (np.concatenate(seqs) if seqs
                 else np.zeros(0, dtype=np.uint8)),
        "seq_len": np.array([len(a.seq) for a in aligns], dtype=np.int64),
    }


def unpack_truth(pack: dict, i: int) -> Tuple[np.ndarray, str]:
    """(CIGAR words, sequence) of alignment `i`, as pack_truth took them
    (bases outside BAM's alphabet come back as N, lower case as upper)."""
    c0, c1 = int(pack["cigar_off"][i]), int(pack["cigar_off"][i + 1])
    s0, s1 = int(pack["seq_off"][i]), int(pack["seq_off"][i + 1])
    b = pack["seq4"][s0:s1]
    codes = np.empty(2 * len(b), dtype=np.uint8)
    codes[0::2], codes[1::2] = b >> 4, b & 15
    alphabet = np.frombuffer(_SEQ_CODES.encode("ascii"), dtype=np.uint8)
    seq = alphabet[codes[: int(pack["seq_len"][i])]].tobytes().decode("ascii")
    return pack["cigar"][c0:c1].copy(), seq


def _checked(pack: dict) -> dict:
    """The pack's arrays, contiguous and of the right type, after the checks
    the kernels rely on (the ones ops/windows.py makes for a read pack)."""
    a = {}
    for name, dt in _FIELDS:
        v = np.ascontiguousarray(pack[name])
        if v.dtype != dt or v.ndim != 1:
            raise ValueError(f"pack[{name!r}] must be a 1-d {np.dtype(dt)} array")
        a[name] = v
    n = len(a["ref_start"])
    if len(a["ref_end"]) != n:
        raise ValueError("pack: per-alignment arrays disagree on the count")
    for off, flat in (("cigar_off", "cigar"), ("seq_off", "seq4")):
        o = a[off].astype(np.int64)
        if len(o) != n + 1 or o[0] != 0 or o[-1] != len(a[flat]) \
                or (np.diff(o) < 0).any() or len(a[flat]) >= 1 << 31:
            raise ValueError(f"pack[{off!r}] does not index pack[{flat!r}]")
    if n and (np.diff(a["cigar_off"].astype(np.int64)) == 0).any():
        raise ValueError("pack: an alignment without CIGAR ops")
    if (a["ref_end"] < a["ref_start"]).any() or (a["ref_start"] < 0).any():
        raise ValueError("pack: bad reference bounds")
    return a


# ---------------------------------------------------------------------------
# host scan (what truth_scan computes on the device, plus what label_span
# needs)

class _Scan:
    """Per-op tables of one alignment."""

    __slots__ = ("op", "ln", "rpos", "qpos", "run_end", "err", "_kcum")

    def __init__(self, ref_start: int, cigar: np.ndarray):
        op = (cigar & 0xF).astype(np.int64)
        ln = (cigar >> 4).astype(np.int64)
        rl = np.where(np.isin(op, _REF_OPS), ln, 0)
        ql = np.where(np.isin(op, _QUERY_OPS), ln, 0)
        self.op, self.ln = op, ln
        self.rpos = ref_start + np.cumsum(rl) - rl
        self.qpos = np.cumsum(ql) - ql
        # run_end[k]: query index behind the run of consecutive I ops that
        # starts at op k (qpos[k] itself if op k is no I)
        n = len(op)
        idx = np.where(op != _OP_INS, np.arange(n), n)
        nxt = np.minimum.accumulate(idx[::-1])[::-1]
        qext = np.append(self.qpos, int(ql.sum()))
        self.run_end = qext[nxt]
        body = np.flatnonzero(~np.isin(op, _CLIP_OPS))
        err = TRUTH_ERR_ZERO_OP if (ln == 0).any() else 0
        if (op > 8).any():
            err |= TRUTH_ERR_CLIP
        if len(body):
            inner = op[body[0] : body[-1] + 1]
            if np.isin(inner, _CLIP_OPS).any():
                err |= TRUTH_ERR_CLIP
        self.err = err
        self._kcum = None


def scan_truth(pack: dict) -> List[_Scan]:
    """Host twin of the truth_scan kernel: one _Scan per alignment."""
    co = pack["cigar_off"].astype(np.int64)
    return [_Scan(int(pack["ref_start"][i]), pack["cigar"][co[i] : co[i + 1]])
            for i in range(len(pack["ref_start"]))]


def _labels_at(pack: dict, i: int, q: np.ndarray) -> np.ndarray:
    """Label of the query bases `q` of alignment i (read_base of
    windows.hip): LABEL_UNKNOWN outside the stored sequence."""
    s0, s1 = int(pack["seq_off"][i]), int(pack["seq_off"][i + 1])
    byte = q >> 1
    ok = (q >= 0) & (byte < s1 - s0)
    b = pack["seq4"][s0 + np.where(ok, byte, 0)] if s1 > s0 \
        else np.zeros(q.shape, dtype=np.uint8)
    nib = np.where(q & 1, b & 15, b >> 4)
    return np.where(ok, _LABEL_OF[nib], C.LABEL_UNKNOWN).astype(np.uint8)


def _known_prefix(pack: dict, i: int, sc: _Scan) -> np.ndarray:
    """kcum[q] = number of A/C/G/T among the first q query bases."""
    if sc._kcum is None:
        s0, s1 = int(pack["seq_off"][i]), int(pack["seq_off"][i + 1])
        b = pack["seq4"][s0:s1]
        codes = np.empty(2 * len(b), dtype=np.uint8)
        codes[0::2], codes[1::2] = b >> 4, b & 15
        known = _LABEL_OF[codes] != C.LABEL_UNKNOWN
        sc._kcum = np.concatenate(([0], np.cumsum(known, dtype=np.int64)))
    return sc._kcum


def _lookup(sc: _Scan, p: np.ndarray):
    """The op that covers every position of `p` (inside the alignment):
    (j, op, last): its index, its code, and whether p is its last reference
    position."""
    j = np.searchsorted(sc.rpos, p, side="right") - 1
    j = np.clip(j, 0, len(sc.op) - 1)
    return j, sc.op[j], p == sc.rpos[j] + sc.ln[j] - 1


def label_windows_reference(pos: np.ndarray, pack: dict, index: int, lo: int,
                            hi: int, scan: Optional[List[_Scan]] = None):
    """numpy twin of the label_windows kernel: positions (n, 90, 2) of built
    windows, alignment `index` of the pack and its label span [lo, hi) ->
    (labels (n, 90) uint8, keep (n) uint8, err). err has LABEL_ERR_RANGE set
    if a column lies outside the span (such a column is labelled
    LABEL_GAP)."""
    pos = np.asarray(pos)
    if pos.ndim != 3 or pos.shape[1:] != (C.WINDOW_COLS, 2):
        raise ValueError(f"pos must be (n, {C.WINDOW_COLS}, 2), got {pos.shape}")
    sc = (scan or scan_truth(pack))[index]
    lo = max(int(lo), int(pack["ref_start"][index]))
    hi = min(int(hi), int(pack["ref_end"][index]))
    p = pos[..., 0].astype(np.int64)
    s = pos[..., 1].astype(np.int64)
    inside = (p >= lo) & (p < hi) & (s >= 0)
    j, op, last = _lookup(sc, p)
    labels = np.full(p.shape, C.LABEL_GAP, dtype=np.uint8)
    err = 0 if inside.all() else LABEL_ERR_RANGE

    slot0 = inside & (s == 0)
    match = slot0 & np.isin(op, _MATCH_OPS)
    labels[match] = _labels_at(pack, index, (sc.qpos[j] + p - sc.rpos[j])[match])
    if (slot0 & ~np.isin(op, _REF_OPS)).any():
        err |= LABEL_ERR_RANGE

    # insertion slots: the I run behind op j starts at op k = j + 1
    k = np.minimum(j + 1, len(sc.op) - 1)
    run = np.where((j + 1 < len(sc.op)) & (sc.op[k] == _OP_INS),
                   sc.run_end[k] - sc.qpos[k], 0)
    ins = inside & (s > 0) & last & (s <= run)
    labels[ins] = _labels_at(pack, index, (sc.qpos[k] + s - 1)[ins])

    keep = (~(labels == C.LABEL_UNKNOWN).any(axis=1)).astype(np.uint8)
    return labels, keep, err


def label_span(pack: dict, index: int, lo: int, hi: int,
               scan: Optional[List[_Scan]] = None,
               chunk: int = 4096) -> Optional[Tuple[int, int]]:
    """(sub_start, sub_end) of alignment `index` over the label span
    [lo, hi): the smallest and the largest position that has a column, slot 0
    or insertion, whose label is not LABEL_UNKNOWN. This is the span
    features._generate_train builds the alignment's windows over (sub_end
    exclusive, as there). None if no column is labelled. Looks at the two
    ends of the span only, `chunk` positions at a time."""
    sc = (scan or scan_truth(pack))[index]
    lo = max(int(lo), int(pack["ref_start"][index]))
    hi = min(int(hi), int(pack["ref_end"][index]))
    if lo >= hi:
        return None
    kcum = _known_prefix(pack, index, sc)

    def labelled(a: int, b: int) -> np.ndarray:
        p = np.arange(a, b, dtype=np.int64)
        j, op, last = _lookup(sc, p)
        base = _labels_at(pack, index, sc.qpos[j] + p - sc.rpos[j])
        known = np.where(np.isin(op, _MATCH_OPS), base != C.LABEL_UNKNOWN,
                         np.isin(op, (2, 3)))
        k = np.minimum(j + 1, len(sc.op) - 1)
        has_run = last & (j + 1 < len(sc.op)) & (sc.op[k] == _OP_INS)
        ins_known = has_run & (kcum[sc.run_end[k]] - kcum[sc.qpos[k]] > 0)
        return known | ins_known

    first = None
    for a in range(lo, hi, chunk):
        hit = np.flatnonzero(labelled(a, min(a + chunk, hi)))
        if len(hit):
            first = a + int(hit[0])
            break
    if first is None:
        return None
    for b in range(hi, lo, -chunk):
        a = max(b - chunk, lo)
        hit = np.flatnonzero(labelled(a, b))
        if len(hit):
            return first, a + int(hit[-1])
    return None  # not reached: `first` is labelled


# ---------------------------------------------------------------------------
# which alignments label a region (host)

def region_aligns(contig_aligns: Sequence[TruthAlign], ref_ends: np.ndarray,
                  start: int, end: int) -> List[Tuple[int, TruthAlign]]:
    """What `filter_aligns(get_aligns(bam, contig, start, end))` gives, from
    the contig's records fetched once (`get_aligns(bam, contig)`): the kept
    alignments of the region with their clipped start / end, each with its
    index into `contig_aligns`. filter_aligns changes its inputs, so every
    region works on fresh copies."""
    picked = []
    for i, a in enumerate(contig_aligns):
        if ref_ends[i] <= start or a.pos >= end:
            continue
        b = copy.copy(a)
        b.start, b.end, b.keep = a.pos, int(ref_ends[i]), True
        picked.append((i, b))
    index_of = {id(b): i for i, b in picked}
    return [(index_of[id(b)], b) for b in filter_aligns([b for _, b in picked])]


# ---------------------------------------------------------------------------
# device

class TruthPack:
    """A contig's truth alignments on the device: uploaded once, scanned once
    (truth_scan), indexed by every region of the contig."""

    def __init__(self, aligns: Sequence[TruthAlign], device,
                 pack: Optional[dict] = None):
        """`pack`: pack_truth(aligns), if the caller has it already."""
        import torch

        from . import ext

        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("TruthPack needs a GPU device, got "
                             f"{device.type!r}")
        self.device = device
        self.host = pack if pack is not None else pack_truth(aligns)
        a = _checked(self.host)
        self.n = len(a["ref_start"])
        self.err = np.zeros(self.n, dtype=np.int32)
        self._dev = None
        if self.n == 0:
            return
        dev = [torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32
                                else v).to(device)
               for v in (a[name] for name, _ in _FIELDS)]
        with torch.cuda.device(device):
            op_rpos, op_qpos, err = ext().truth_scan(*dev)
        self._dev = dev + [op_rpos, op_qpos]
        self.err = err.cpu().numpy()

    def label_windows(self, pos, index: int, lo: int, hi: int):
        """pos (n, 90, 2) int32 on the device -> (labels (n, 90) uint8,
        keep (n) uint8, err (1) int32), device tensors on the current
        stream."""
        import torch

        from . import ext

        if self._dev is None or not 0 <= index < self.n:
            raise ValueError(f"no truth alignment {index} in the pack")
        if self.err[index]:
            raise ValueError(f"truth alignment {index} was refused by "
                             f"truth_scan (bits {int(self.err[index])})")
        with torch.cuda.device(self.device):
            return tuple(ext().label_windows(pos, *self._dev, int(index),
                                             int(lo), int(hi)))
