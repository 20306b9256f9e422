"""Small truth + reads BAM pairs for the device label tests
(test_labels_device.py, test_gpu_labels.py), and the dict-path oracle both
compare against. Every builder returns a dict: reads_bam, truth_bam, contig,
regions [(start, end)], draft_len."""

from __future__ import annotations

import numpy as np

from roko_amd import config as C
from roko_amd.io.bamio import SamRecord, write_bam
from tests.window_cases import read

CONTIG = "ctg1"
SEED = 11


def _ref_len(cig):
    return sum(l for l, op in cig if op in "MDN=X")


def _ins_positions(pos, cig):
    """Reference positions an I op of the CIGAR hangs behind."""
    out, r = [], pos
    for l, op in cig:
        if op == "I":
            out.append(r - 1)
        elif op in "MDN=X":
            r += l
    return out


def _write(tmp_path, name, draft_len, truths, regions, extra_reads=()):
    """truths: [(pos, cigar list, sequence or None)]. Reads: plain
    background, copies of every truth CIGAR with random bases, and a read
    with an insertion of 4 behind every position a truth insertion hangs
    behind (a read's insertion makes a column only behind a match op)."""
    rng = np.random.default_rng(sum(map(ord, name)))
    d = tmp_path / name
    d.mkdir(exist_ok=True)
    refs = [(CONTIG, draft_len)]
    trecs = []
    R = [read(rng, f"bg{i}", 0, f"{draft_len}M", flag=16 if i % 2 else 0)
         for i in range(5)]
    for t, (pos, cig, seq) in enumerate(truths):
        rec = read(rng, f"truth{t}", pos, cig)
        if seq is not None:
            assert len(seq) == len(rec.seq)
            rec = SamRecord(rec.qname, 0, 0, pos, 60, rec.cigar, seq)
        trecs.append(rec)
        for i in range(2):
            R.append(read(rng, f"like{t}_{i}", pos, cig,
                          flag=16 if i else 0))
        for k, p in enumerate(sorted(set(_ins_positions(pos, cig)))):
            if 30 <= p < draft_len - 40:
                R.append(read(rng, f"ins{t}_{k}", p - 30, "31M4I35M"))
    R += list(extra_reads)
    R.sort(key=lambda r: (r.tid, r.pos))
    trecs.sort(key=lambda r: (r.tid, r.pos))
    write_bam(str(d / "reads.bam"), refs, R)
    write_bam(str(d / "truth.bam"), refs, trecs)
    return {"reads_bam": str(d / "reads.bam"),
            "truth_bam": str(d / "truth.bam"), "contig": CONTIG,
            "regions": list(regions), "draft_len": draft_len,
            "truth_records": trecs}


# positions of the `shapes` record, by construction:
#   [0, 300) M, [300, 302) D, 2I behind the D (at 301), [302, 500) M,
#   2I behind 499, [500, 700) M, 2I 3I behind 699, [700, 1000) M, 5I behind
#   999, [1000, 1004) N, 1I behind the N (at 1003), [1004, 1700) M, 3I behind
#   1699, [1700, 2200) M
SHAPES_CIGAR = [(300, "M"), (2, "D"), (2, "I"), (198, "M"), (2, "I"),
                (200, "M"), (2, "I"), (3, "I"), (300, "M"), (5, "I"),
                (4, "N"), (1, "I"), (696, "M"), (3, "I"), (500, "M")]
SHAPES_REGIONS = [(0, 2200), (500, 1700), (301, 1000), (1003, 1004 + 400)]


def shapes(tmp_path):
    """One record with every CIGAR shape the label rule names: an I right
    behind a D and behind an N, 2I 3I back to back, an insertion of 5, and
    for the region [500, 1700) an insertion right before lo and one right
    behind hi - 1. The regions clip the record on both sides."""
    assert _ref_len(SHAPES_CIGAR) == 2200
    return _write(tmp_path, "shapes", 2200, [(0, SHAPES_CIGAR, None)],
                  SHAPES_REGIONS)


def two_records(tmp_path):
    """Two records that overlap by 50: filter_aligns moves the first one's
    end to 1250 and the second one's start to 1300."""
    a = [(600, "M"), (1, "I"), (700, "M")]              # [0, 1300)
    b = [(10, "S"), (700, "M"), (2, "I"), (650, "M")]   # [1250, 2600)
    return _write(tmp_path, "two", 2600, [(0, a, None), (1250, b, None)],
                  [(0, 2600), (1000, 2000), (1240, 1310)])


def long_cigar(tmp_path):
    """181 ops: two 64-op scan chunks and a tail of 53."""
    cig = []
    for i in range(45):
        cig += [(10, "M"), (1 + i % 4, "I"), (12, "M"), (1 + i % 2, "D")]
    cig.append((200, "M"))
    assert len(cig) >= 130
    n = _ref_len(cig) + 60
    return _write(tmp_path, "long", n, [(30, cig, None)],
                  [(0, n), (100, n - 100)])


def one_op(tmp_path):
    """A one-op CIGAR; the reads have insertions the truth has not."""
    return _write(tmp_path, "one", 1200, [(0, [(1200, "M")], None)],
                  [(0, 1200), (50, 1100)])


def with_n(tmp_path):
    """The `shapes` record with N bases: a run in the middle (windows are
    dropped), in the 5I insertion, and at both ends of the spans of the
    regions (0, 2200) and (500, 1700), so sub_start / sub_end move."""
    rng = np.random.default_rng(5)
    rec = read(rng, "t", 0, SHAPES_CIGAR)
    seq = list(rec.seq)
    q_of = {}  # reference position -> query index (match ops)
    q, r = 0, 0
    ins_q = {}
    for l, op in SHAPES_CIGAR:
        if op == "M":
            for k in range(l):
                q_of[r + k] = q + k
            q, r = q + l, r + l
        elif op == "I":
            ins_q.setdefault(r - 1, q)
            q += l
        else:
            r += l
    for p in (0, 1, 2199, 2198, 500, 1699, 1698) + tuple(range(1300, 1306)):
        seq[q_of[p]] = "N"
    seq[ins_q[999] + 3] = "N"  # 4th base of the 5I: beyond MAX_INS
    seq[ins_q[699] + 1] = "N"  # 2nd base of 2I 3I: drops windows
    return _write(tmp_path, "with_n", 2200, [(0, SHAPES_CIGAR, "".join(seq))],
                  [(0, 2200), (500, 1700)])


def two_records_n(tmp_path):
    """two_records with N in the second record (the end-to-end case)."""
    rng = np.random.default_rng(6)
    a = [(600, "M"), (1, "I"), (700, "M")]
    b = [(10, "S"), (700, "M"), (2, "I"), (650, "M")]
    rb = read(rng, "t", 1250, b)
    seq = list(rb.seq)
    for k in (400, 401, 402, 900):
        seq[k] = "N"
    return _write(tmp_path, "two_n", 2600,
                  [(0, a, None), (1250, b, "".join(seq))], [(0, 2600)])


CASES_B = (shapes, two_records, long_cigar, one_op)
CASES_C = (with_n,)


# ---------------------------------------------------------------------------
# the dict path: labels.get_pos_and_labels + the lookup of
# features._generate_train, every column looked up (no early break)

def dict_labels(a, start, end, positions):
    """(labels (n, 90), keep (n)) of `positions` for truth alignment `a`
    over the region, by the host rule."""
    from roko_amd.labels import get_pos_and_labels

    t_pos, t_labels = get_pos_and_labels(a, start, end)
    table = dict(zip(t_pos, t_labels))
    n = len(positions)
    labels = np.empty((n, C.WINDOW_COLS), dtype=np.uint8)
    for w in range(n):
        for s in range(C.WINDOW_COLS):
            p = (int(positions[w, s, 0]), int(positions[w, s, 1]))
            if p in table:
                labels[w, s] = table[p]
            elif p[1] != 0:
                labels[w, s] = C.LABEL_GAP
            else:
                raise KeyError(f"no label for draft position {p}")
    keep = (~(labels == C.LABEL_UNKNOWN).any(axis=1)).astype(np.uint8)
    return labels, keep


def dict_span(a, start, end):
    """(sub_start, sub_end) as _generate_train computes them, or None."""
    from roko_amd.labels import get_pos_and_labels

    t_pos, t_labels = get_pos_and_labels(a, start, end)
    known = sorted(p for p, l in zip(t_pos, t_labels)
                   if l != C.LABEL_UNKNOWN)
    if not known:
        return None
    return known[0][0], known[-1][0]


def oracle_spans(case, start, end):
    """For one region of a case: [(align index into the contig's records,
    clipped align, lo, hi, (sub_start, sub_end) or None)] by the host
    functions, in _generate_train's order."""
    from roko_amd.labels import filter_aligns, get_aligns

    every = get_aligns(case["truth_bam"], case["contig"], 0,
                       case["draft_len"])
    out = []
    for a in filter_aligns(get_aligns(case["truth_bam"], case["contig"],
                                      start, end)):
        index = [i for i, b in enumerate(every)
                 if (b.qname, b.pos) == (a.qname, a.pos)][0]
        out.append((index, a, max(start, a.start), min(end, a.end),
                    dict_span(a, start, end)))
    return out


def window_positions(case, sub_start, sub_end, seed=SEED):
    from roko_amd.ops import _pileup

    pos, _ = _pileup.generate_features(case["reads_bam"], case["contig"],
                                       sub_start, sub_end, seed=seed,
                                       sampler="counter")
    return pos
