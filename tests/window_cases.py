"""Small BAMs for the window-builder tests (test_sampler_counter.py,
test_gpu_windows.py), written with roko_amd.io.bamio. Every builder returns
(bam path, contig, start, end)."""

from __future__ import annotations

import re

import numpy as np

from roko_amd.io.bamio import SamRecord, write_bam


def parse_cigar(text):
    return [(int(n), op) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", text)]


def read(rng, name, pos, cigar, flag=0, mapq=60, alphabet="ACGT", tid=0):
    """A SamRecord with a random sequence of the CIGAR's query length."""
    cig = parse_cigar(cigar) if isinstance(cigar, str) else list(cigar)
    qlen = sum(l for l, op in cig if op in "MIS=X")
    seq = "".join(alphabet[int(i)] for i in rng.integers(0, len(alphabet), qlen))
    return SamRecord(name, flag, tid, pos, mapq, cig, seq)


def _write(path, refs, reads):
    reads.sort(key=lambda r: (r.tid, r.pos))
    write_bam(str(path), refs, reads)
    return str(path)


def crafted(tmp_path):
    """600 bp contig, region [100, 500): every CIGAR shape the builder has a
    rule for, both strands, N/IUPAC bases, reads across both region ends,
    insertions at start-1 and end-1, and reads each filter drops."""
    rng = np.random.default_rng(101)
    R = []
    # background so that every position of the region is covered
    for i in range(6):
        R.append(read(rng, f"bg{i}", 0, "600M", flag=16 if i % 2 else 0))
    R += [
        # starts before `start`; insertion of 2, deletion
        read(rng, "before", 50, "200M2I100M3D150M"),
        # reverse; soft clip; insertions of 1, 5 (cap 3), 4; = and X ops
        read(rng, "rev_ops", 90, "10S9M1I100M5I50M4I60=2X100M", flag=16),
        # leading insertion: attaches nowhere
        read(rng, "lead_ins", 120, "3I100M"),
        # insertion after a deletion: dropped
        read(rng, "ins_after_del", 150, "50M2D2I60M", flag=16),
        # N-skip (no events inside), then an insertion of 1
        read(rng, "skip", 130, "40M20N40M1I30M"),
        # insertion after an N-skip, and after a soft clip: attach nowhere
        read(rng, "ins_after_skip", 140, "30M10N2I30M"),
        read(rng, "ins_after_clip", 160, "5S2I50M", flag=16),
        # hard clip and pad; an I behind a P is not behind an M
        read(rng, "clip_pad", 200, "5H50M2P1I40M"),
        # N and IUPAC bases, also inside an insertion
        read(rng, "iupac", 210, "60M3I60M", alphabet="ACGTNRYACGT"),
        read(rng, "iupac_rev", 230, "30M2I30M1D30M", flag=16,
             alphabet="ANCNGNTNK"),
        # ends after `end`
        read(rng, "after", 420, "150M", flag=16),
        # insertion behind position end-1 = 499: kept
        read(rng, "ins_at_end", 450, "50M2I60M"),
        # insertion behind position start-1 = 99: outside the region
        read(rng, "ins_before_start", 60, "40M3I100M"),
        # insertions of every length 1..5 at distinct positions
        read(rng, "ins_lengths", 240, "20M1I20M2I20M3I20M4I20M5I20M"),
        read(rng, "ins_lengths_rev", 250, "25M5I25M4I25M3I25M2I25M1I25M",
             flag=16),
        # 14 more columns: the region then has 90 + 12 * 30 columns, so the
        # last window ends on the insertion behind position 499
        read(rng, "pad", 400, "10M3I10M3I10M3I10M3I10M2I10M", flag=16),
        # a proper pair is kept
        read(rng, "proper", 300, "100M", flag=0x1 | 0x2),
        # dropped by the filters
        read(rng, "f_secondary", 110, "100M5I100M", flag=0x100),
        read(rng, "f_unmapped", 115, "100M", flag=0x4),
        read(rng, "f_dup", 125, "100M", flag=0x400),
        read(rng, "f_mapq", 135, "100M4I100M", mapq=5),
        read(rng, "f_improper", 145, "100M3I100M", flag=0x1),
    ]
    return _write(tmp_path / "crafted.bam", [("ctg1", 600), ("empty", 400)],
                  R), "ctg1", 100, 500


def empty_windows(tmp_path):
    """[300, 600) is covered by one all-N read only: the windows inside it
    have no valid read and are skipped; windows on both sides are not."""
    rng = np.random.default_rng(102)
    R = [read(rng, f"l{i}", 0, "300M", flag=16 if i % 2 else 0)
         for i in range(5)]
    R.append(read(rng, "all_n", 250, "400M", alphabet="N"))
    R += [read(rng, f"r{i}", 600, "400M", flag=16 if i % 2 else 0)
          for i in range(5)]
    return _write(tmp_path / "empty.bam", [("ctg1", 1000)], R), "ctg1", 0, 1000


def wide(tmp_path):
    """One window whose valid list has 300 reads (more than 256)."""
    rng = np.random.default_rng(103)
    R = [read(rng, f"w{i}", i % 50, "45M", flag=16 if i % 3 == 0 else 0)
         for i in range(300)]
    return _write(tmp_path / "wide.bam", [("ctg1", 100)], R), "ctg1", 0, 100


def long_cigar(tmp_path):
    """One read with 1201 CIGAR ops over a few plain reads."""
    rng = np.random.default_rng(104)
    cig = []
    for i in range(300):
        cig += [(3, "M"), (1 + i % 4, "I"), (2, "M"), (1 + i % 2, "D")]
    cig.append((5, "M"))
    span = sum(l for l, op in cig if op in "MD")
    R = [read(rng, "long", 10, cig, flag=16)]
    R += [read(rng, f"bg{i}", 0, f"{span + 40}M") for i in range(3)]
    return (_write(tmp_path / "long.bam", [("ctg1", span + 40)], R), "ctg1",
            0, span + 40)


def random_region(tmp_path, seed):
    """3 kb at 20x: noisy draft, 400 bp reads aligned through the edit
    script (the generator of the e2e tests); a sub-range region."""
    from tests.simple_align import BASES, EditScript

    rng = np.random.default_rng(seed)
    truth = "".join(BASES[int(b)] for b in rng.integers(0, 4, 3000))
    es = EditScript(rng, truth, sub_rate=0.02, ins_rate=0.02, del_rate=0.02)
    R = []
    for i in range(20 * len(truth) // 400):
        s = int(rng.integers(0, len(truth) - 400))
        rec = es.align_substring(f"read{i}", s, s + 400,
                                 flag=16 if i % 2 else 0)
        if rec is not None:
            R.append(rec)
    n = len(es.draft)
    return (_write(tmp_path / f"random{seed}.bam", [("ctg1", n)], R), "ctg1",
            50 * (seed % 3), n - 70 * (seed % 2))
