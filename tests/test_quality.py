"""Per-base quality (CPU): the numpy reference of the quality contract
(roko_amd/quality.py) against the formula and hand-made tables, and the FASTQ
output of polish() and infer() on the CPU route."""

import math

import numpy as np
import pytest
import torch

from roko_amd import config as C
from roko_amd import features as F
from roko_amd.inference import (NO_VOTE, SLOTS_PER_POS, accumulate_votes,
                                dense_majority, infer, stitch_dense)
from roko_amd.io.fasta import read_fasta, read_fastq, write_fastq
from roko_amd.polish import main as polish_main
from roko_amd.polish import polish
from tests.test_polish import model  # noqa: F401  (the briefly trained model)

CPU = torch.device("cpu")
QUIET = lambda *a, **k: None  # noqa: E731


def _units_by_formula(z):
    """The contract, evaluated with plain Python floats."""
    m = max(z)
    t = [math.exp(v - m) for v in z]
    out = []
    for k in range(len(z)):
        e = sum(t[j] for j in range(len(z)) if j != k) / sum(t)
        out.append(255 if e == 0 else
                   min(255, math.floor(4 * (-10 * math.log10(e)) + 0.5)))
    return out


def test_phred_units_follow_the_formula():
    from roko_amd.quality import phred_units

    uniform = [0.7] * 5                      # e_k = 0.8 for every class
    ahead = [1.0, -2.0, 31.0, 0.5, 1.0]      # class 2 ahead by 30
    tie = [3.0, -1.0, 3.0, -4.0, 0.0]        # classes 0 and 2 tie
    far = [0.0, 0.0, 0.0, 800.0, 0.0]        # the others underflow: e_3 = 0
    mild = [0.3, 1.9, -0.6, 1.1, 0.2]
    z = np.array([uniform, ahead, tie, far, mild])
    got = phred_units(z)
    assert got.dtype == np.uint8 and got.shape == (5, 5)
    assert got[0].tolist() == [4] * 5
    assert got[1].tolist() == [0, 0, 255, 0, 0]
    assert got[2, 0] == got[2, 2] and got[2, 0] > got[2, 1]
    assert got[3].tolist() == [0, 0, 0, 255, 0]
    for row, want in zip(got, (uniform, ahead, tie, far, mild)):
        assert row.tolist() == _units_by_formula(want)
    # float32 input and leading dimensions
    got32 = phred_units(z.astype(np.float32).reshape(1, 5, 5))
    assert got32.shape == (1, 5, 5)
    np.testing.assert_array_equal(got32[0, :4], got[:4])


def test_accumulate_quality_has_the_keys_of_accumulate_votes(rng):
    from roko_amd.quality import accumulate_quality

    pos = np.stack([rng.integers(0, 40, (7, 90)),
                    rng.integers(0, C.MAX_INS + 1, (7, 90))], axis=2)
    preds = rng.integers(0, C.NUM_CLASSES, (7, 90)).astype(np.uint8)
    units = rng.integers(0, 256, (7, 90, C.NUM_CLASSES)).astype(np.uint8)
    keys, counts = accumulate_votes(pos, preds)
    qkeys, sums = accumulate_quality(pos, units)
    np.testing.assert_array_equal(qkeys, keys)
    assert sums.dtype == np.int64 and sums.shape == counts.shape
    flat_keys = (pos[..., 0].astype(np.int64) << 3 | pos[..., 1]).reshape(-1)
    for i in (0, len(keys) // 2, len(keys) - 1):
        want = units.reshape(-1, C.NUM_CLASSES)[flat_keys == keys[i]] \
            .astype(np.int64).sum(axis=0)
        np.testing.assert_array_equal(sums[i], want)
    assert sums.sum() == units.astype(np.int64).sum()


def test_dense_quality_on_hand_made_slots():
    from roko_amd.quality import NO_QUAL, Q_MAX, dense_quality

    # slot (pos 2, ins 0): votes 1, 1, 3 with class-1 units 200, 180, 8
    # slot (pos 3, ins 1): two confident votes for class 0 -> capped at 60
    keys = np.array([2 << 3 | 0, 3 << 3 | 1], dtype=np.int64)
    counts = np.array([[0, 2, 0, 1, 0], [2, 0, 0, 0, 0]], dtype=np.int64)
    sums = np.array([[5, 388, 0, 130, 9], [510, 0, 0, 0, 0]], dtype=np.int64)
    qual = dense_quality(keys, counts, sums, contig_len=5)
    assert qual.dtype == np.uint8 and qual.shape == (5 * SLOTS_PER_POS,)
    assert qual[2 * SLOTS_PER_POS] == 388 // 12 == 32
    assert qual[3 * SLOTS_PER_POS + 1] == Q_MAX == 60
    rest = np.delete(qual, [2 * SLOTS_PER_POS, 3 * SLOTS_PER_POS + 1])
    assert (rest == NO_QUAL).all() and NO_QUAL == 0xFF
    empty = dense_quality(np.empty(0, np.int64), np.empty((0, 5), np.int64),
                          np.empty((0, 5), np.int64), 3)
    assert (empty == NO_QUAL).all() and len(empty) == 3 * SLOTS_PER_POS


def test_stitch_dense_qual():
    from roko_amd.quality import NO_QUAL, stitch_dense_qual

    draft = "ACGTACGTAC"
    maj = np.full(len(draft) * SLOTS_PER_POS, NO_VOTE, dtype=np.uint8)
    qual = np.full(len(draft) * SLOTS_PER_POS, NO_QUAL, dtype=np.uint8)

    def vote(pos, ins, cls, q):
        maj[pos * SLOTS_PER_POS + ins] = cls
        qual[pos * SLOTS_PER_POS + ins] = q

    vote(1, 2, 0, 50)                # leading insertion-only column: dropped
    vote(3, 0, 2, 10)                # G, Q10
    vote(3, 1, 3, 0)                 # inserted T, Q0
    vote(4, 0, C.LABEL_GAP, 40)      # deleted base: nothing emitted
    vote(5, 0, 1, 60)                # C, Q60
    vote(6, 0, 0, 33)                # A, Q33
    seq, q = stitch_dense_qual(draft, maj, qual)
    assert seq == stitch_dense(draft, maj) == "ACG" + "GTCA" + "TAC"
    assert len(q) == len(seq)
    assert q == "!!!" + "+!]B" + "!!!"
    # no votes at all, and insertion-only votes: the draft, all Q0
    none = np.full_like(maj, NO_VOTE)
    assert stitch_dense_qual(draft, none, qual) == (draft, "!" * len(draft))
    ins_only = none.copy()
    ins_only[2 * SLOTS_PER_POS + 1] = 1
    assert stitch_dense_qual(draft, ins_only, qual) == \
        (draft, "!" * len(draft))


def test_streaming_form_equals_one_shot(rng):
    from roko_amd.quality import StreamingQualityVotes, accumulate_quality

    pos = np.stack([rng.integers(0, 30, (11, 90)),
                    rng.integers(0, C.MAX_INS + 1, (11, 90))], axis=2)
    preds = rng.integers(0, C.NUM_CLASSES, (11, 90)).astype(np.uint8)
    units = rng.integers(0, 256, (11, 90, C.NUM_CLASSES)).astype(np.uint8)
    sv = StreamingQualityVotes(chunk_windows=4)  # two folds and a remainder
    for i in range(11):
        sv.add("c", pos[i], preds[i], units[i])
    tables, sums = sv.finalize()
    for got, want in ((tables["c"], accumulate_votes(pos, preds)),
                      (sums["c"], accumulate_quality(pos, units))):
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])


def test_fastq_round_trip(tmp_path):
    path = str(tmp_path / "sub" / "x.fastq")
    recs = [("a", "ACGT", "!+5]"), ("b desc", "", ""), ("c", "@+AC", "@+!!")]
    write_fastq(path, recs)
    with open(path) as fh:
        assert fh.read() == "@a\nACGT\n+\n!+5]\n@b desc\n\n+\n\n@c\n@+AC\n+\n@+!!\n"
    assert list(read_fastq(path)) == [("a", "ACGT", "!+5]"), ("b", "", ""),
                                      ("c", "@+AC", "@+!!")]
    with pytest.raises(ValueError, match="qualities"):
        write_fastq(path, [("a", "ACGT", "!!")])


def _read(path):
    with open(path, "rb") as fh:
        return fh.read()


def test_polish_fastq_equals_fasta_and_two_step(tiny_assembly, model,  # noqa: F811
                                                tmp_path):
    cfg = F.FeatureConfig(region_size=1500, region_overlap=300, seed=5)
    fasta, fastq = str(tmp_path / "p.fasta"), str(tmp_path / "p.fastq")
    got = polish(tiny_assembly["draft_fasta"], tiny_assembly["reads_bam"],
                 None, fasta, workers=1, batch_size=32, cfg=cfg, device=CPU,
                 model=model, log=QUIET, out_fastq=fastq)
    plain = polish(tiny_assembly["draft_fasta"], tiny_assembly["reads_bam"],
                   None, None, workers=1, batch_size=32, cfg=cfg, device=CPU,
                   model=model, log=QUIET)
    assert got == plain  # the sequence does not depend on the quality output
    assert got["ctg1"] != tiny_assembly["draft"]
    recs = list(read_fastq(fastq))
    assert [(n, s) for n, s, _ in recs] == list(read_fasta(fasta))
    assert recs[0][1] == got["ctg1"]
    quals = recs[0][2]
    assert len(quals) == len(got["ctg1"])
    assert all("!" <= ch <= chr(33 + 60) for ch in quals)
    assert len(set(quals)) >= 3

    rkw = str(tmp_path / "infer.rkw")
    F.run(tiny_assembly["draft_fasta"], tiny_assembly["reads_bam"], rkw,
          workers=1, cfg=cfg, log=QUIET)
    two_fasta, two_fastq = (str(tmp_path / "t.fasta"),
                            str(tmp_path / "t.fastq"))
    want = infer(rkw, None, two_fasta, batch_size=32, device=CPU, model=model,
                 log=QUIET, out_fastq=two_fastq)
    assert want == got
    assert _read(two_fastq) == _read(fastq)
    assert _read(two_fasta) == _read(fasta)


def test_contig_without_reads_is_draft_with_q0(tiny_assembly, model, rng,  # noqa: F811
                                               tmp_path):
    from roko_amd.io.bamio import write_bam
    from roko_amd.io.fasta import write_fasta

    es = tiny_assembly["edit_script"]
    truth = tiny_assembly["truth"]
    bare = "".join(rng.choice(list("ACGT"), 700))
    draft_fasta = str(tmp_path / "two.fasta")
    write_fasta(draft_fasta, [("ctg1", es.draft), ("ctg2", bare)])
    reads = []
    for i in range(150):
        s = int(rng.integers(0, len(truth) - 400))
        rec = es.align_substring(f"r{i}", s, s + 400, flag=16 if i % 2 else 0)
        if rec is not None:
            reads.append(rec)
    reads.sort(key=lambda r: (r.tid, r.pos))
    bam = str(tmp_path / "two.bam")
    write_bam(bam, [("ctg1", len(es.draft)), ("ctg2", len(bare))], reads)

    cfg = F.FeatureConfig(region_size=1500, region_overlap=300, seed=2)
    fastq = str(tmp_path / "p.fastq")
    got = polish(draft_fasta, bam, None, None, workers=1, batch_size=32,
                 cfg=cfg, device=CPU, model=model, log=QUIET, out_fastq=fastq)
    recs = {n: (s, q) for n, s, q in read_fastq(fastq)}
    assert recs["ctg2"] == (bare, "!" * len(bare))
    assert recs["ctg1"][0] == got["ctg1"] != es.draft
    assert set(recs["ctg1"][1]) != {"!"}

    rkw = str(tmp_path / "infer.rkw")
    F.run(draft_fasta, bam, rkw, workers=1, cfg=cfg, log=QUIET)
    two_fastq = str(tmp_path / "t.fastq")
    infer(rkw, None, None, batch_size=32, device=CPU, model=model, log=QUIET,
          out_fastq=two_fastq)
    assert _read(two_fastq) == _read(fastq)


def test_fastq_cli_writes_the_same_file(tiny_assembly, model, tmp_path,  # noqa: F811
                                        monkeypatch):
    """`python -m roko_amd.polish --fastq` and `python -m roko_amd.inference
    --fastq` entries against the functions, all on the CPU: the CLIs pick
    their device themselves, so the GPU is hidden from them."""
    from roko_amd.inference import main as infer_main

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    ckpt = str(tmp_path / "m.pth")
    torch.save(model.state_dict(), ckpt)
    want_fastq = str(tmp_path / "fn.fastq")
    polish(tiny_assembly["draft_fasta"], tiny_assembly["reads_bam"], ckpt,
           None, workers=1, batch_size=32, cfg=F.FeatureConfig(seed=3),
           device=CPU, log=QUIET, out_fastq=want_fastq)

    cli_fasta, cli_fastq = (str(tmp_path / "cli.fasta"),
                            str(tmp_path / "cli.fastq"))
    polish_main([tiny_assembly["draft_fasta"], tiny_assembly["reads_bam"],
                 ckpt, cli_fasta, "--t", "1", "--b", "32", "--seed", "3",
                 "--fastq", cli_fastq])
    assert _read(cli_fastq) == _read(want_fastq)
    assert [(n, s) for n, s, _ in read_fastq(cli_fastq)] == \
        list(read_fasta(cli_fasta))

    rkw = str(tmp_path / "infer.rkw")
    F.run(tiny_assembly["draft_fasta"], tiny_assembly["reads_bam"], rkw,
          workers=1, cfg=F.FeatureConfig(seed=3), log=QUIET)
    inf_fastq = str(tmp_path / "inf.fastq")
    infer_main([rkw, ckpt, str(tmp_path / "inf.fasta"), "--b", "32",
                "--fastq", inf_fastq])
    assert _read(inf_fastq) == _read(want_fastq)


def test_infer_fastq_is_single_process(tiny_assembly, model, tmp_path,  # noqa: F811
                                       monkeypatch):
    import roko_amd.inference as inference

    rkw = str(tmp_path / "infer.rkw")
    F.run(tiny_assembly["draft_fasta"], tiny_assembly["reads_bam"], rkw,
          workers=1, log=QUIET)
    monkeypatch.setattr(inference, "init_distributed", lambda: (0, 0, 2))
    with pytest.raises(ValueError, match="single-process"):
        infer(rkw, None, None, device=CPU, model=model, log=QUIET,
              out_fastq=str(tmp_path / "x.fastq"))


def test_dense_forms_agree_with_the_host_stitch(rng):
    """stitch_tables (the host route's FASTQ stitch) returns the sequence of
    stitch_contig on a random table with gaps, insertions and ties."""
    from roko_amd.inference import stitch_contig
    from roko_amd.quality import accumulate_quality, stitch_tables

    draft = "".join(rng.choice(list("ACGT"), 60))
    pos = np.stack([rng.integers(5, 50, (3, 90)),
                    rng.integers(0, C.MAX_INS + 1, (3, 90))], axis=2)
    preds = rng.integers(0, C.NUM_CLASSES, (3, 90)).astype(np.uint8)
    units = rng.integers(0, 256, (3, 90, C.NUM_CLASSES)).astype(np.uint8)
    table = accumulate_votes(pos, preds)
    seq, q = stitch_tables(draft, table, accumulate_quality(pos, units))
    assert seq == stitch_contig(draft, *table)
    assert seq == stitch_dense(draft, dense_majority(*table, len(draft)))
    assert len(q) == len(seq)
