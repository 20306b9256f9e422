"""Polishing edits and their VCF (roko_amd/edits.py, CPU): the edit rule on
hand-written slots, the replay property against stitch_dense on random
arrays, VCF records applied back to the draft by a small parser, and
`polish(..., out_vcf=...)` on the CPU route."""

import numpy as np
import pytest
import torch

from roko_amd import config as C
from roko_amd import features as F
from roko_amd.edits import (EDIT_DTYPE, apply_edits, dense_edits,
                            vcf_records, write_vcf)
from roko_amd.inference import NO_VOTE, SLOTS_PER_POS, infer, stitch_dense
from roko_amd.polish import main as polish_main
from roko_amd.polish import polish
from roko_amd.quality import NO_QUAL
from tests.test_polish import model  # noqa: F401  (the briefly trained model)

CPU = torch.device("cpu")
QUIET = lambda *a, **k: None  # noqa: E731
A, CC, G, T, GAP = 0, 1, 2, 3, C.LABEL_GAP


def _dense(n, votes):
    """maj / qual of an n-base contig from {(pos, ins): (class, qual)}."""
    maj = np.full(n * SLOTS_PER_POS, NO_VOTE, dtype=np.uint8)
    qual = np.full(n * SLOTS_PER_POS, NO_QUAL, dtype=np.uint8)
    for (p, i), (c, q) in votes.items():
        maj[p * SLOTS_PER_POS + i] = c
        qual[p * SLOTS_PER_POS + i] = q
    return maj, qual


def _edits(rows):
    """EDIT_DTYPE array from (pos, ins, 'ref', 'alt', qual) tuples."""
    return np.array([(p, i, ord(r), ord(a), q) for p, i, r, a, q in rows],
                    dtype=EDIT_DTYPE)


def _same(draft, i=0):
    """A vote that calls the draft's own base."""
    return (C.LABEL_ENCODING[draft[i].upper()], 30)


# -- the edit rule on hand-written cases ---------------------------------------

def test_one_substitution():
    draft = "ACGTA"
    votes = {(p, 0): _same(draft, p) for p in range(5)}
    votes[(2, 0)] = (T, 17)
    got = dense_edits(draft, *_dense(5, votes))
    assert got.dtype == EDIT_DTYPE
    assert np.array_equal(got, _edits([(2, 0, "G", "T", 17)]))


def test_vote_deletion_and_uncovered_position_inside_the_window():
    draft = "ACGTAC"
    votes = {(p, 0): _same(draft, p) for p in range(6)}
    votes[(1, 0)] = (GAP, 41)
    del votes[(3, 0)]            # no window covered position 3
    votes[(3, 2)] = (GAP, 9)     # a voted GAP insertion slot: nothing
    got = dense_edits(draft, *_dense(6, votes))
    assert np.array_equal(got, _edits([(1, 0, "C", "*", 41),
                                       (3, 0, "T", "*", NO_QUAL)]))


def test_three_base_insertion():
    draft = "ACGT"
    votes = {(p, 0): _same(draft, p) for p in range(4)}
    votes.update({(1, 1): (G, 12), (1, 2): (G, 13), (1, 3): (A, 14)})
    got = dense_edits(draft, *_dense(4, votes))
    assert np.array_equal(got, _edits([(1, 1, "*", "G", 12),
                                       (1, 2, "*", "G", 13),
                                       (1, 3, "*", "A", 14)]))
    assert apply_edits(draft, got) == "ACGGAGT"


def test_lowercase_equal_is_no_edit_and_draft_n_is_a_substitution():
    draft = "AcgNt"
    votes = {(0, 0): (A, 30), (1, 0): (CC, 30), (2, 0): (T, 22),
             (3, 0): (A, 8), (4, 0): (T, 30)}
    got = dense_edits(draft, *_dense(5, votes))
    assert np.array_equal(got, _edits([(2, 0, "G", "T", 22),
                                       (3, 0, "N", "A", 8)]))
    assert apply_edits(draft, got) == "AcTAt"


def test_insertion_only_slots_before_s0_are_ignored():
    draft = "ACGTAC"
    votes = {(p, 0): _same(draft, p) for p in range(2, 5)}
    votes[(0, 1)] = (T, 5)   # before the first voted ins == 0 slot
    votes[(1, 3)] = (A, 5)
    maj, qual = _dense(6, votes)
    got = dense_edits(draft, maj, qual)
    assert len(got) == 0 and got.dtype == EDIT_DTYPE
    assert stitch_dense(draft, maj) == draft


def test_insertion_at_position_last():
    draft = "ACGTAC"
    votes = {(p, 0): _same(draft, p) for p in range(1, 4)}
    votes[(4, 2)] = (CC, 33)  # the last voted slot: position 4 is uncovered
    maj, qual = _dense(6, votes)
    got = dense_edits(draft, maj, qual)
    assert np.array_equal(got, _edits([(4, 0, "A", "*", NO_QUAL),
                                       (4, 2, "*", "C", 33)]))
    assert apply_edits(draft, got) == stitch_dense(draft, maj) == "ACGTCC"
    votes[(3, 1)] = (G, 2)
    del votes[(4, 2)]         # now an insertion after the last voted base
    maj, qual = _dense(6, votes)
    got = dense_edits(draft, maj, qual)
    assert np.array_equal(got, _edits([(3, 1, "*", "G", 2)]))
    assert apply_edits(draft, got) == stitch_dense(draft, maj) == "ACGTGAC"


def test_no_votes_and_votes_only_in_insertion_slots_are_empty():
    draft = "ACGT"
    for votes in ({}, {(1, 1): (A, 9), (2, 3): (T, 9)}):
        got = dense_edits(draft, *_dense(4, votes))
        assert got.shape == (0,) and got.dtype == EDIT_DTYPE
        assert vcf_records("c", draft, got) == []


def test_shapes_are_checked():
    with pytest.raises(ValueError, match="SLOTS_PER_POS"):
        dense_edits("ACGT", np.zeros(12, np.uint8), np.zeros(12, np.uint8))


# -- random cases ----------------------------------------------------------------

def _random_case(rng):
    """Draft of 50..400 bases with mixed case and Ns; votes over a random
    stretch with uncovered holes, deletions, substitutions, insertions, and
    now and then insertion-only slots before the first voted base."""
    n = int(rng.integers(50, 401))
    letters = rng.choice(list("ACGT"), n)
    letters[rng.random(n) < 0.05] = "N"
    draft = "".join(ch.lower() if lo else ch
                    for ch, lo in zip(letters, rng.random(n) < 0.2))
    maj = np.full((n, SLOTS_PER_POS), NO_VOTE, dtype=np.uint8)
    lo = int(rng.integers(0, n // 3))
    hi = int(rng.integers(2 * n // 3, n + 1))
    own = np.array([max("ACGT".find(ch.upper()), 0) for ch in draft],
                   dtype=np.uint8)
    col0 = own.copy()
    r = rng.random(n)
    col0[r < 0.08] = rng.integers(0, 4, int((r < 0.08).sum()))
    col0[(r >= 0.08) & (r < 0.14)] = GAP
    col0[(r >= 0.14) & (r < 0.20)] = NO_VOTE
    maj[lo:hi, 0] = col0[lo:hi]
    for i in range(1, SLOTS_PER_POS):
        r = rng.random(n)
        col = np.full(n, NO_VOTE, dtype=np.uint8)
        col[r < 0.10 / i] = GAP
        pick = r < 0.05 / i
        col[pick] = rng.integers(0, 4, int(pick.sum()))
        maj[lo:hi, i] = col[lo:hi]
    if lo > 2 and rng.random() < 0.5:
        maj[lo - 1, 1] = A
        maj[lo - 2, 3] = GAP
    if rng.random() < 0.3 and hi < n:
        maj[hi, 2] = T  # the last voted slot is an insertion slot
    maj = maj.reshape(-1)
    qual = np.where(maj == NO_VOTE, NO_QUAL,
                    rng.integers(0, 61, len(maj))).astype(np.uint8)
    return draft, maj, qual


@pytest.fixture(scope="module")
def random_cases():
    rng = np.random.default_rng(77)
    return [_random_case(rng) for _ in range(200)]


def test_replaying_the_edits_gives_the_stitch(random_cases):
    kinds = set()
    for draft, maj, qual in random_cases:
        e = dense_edits(draft, maj, qual)
        assert apply_edits(draft, e).upper() == stitch_dense(draft, maj).upper()
        assert np.all(np.diff(e["pos"] * 4 + e["ins"]) > 0)  # slot order
        for row in e:
            kinds.add("ins" if row["ins"] else
                      "nocov" if row["qual"] == NO_QUAL else
                      "del" if row["alt"] == ord("*") else "sub")
        s = e["pos"] * 4 + e["ins"]
        voted = maj[s] != NO_VOTE
        assert np.array_equal(e["qual"][voted], qual[s][voted])
    assert kinds == {"ins", "nocov", "del", "sub"}


# -- VCF ---------------------------------------------------------------------------

def _parse_vcf(path):
    """(header lines, [(chrom, pos, ref, alt, qual, info)])."""
    header, recs = [], []
    with open(path) as fh:
        for line in fh:
            line = line.rstrip("\n")
            if line.startswith("#"):
                header.append(line)
                continue
            chrom, pos, vid, ref, alt, qual, flt, info = line.split("\t")
            assert vid == "." and flt == "."
            recs.append((chrom, int(pos), ref, alt, int(qual), info))
    return header, recs


def _apply_vcf(draft, recs):
    """Apply one contig's records to draft.upper(); REF must match the draft
    at POS and records must not overlap."""
    src, out, at = draft.upper(), [], 0
    for _, pos, ref, alt, _, _ in recs:
        start = pos - 1
        assert start >= at, "records overlap or are out of order"
        assert src[start:start + len(ref)] == ref, "REF does not match"
        assert ref and alt and ref != alt
        out.append(src[at:start])
        out.append(alt)
        at = start + len(ref)
    out.append(src[at:])
    return "".join(out)


def _round_trip(tmp_path, draft, maj, qual, name="c"):
    e = dense_edits(draft, maj, qual)
    path = str(tmp_path / "x.vcf")
    n = write_vcf(path, [(name, len(draft))], vcf_records(name, draft, e))
    header, recs = _parse_vcf(path)
    assert n == len(recs)
    assert _apply_vcf(draft, recs) == stitch_dense(draft, maj).upper()
    return e, header, recs


def test_vcf_applied_to_the_draft_gives_the_stitch(random_cases, tmp_path):
    n_recs = n_anchor = 0
    for draft, maj, qual in random_cases:
        e, _, recs = _round_trip(tmp_path, draft, maj, qual)
        # every edit is in one record, but for clusters that cancel out
        assert sum(int(r[5].split(";")[0][3:]) for r in recs) <= len(e)
        n_recs += len(recs)
        n_anchor += sum(len(r[2]) != len(r[3]) for r in recs)
    assert n_recs > 1000 and n_anchor > 100


def test_vcf_deletion_at_position_zero_takes_the_trailing_anchor(tmp_path):
    draft = "ACGTAC"
    votes = {(p, 0): _same(draft, p) for p in range(6)}
    votes[(0, 0)] = (GAP, 25)
    votes[(1, 0)] = (GAP, 19)
    _, _, recs = _round_trip(tmp_path, draft, *_dense(6, votes))
    assert recs == [("c", 1, "ACG", "G", 19, "NE=2")]


def test_vcf_records_by_kind(tmp_path):
    draft = "ACGTACGT"
    votes = {(p, 0): _same(draft, p) for p in range(8)}
    votes[(1, 0)] = (T, 11)                    # substitution
    votes[(3, 0)] = (GAP, 40)                  # deletion, anchored on G
    votes[(5, 1)] = (A, 7)                     # insertion after C
    votes[(5, 2)] = (A, 6)
    _, _, recs = _round_trip(tmp_path, draft, *_dense(8, votes))
    assert recs == [("c", 2, "C", "T", 11, "NE=1"),
                    ("c", 3, "GT", "G", 40, "NE=1"),
                    ("c", 6, "C", "CAA", 6, "NE=2")]


def test_vcf_one_record_for_a_long_uncovered_run(tmp_path):
    rng = np.random.default_rng(3)
    draft = "".join(rng.choice(list("ACGT"), 1300))
    votes = {(p, 0): _same(draft, p) for p in range(1300)
             if not 150 <= p < 1150}
    e, _, recs = _round_trip(tmp_path, draft, *_dense(1300, votes))
    assert len(e) == 1000
    assert recs == [("c", 150, draft[149:1150], draft[149], 0,
                     "NE=1000;NOCOV")]


def test_vcf_header_and_contig_order(tmp_path):
    path = str(tmp_path / "h.vcf")
    recs = [("zeta", 5, "A", "C", 30, "NE=1"),
            ("alpha", 2, "GT", "G", 0, "NE=1;NOCOV")]
    assert write_vcf(path, [("zeta", 40), ("bare", 7), ("alpha", 9)],
                     recs) == 2
    header, got = _parse_vcf(path)
    assert header[0] == "##fileformat=VCFv4.2"
    assert [h for h in header if h.startswith("##contig")] == [
        "##contig=<ID=zeta,length=40>", "##contig=<ID=bare,length=7>",
        "##contig=<ID=alpha,length=9>"]
    assert sum(h.startswith("##INFO=<ID=NE,Number=1,Type=Integer")
               for h in header) == 1
    assert sum(h.startswith("##INFO=<ID=NOCOV,Number=0,Type=Flag")
               for h in header) == 1
    assert header[-1] == "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"
    assert got == recs


# -- polish / infer on the CPU route -------------------------------------------------

def _read(path):
    with open(path, "rb") as fh:
        return fh.read()


def test_polish_vcf_on_the_cpu_route(tiny_assembly, model, tmp_path):  # noqa: F811
    cfg = F.FeatureConfig(region_size=1500, region_overlap=300, seed=5)
    draft = tiny_assembly["draft"]
    fasta, vcf = str(tmp_path / "p.fasta"), str(tmp_path / "p.vcf")
    plain_fasta = str(tmp_path / "plain.fasta")
    got = polish(tiny_assembly["draft_fasta"], tiny_assembly["reads_bam"],
                 None, fasta, workers=1, batch_size=32, cfg=cfg, device=CPU,
                 model=model, log=QUIET, out_vcf=vcf)
    plain = polish(tiny_assembly["draft_fasta"], tiny_assembly["reads_bam"],
                   None, plain_fasta, workers=1, batch_size=32, cfg=cfg,
                   device=CPU, model=model, log=QUIET)
    assert got == plain and _read(fasta) == _read(plain_fasta)
    header, recs = _parse_vcf(vcf)
    assert len(recs) > 0 and got["ctg1"] != draft
    assert f"##contig=<ID=ctg1,length={len(draft)}>" in header
    assert _apply_vcf(draft, recs) == got["ctg1"].upper()

    # the two-step route and the command lines write the same VCF
    rkw = str(tmp_path / "infer.rkw")
    F.run(tiny_assembly["draft_fasta"], tiny_assembly["reads_bam"], rkw,
          workers=1, cfg=cfg, log=QUIET)
    two_vcf = str(tmp_path / "t.vcf")
    want = infer(rkw, None, None, batch_size=32, device=CPU, model=model,
                 log=QUIET, out_vcf=two_vcf)
    assert want == got and _read(two_vcf) == _read(vcf)


def test_vcf_cli_and_a_contig_without_reads(tiny_assembly, model, rng,  # noqa: F811
                                            tmp_path, monkeypatch):
    """`--vcf` of both command lines against the function, on the CPU (the
    GPU is hidden: the CLIs pick their device themselves), over a draft with
    a second contig that no read touches: no records, but a ##contig line."""
    from roko_amd.inference import main as infer_main
    from roko_amd.io.bamio import write_bam
    from roko_amd.io.fasta import write_fasta

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
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
    ckpt = str(tmp_path / "m.pth")
    torch.save(model.state_dict(), ckpt)

    want_vcf = str(tmp_path / "fn.vcf")
    got = polish(draft_fasta, bam, ckpt, None, workers=1, batch_size=32,
                 cfg=F.FeatureConfig(seed=3), device=CPU, log=QUIET,
                 out_vcf=want_vcf)
    header, recs = _parse_vcf(want_vcf)
    assert [h for h in header if h.startswith("##contig")] == [
        f"##contig=<ID=ctg1,length={len(es.draft)}>",
        "##contig=<ID=ctg2,length=700>"]
    assert recs and {r[0] for r in recs} == {"ctg1"}
    assert _apply_vcf(es.draft, recs) == got["ctg1"].upper()
    assert got["ctg2"] == bare

    cli_vcf = str(tmp_path / "cli.vcf")
    polish_main([draft_fasta, bam, ckpt, str(tmp_path / "cli.fasta"),
                 "--t", "1", "--b", "32", "--seed", "3", "--vcf", cli_vcf])
    assert _read(cli_vcf) == _read(want_vcf)
    rkw = str(tmp_path / "infer.rkw")
    F.run(draft_fasta, bam, rkw, workers=1, cfg=F.FeatureConfig(seed=3),
          log=QUIET)
    inf_vcf = str(tmp_path / "inf.vcf")
    infer_main([rkw, ckpt, str(tmp_path / "inf.fasta"), "--b", "32",
                "--vcf", inf_vcf])
    assert _read(inf_vcf) == _read(want_vcf)


def test_infer_vcf_is_single_process(tiny_assembly, model, tmp_path,  # noqa: F811
                                     monkeypatch):
    import roko_amd.inference as inference

    rkw = str(tmp_path / "infer.rkw")
    F.run(tiny_assembly["draft_fasta"], tiny_assembly["reads_bam"], rkw,
          workers=1, log=QUIET)
    monkeypatch.setattr(inference, "init_distributed", lambda: (0, 0, 2))
    with pytest.raises(ValueError, match="single-process"):
        infer(rkw, None, None, device=CPU, model=model, log=QUIET,
              out_vcf=str(tmp_path / "x.vcf"))
