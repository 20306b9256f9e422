"""The exact wavefront aligner without a GPU: the C++ route
(`_pileup.wfa_ops`, `_pileup.replay_ops`) against the Python contract in
`roko_amd/wfa.py` and against the unbanded DP, and its public interface in
`accuracy` (seq_stats, assess_polishing, the CLI)."""

import math

import numpy as np
import pytest

from roko_amd import accuracy, wfa
from roko_amd.ops import pileup_ext
from tests.simple_align import EditScript

FIXED = [("AC", "CA", b"XX"), ("", "ACG", b"DDD"), ("ACG", "", b"III"),
         ("", "", b"")]


def _rand(rng, alphabet, n):
    return "".join(rng.choice(list(alphabet), n)) if n else ""


def _edit(rng, alphabet, seq, k):
    s = list(seq)
    for _ in range(k):
        r = int(rng.integers(3))
        p = int(rng.integers(len(s) + 1))
        if r == 0 and s:
            s[min(p, len(s) - 1)] = alphabet[int(rng.integers(len(alphabet)))]
        elif r == 1 and s:
            del s[min(p, len(s) - 1)]
        else:
            s.insert(p, alphabet[int(rng.integers(len(alphabet)))])
    return "".join(s)


def make_pairs(seed=7):
    """2,000 random pairs of length 0-300 over AC and ACGT, three in four
    related by a few edits and the rest unrelated, plus homopolymer pairs and
    the fixed cases."""
    rng = np.random.default_rng(seed)
    pairs = [(q, t) for q, t, _ in FIXED]
    for it in range(2000):
        al = "AC" if it % 2 else "ACGT"
        q = _rand(rng, al, int(rng.integers(0, 301)))
        if it % 4 == 0:
            t = _rand(rng, al, int(rng.integers(0, 301)))
        else:
            t = _edit(rng, al, q, int(rng.integers(0, 13)))[:300]
        pairs.append((q, t))
    for a, b in [(0, 1), (1, 0), (7, 7), (40, 33), (33, 40), (300, 299)]:
        pairs.append(("A" * a, "A" * b))
        pairs.append(("A" * a + "C" * b, "A" * b + "C" * a))
    return pairs


@pytest.fixture(scope="module")
def px():
    return pileup_ext()


@pytest.fixture(scope="module")
def cases(px):
    """(query, target, reference op string) of every pair, computed once."""
    return [(q, t, wfa.reference_ops(q, t)) for q, t in make_pairs()]


def test_fixed_cases(px):
    for q, t, want in FIXED:
        assert wfa.reference_ops(q, t) == want
        assert px.wfa_ops(q, t) == want


def test_cpp_equals_reference_ops(px, cases):
    assert len(cases) >= 2000
    for q, t, want in cases:
        assert px.wfa_ops(q, t) == want, (q, t)


def test_distance_equals_unbanded_dp(px, cases):
    for q, t, want in cases:
        band = max(len(q), len(t), 1)
        assert len(want) == px.align_stats(q, t, band=band)["edit_distance"], \
            (q, t)


def test_distance_3kb_pair(px, rng):
    truth = _rand(rng, "ACGT", 3000)
    draft = EditScript(rng, truth, sub_rate=0.01, ins_rate=0.003,
                       del_rate=0.003).draft
    ops = px.wfa_ops(draft, truth)
    full = px.align_stats(draft, truth, band=max(len(draft), len(truth)))
    assert len(ops) == full["edit_distance"]
    assert ops == wfa.reference_ops(draft, truth)


def _cigar_lengths(cigar):
    qlen = tlen = num = 0
    for ch in cigar:
        if ch.isdigit():
            num = num * 10 + int(ch)
            continue
        qlen += num if ch in "MI" else 0
        tlen += num if ch in "MD" else 0
        num = 0
    return qlen, tlen


def test_replay_invariants(px, cases):
    for q, t, ops in cases:
        r = px.replay_ops(q, t, ops)  # raises unless it ends at (n, m)
        assert r == wfa.replay(q, t, ops)
        assert r["edit_distance"] == len(ops)
        assert r["mismatches"] + r["insertions"] + r["deletions"] == len(ops)
        assert r["insertions"] - r["deletions"] == len(q) - len(t)
        assert r["matches"] == len(q) - r["mismatches"] - r["insertions"]
        assert _cigar_lengths(r["cigar"]) == (len(q), len(t))


def test_replay_rejects_tampered_ops(px, rng):
    truth = _rand(rng, "ACGT", 400)
    q = _edit(rng, "ACGT", truth, 9)
    ops = px.wfa_ops(q, truth)
    assert len(ops) >= 3
    px.replay_ops(q, truth, ops)
    mid = len(ops) // 2
    other = {"X": b"D", "D": b"I", "I": b"D"}[chr(ops[mid])]
    for bad in (ops[:mid] + other + ops[mid + 1:],   # one op changed
                ops[:mid] + ops[mid + 1:],           # one op removed
                ops + b"X", ops + b"D", ops + b"I",  # one op appended
                ops[:mid] + b"M" + ops[mid + 1:]):   # not an op at all
        with pytest.raises(ValueError):
            px.replay_ops(q, truth, bad)
        with pytest.raises(ValueError):
            wfa.replay(q, truth, bad)


def test_align_cpu_route(px, rng):
    truth = _rand(rng, "ACGT", 500)
    q = _edit(rng, "ACGT", truth, 12)
    res = wfa.align(q, truth, device=False)
    assert res["route"] == "cpu"
    assert res["ops"] == px.wfa_ops(q, truth)
    want = px.replay_ops(q, truth, res["ops"])
    assert {k: res[k] for k in want} == want
    assert len(list(wfa.edit_sites(q, truth, res["cigar"]))) == \
        res["edit_distance"]


def test_seq_stats_wfa_matches_banded(rng):
    truth = _rand(rng, "ACGT", 3000)
    draft = EditScript(rng, truth, sub_rate=0.01, ins_rate=0.003,
                       del_rate=0.003).draft
    banded = accuracy.seq_stats(draft, truth)
    exact = accuracy.seq_stats(draft, truth, aligner="wfa")
    assert set(banded) <= set(exact)
    assert exact["edit_distance"] == banded["edit_distance"]
    assert exact["band"] == 0 and exact["aligner"] == "wfa"
    assert exact["route"] in ("cpu", "device")
    n = len(truth)
    assert exact["total_error"] == exact["edit_distance"] / n
    assert exact["mismatch"] + exact["insertion"] + exact["deletion"] == \
        pytest.approx(exact["total_error"], rel=1e-12)
    assert exact["qscore"] == pytest.approx(
        -10 * np.log10(exact["total_error"]))
    both = accuracy.assess_polishing(draft, truth, truth, aligner="wfa")
    assert both["polished"]["edit_distance"] == 0
    assert both["polished"]["qscore"] == float("inf")
    assert both["error_reduction"] == 1.0
    with pytest.raises(ValueError):
        accuracy.seq_stats(draft, truth, aligner="nope")


def test_seq_stats_default_unchanged(px, rng):
    truth = _rand(rng, "ACGT", 2000)
    draft = EditScript(rng, truth, sub_rate=0.01, ins_rate=0.003,
                       del_rate=0.003).draft
    b = min(len(truth), 32 + len(truth) // 20)
    s = px.align_stats(draft, truth, band=b)
    n = len(truth)
    err = s["edit_distance"] / n
    want = {
        "edit_distance": int(s["edit_distance"]),
        "total_error": err,
        "mismatch": s["mismatches"] / n,
        "insertion": s["insertions"] / n,
        "deletion": s["deletions"] / n,
        "qscore": -10.0 * math.log10(err),
        "band": b,
    }
    got = accuracy.seq_stats(draft, truth)
    assert list(got) == list(want)
    assert got == want
    assert got == accuracy.seq_stats(draft, truth, 0, "banded")


def test_cli_wfa_and_errors(rng, tmp_path, capsys):
    from roko_amd.io.fasta import write_fasta

    truths = [("ctgA", _rand(rng, "ACGT", 1500)),
              ("ctgB", _rand(rng, "ACGT", 900))]
    asm = [(name, EditScript(rng, seq, 0.01, 0.003, 0.003).draft)
           for name, seq in truths]
    write_fasta(str(tmp_path / "truth.fasta"), truths)
    write_fasta(str(tmp_path / "asm.fasta"), asm)
    args = [str(tmp_path / "asm.fasta"), str(tmp_path / "truth.fasta")]

    accuracy.main(args)
    banded = capsys.readouterr().out.strip().splitlines()
    errors = tmp_path / "errors.tsv"
    accuracy.main(args + ["--aligner", "wfa", "--errors", str(errors)])
    exact = capsys.readouterr().out.strip().splitlines()
    assert len(exact) == len(banded) == 3
    assert exact[-1] == banded[-1] and exact[-1].startswith("TOTAL:")
    assert [ln.split(":")[0] for ln in exact] == ["ctgA", "ctgB", "TOTAL"]

    rows = [ln.split("\t") for ln in errors.read_text().splitlines()]
    total = 0
    for (name, truth), (_, draft) in zip(truths, asm):
        st = accuracy.seq_stats(draft, truth, aligner="wfa")
        mine = [r for r in rows if r[0] == name]
        assert len(mine) == st["edit_distance"]
        for _, tpos, op, apos in mine:
            assert op in ("X", "I", "D")
            if op == "X":
                assert truth[int(tpos) - 1] != draft[int(apos) - 1]
        total += st["edit_distance"]
    assert len(rows) == total

    with pytest.raises(SystemExit):
        accuracy.main(args + ["--errors", str(errors)])  # banded: refused
    capsys.readouterr()


def test_max_score_exceeded_raises(px, rng):
    truth = _rand(rng, "ACGT", 300)
    q = _edit(rng, "ACGT", truth, 10)
    dist = len(px.wfa_ops(q, truth))
    assert dist >= 2
    assert len(px.wfa_ops(q, truth, max_score=dist)) == dist
    with pytest.raises(RuntimeError):
        px.wfa_ops(q, truth, max_score=dist - 1)
    with pytest.raises(wfa.ScoreLimitError):
        wfa.align(q, truth, device=False, max_score=dist - 1)
    with pytest.raises(wfa.ScoreLimitError):
        wfa.reference_ops(q, truth, max_score=dist - 1)
    assert wfa.align(q, truth, device=False,
                     max_score=dist)["edit_distance"] == dist


@pytest.mark.parametrize("bad", ["AC\x01GT", "AC\nGT", "AC\x7fGT", "ACéGT",
                                 b"AC\x00GT", b"AC\xffGT"])
def test_non_printable_byte_raises(bad):
    good = "ACGT" if isinstance(bad, str) else b"ACGT"
    with pytest.raises(ValueError):
        wfa.align(bad, good)
    with pytest.raises(ValueError):
        wfa.align(good, bad)


def test_schedule_and_table_size():
    it = wfa.chunk_bounds()
    first = [next(it) for _ in range(9)]
    assert first == [64, 192, 448, 960, 1984, 4032, 8128, 12224, 16320]
    assert list(wfa.chunk_bounds(200)) == [64, 192, 448]
    for n, m in [(0, 0), (0, 5), (5, 0), (3, 300), (300, 3), (100, 120)]:
        for s0, s1 in [(0, 1), (0, 64), (64, 192), (2, 7), (100, 130)]:
            want = sum(min(s, m) + min(s, n) + 1 for s in range(s0, s1))
            assert wfa.dir_cells(n, m, s0, s1) == want


def test_small_band_inflates_and_wfa_is_exact(px, rng):
    """ADVICE.md on accuracy.py: the band only grows when the end cell is
    unreachable. Twenty bases missing near the start and twenty extra near
    the end leave the lengths equal, so a narrow band reaches the end cell
    along a path of mismatches and reports it without an error."""
    truth = _rand(rng, "ACGT", 400)
    query = truth[:50] + truth[70:330] + _rand(rng, "ACGT", 20) + truth[330:]
    assert len(query) == len(truth)
    narrow = accuracy.seq_stats(query, truth, band=5)
    exact = accuracy.seq_stats(query, truth, aligner="wfa")
    full = px.align_stats(query, truth, band=len(truth))
    assert exact["edit_distance"] == full["edit_distance"] <= 40
    assert narrow["edit_distance"] > exact["edit_distance"]
