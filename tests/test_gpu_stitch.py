"""The stitch on the GPU (ops/hip/stitch.hip) against the numpy contract:
`DeviceVotes.stitch` must equal `stitch_filtered` over the same tables'
`consensus_quality`, both strings exactly; tables without quality, errors, and
`--stitch device` end to end over the device routes.

The stitch kernels give one thread a draft position and one 256-thread
workgroup 256 positions (at most 1024 output bytes); the scan kernel takes
1024 workgroup counts a pass. The contig lengths below are chosen against
those two numbers."""

import numpy as np
import pytest
import torch

from roko_amd import config as C
from tests.test_gpu_edits import (GAP, QUIET, SCAN_PASS, STAR, TILE, _draft,
                                  _own, _read, _tables)
from tests.test_gpu_edits import case  # noqa: F401  (3 kb case, trained model)

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs ROCm GPU"
)

FILTERS = [(q, k) for q in (0, 30, 60) for k in (False, True)]


def _check(dv, draft, min_qual=0, keep_uncovered=False, ref=None):
    """stitch() against the contract; returns the pair of strings. `ref` is
    the tables' consensus_quality, fetched once per set of tables."""
    from roko_amd.stitch import stitch_filtered

    maj, qual = ref if ref is not None else dv.consensus_quality("c")
    want = stitch_filtered(draft, maj, qual, min_qual, keep_uncovered)
    got = dv.stitch("c", draft, min_qual, keep_uncovered)
    assert len(got[0]) == len(want[0])
    assert got[0] == want[0]
    assert got[1] == want[1]
    return got


# -- the kernels against the contract --------------------------------------------

@pytest.fixture(scope="module")
def mixed():
    """700 bases: three workgroups, the last ragged; lowercase and N in the
    draft; slots hit 1 to 6 times with random classes; an uncovered run across
    the 256-position boundary; votes from position 5 to 689."""
    rng = np.random.default_rng(21)
    n = 700
    draft = _draft(rng, n)
    own = _own(draft)
    slots, classes = [], []
    for p in range(5, 690):
        if 250 <= p < 263 or rng.random() < 0.04:
            continue  # uncovered
        for i in range(4):
            if i and rng.random() > 0.3:
                continue
            hits = int(rng.integers(1, 7))
            for _ in range(hits):
                if i == 0:
                    c = own[p] if rng.random() < 0.6 else rng.integers(0, 5)
                else:
                    c = GAP if rng.random() < 0.5 else rng.integers(0, 4)
                slots.append(p * 4 + i)
                classes.append(int(c))
    dv = _tables(rng, n, slots, classes)
    return dv, draft, dv.consensus_quality("c")


@requires_gpu
@pytest.mark.parametrize("min_qual,keep", FILTERS)
def test_mixed_edits_over_three_workgroups(mixed, min_qual, keep):
    from roko_amd.edits import dense_edits, is_uncovered
    from roko_amd.stitch import applied

    dv, draft, ref = mixed
    seq, _ = _check(dv, draft, min_qual, keep, ref)
    e = dense_edits(draft, *ref)
    nocov = is_uncovered(e)
    assert set(range(250, 263)) <= set(e["pos"][nocov].tolist())
    if min_qual == 30:
        # the threshold splits every kind of edit: it is not vacuous
        ok = applied(e, 30, keep)
        kinds = {"sub": (e["ins"] == 0) & (e["alt"] != STAR),
                 "del": (e["ins"] == 0) & (e["alt"] == STAR) & ~nocov,
                 "ins": e["ins"] > 0}
        for name, kind in kinds.items():
            assert (kind & ok).sum() >= 3, name
            assert (kind & ~ok).sum() >= 3, name
    if keep:
        short = dv.stitch("c", draft, min_qual, False)[0]
        assert len(seq) - len(short) == int(nocov.sum()) >= 13


@requires_gpu
def test_every_slot_emits():
    """600 bases, every ins == 0 slot called a base and every ins > 0 slot
    too: 4 bytes from every thread, 1024 from every full workgroup, the
    largest offsets the workgroups can have."""
    rng = np.random.default_rng(22)
    n = 600
    draft = _draft(rng, n, ns=0.0)
    dv = _tables(rng, n, np.arange(n * 4), rng.integers(0, 4, n * 4))
    seq, qual = _check(dv, draft)
    assert len(seq) == len(qual) == 4 * n
    ref = dv.consensus_quality("c")
    _check(dv, draft, 30, True, ref)


@requires_gpu
def test_every_deletion_rejected():
    """600 bases whose every ins == 0 call is a deletion with all-zero
    quality units, so quality 0: at min_qual = 60 every one is rejected and
    the draft comes back as it is, at Q0; at 0 nothing is left."""
    from roko_amd.ops.votes import DeviceVotes

    rng = np.random.default_rng(23)
    n = 600
    draft = _draft(rng, n)
    pos = np.stack([np.arange(n), np.zeros(n)], axis=1).astype(np.int32)
    dv = DeviceVotes({"c": n}, quality=True)
    dv.scatter("c", np.full(n, GAP, np.uint8), pos,
               np.zeros((n, C.NUM_CLASSES), np.uint8))
    ref = dv.consensus_quality("c")
    assert _check(dv, draft, 60, False, ref) == (draft, "!" * n)
    assert _check(dv, draft, 1, True, ref) == (draft, "!" * n)
    assert _check(dv, draft, 0, False, ref) == ("", "")


@requires_gpu
@pytest.mark.parametrize("min_qual,keep", [(0, False), (30, True)])
def test_edges_first_and_last_base(min_qual, keep):
    """Votes from position 0 through len - 1, a deletion at position 0 and an
    insertion after the last base; 300 bases, the second workgroup ragged."""
    rng = np.random.default_rng(24)
    n = 300
    draft = _draft(rng, n, ns=0.0)
    slots = np.concatenate([np.arange(n) * 4, [(n - 1) * 4 + 1]])
    classes = np.concatenate([_own(draft), [2]])
    classes[0] = GAP
    dv = _tables(rng, n, slots, classes)
    seq, _ = _check(dv, draft, min_qual, keep)
    if min_qual == 0:
        assert seq == draft[1:].upper() + "G"


@requires_gpu
@pytest.mark.parametrize("which", ["equal", "none", "untouched", "ins_only"])
def test_nothing_to_stitch(which):
    from roko_amd.ops.votes import DeviceVotes

    rng = np.random.default_rng(25)
    n = 600
    draft = _draft(rng, n, ns=0.0)
    if which == "equal":      # every call is the draft's base; GAP insertions
        slots = np.concatenate([np.arange(n) * 4, np.arange(0, n, 3) * 4 + 1])
        classes = np.concatenate([_own(draft), np.full(len(slots) - n, GAP)])
        dv = _tables(rng, n, slots, classes)
    elif which == "none":     # a table that exists and holds no vote
        dv = DeviceVotes({"c": n}, quality=True)
        dv.scatter("c", np.zeros(8, np.uint8), np.full((8, 2), -1, np.int32),
                   np.zeros((8, 5), np.uint8))
        assert dv.has_votes("c")
    elif which == "untouched":  # no table at all
        dv = DeviceVotes({"c": n}, quality=True)
    else:                    # votes only in ins > 0 slots
        slots = np.arange(n)[:, None] * 4 + np.array([1, 2, 3])
        slots = slots.reshape(-1)[rng.random(3 * n) < 0.5]
        dv = _tables(rng, n, slots, rng.integers(0, 5, len(slots)))
    for min_qual, keep in ((0, False), (60, True)):
        seq, qual = dv.stitch("c", draft, min_qual, keep)
        assert seq == (draft.upper() if which == "equal" else draft)
        assert len(qual) == n
        if which != "equal":
            assert qual == "!" * n
        if which != "untouched":
            _check(dv, draft, min_qual, keep)


@requires_gpu
def test_more_workgroups_than_one_scan_pass():
    """300,000 bases: 1,172 workgroup counts, more than one 1024-wide pass of
    the scan kernel. About 1% of the positions are edits, with emitters forced
    on both sides of workgroup 1024 * 256; a polished prefix and suffix of
    several hundred draft bases and a 100-position uncovered run."""
    from roko_amd.edits import dense_edits, is_uncovered

    rng = np.random.default_rng(26)
    n = 300_000
    assert -(-n // TILE) > SCAN_PASS
    draft = _draft(rng, n, lower=0.1, ns=0.01)
    own = _own(draft)
    classes = own.copy()
    edit = rng.random(n) < 0.01
    boundary = SCAN_PASS * TILE
    edit[[boundary - 1, boundary, boundary - TILE, boundary + TILE - 1]] = True
    classes[edit] = (own[edit] + 1 + rng.integers(0, 4, int(edit.sum()))) % 5
    # votes from position 700 to n - 901; an insertion-only slot before them
    # (ignored) and one 100 positions after them (the window reaches it, the
    # positions between are uncovered)
    voted = np.arange(700, n - 900)
    ins = np.flatnonzero(rng.random(n) < 0.002)
    ins = ins[(ins >= 700) & (ins < n - 900)]
    ins = np.union1d(ins, [boundary - 1, boundary])
    slots = np.concatenate([voted * 4, ins * 4 + 2,
                            [300 * 4 + 1, (n - 800) * 4 + 3]])
    classes = np.concatenate([classes[voted], rng.integers(0, 4, len(ins)),
                              [1, 2]])
    dv = _tables(rng, n, slots, classes)
    ref = dv.consensus_quality("c")
    e = dense_edits(draft, *ref)
    assert int(is_uncovered(e).sum()) == 101
    assert {boundary - 1, boundary} <= set(e["pos"][e["ins"] == 2].tolist())
    plain, _ = _check(dv, draft, 0, False, ref)
    assert plain[:700] == draft[:700] and plain[-799:] == draft[-799:]
    kept, _ = _check(dv, draft, 30, True, ref)
    assert kept != plain and kept[:700] == draft[:700]


# -- tables without quality, errors ---------------------------------------------------

@requires_gpu
def test_tables_without_quality():
    from roko_amd.inference import stitch_dense
    from roko_amd.ops.votes import DeviceVotes

    rng = np.random.default_rng(27)
    n = 700
    draft = _draft(rng, n)
    p = np.arange(20, 650)
    p = p[rng.random(len(p)) > 0.05]
    slots = np.concatenate([p * 4, p[::7] * 4 + 1])
    classes = np.concatenate([np.where(rng.random(len(p)) < 0.8, _own(draft)[p],
                                       rng.integers(0, 5, len(p))),
                              rng.integers(0, 5, len(p[::7]))])
    pos = np.stack([slots // 4, slots % 4], axis=1).astype(np.int32)
    dv = DeviceVotes({"c": n})
    dv.scatter("c", classes.astype(np.uint8), pos)
    maj = dv.consensus("c")
    want = stitch_dense(draft, maj)
    assert want != draft
    assert dv.stitch("c", draft) == (want, None)
    kept, none = dv.stitch("c", draft, keep_uncovered=True)
    assert none is None and len(kept) > len(want)
    with pytest.raises(RuntimeError, match="quality=True"):
        dv.stitch("c", draft, min_qual=1)
    assert DeviceVotes({"c": n}).stitch("c", draft) == (draft, None)


@requires_gpu
def test_stitch_raises_on_a_tripped_overflow_flag():
    """The set-up of test_gpu_quality's overflow test: 17 votes of 255 units
    on one slot pass the 12-bit field."""
    from roko_amd.ops.votes import DeviceVotes, VoteOverflowError
    from tests.test_gpu_votes import CONTIG_LEN

    positions = np.full((1, C.WINDOW_COLS, 2), -1, dtype=np.int32)
    preds = np.zeros((1, C.WINDOW_COLS), dtype=np.uint8)
    units = np.full((1, C.WINDOW_COLS, C.NUM_CLASSES), 3, dtype=np.uint8)
    positions[0, :17] = [[5, 2]] * 17
    preds[0, :17] = np.arange(17) % C.NUM_CLASSES
    units[0, :, 2] = 255
    dv = DeviceVotes({"c": CONTIG_LEN}, quality=True)
    dv.scatter("c", preds, positions, units)
    with pytest.raises(VoteOverflowError, match="host votes"):
        dv.stitch("c", "A" * CONTIG_LEN)


@requires_gpu
def test_stitch_checks_the_draft_length_and_min_qual():
    from roko_amd.ops.votes import DeviceVotes

    dv = DeviceVotes({"c": 8}, quality=True)
    with pytest.raises(ValueError, match="draft of 7 bases"):
        dv.stitch("c", "ACGTACG")
    with pytest.raises(ValueError, match="min_qual"):
        dv.stitch("c", "ACGTACGT", min_qual=61)


# -- end to end ----------------------------------------------------------------------

@requires_gpu
@pytest.mark.parametrize("kw", [{"min_qual": 5}, {"keep_uncovered": True},
                                {"stitch": "device"}])
def test_infer_filter_with_host_votes_on_a_gpu_raises(case, kw):  # noqa: F811
    from roko_amd.inference import infer

    with pytest.raises(ValueError, match="votes='device'"):
        infer(case["rkw"], None, None, model=case["model"], log=QUIET,
              votes="host", **kw)


@requires_gpu
@pytest.mark.parametrize("route", ["host", "host_counter", "device"])
def test_device_stitch_over_the_device_routes(case, route):  # noqa: F811
    from roko_amd.config import FeatureConfig
    from roko_amd.inference import infer
    from roko_amd.polish import polish
    from tests.test_edits import _apply_vcf, _parse_vcf
    from tests.test_stitch import pick_min_qual

    d, model = case["dir"], case["model"]
    path = lambda name: str(d / f"st_{name}_{route}")  # noqa: E731
    cfg = FeatureConfig(seed=1,
                        sampler="mt19937" if route == "host" else "counter")
    common = dict(workers=1, batch_size=32, model=model, log=QUIET, depth=2,
                  cfg=cfg, extract="device" if route == "device" else "host")

    def run(tag, stitch, **filt):
        out = polish(case["ref"], case["bam"], None, path(f"{tag}.fasta"),
                     out_fastq=path(f"{tag}.fastq"), out_vcf=path(f"{tag}.vcf"),
                     stitch=stitch, **filt, **common)
        return out, [_read(path(f"{tag}.{e}")) for e in ("fasta", "fastq",
                                                         "vcf")]

    host, host_files = run("h", "host")
    dev, dev_files = run("d", "device")
    assert dev == host and dev_files == host_files
    assert host["ctg1"] != case["draft"]

    min_qual = pick_min_qual(_parse_vcf(path("h.vcf"))[1])
    filt = dict(min_qual=min_qual, keep_uncovered=True)
    host_f, host_f_files = run("hf", "host", **filt)
    dev_f, dev_f_files = run("df", "device", **filt)
    assert dev_f == host_f and dev_f_files == host_f_files
    assert host_f["ctg1"] != host["ctg1"]
    header, recs = _parse_vcf(path("df.vcf"))
    assert f"##roko_filter=min_qual={min_qual};keep_uncovered=1" in header
    assert _apply_vcf(case["draft"], recs) == dev_f["ctg1"].upper()

    if route == "host":
        for tag, want, files, kw in (("i", host, host_files, {}),
                                     ("if", host_f, host_f_files, filt)):
            got = infer(case["rkw"], None, path(f"{tag}.fasta"),
                        batch_size=32, model=model, log=QUIET, votes="device",
                        depth=2, out_fastq=path(f"{tag}.fastq"),
                        out_vcf=path(f"{tag}.vcf"), stitch="device", **kw)
            assert got == want
            assert [_read(path(f"{tag}.{e}"))
                    for e in ("fasta", "fastq", "vcf")] == files
