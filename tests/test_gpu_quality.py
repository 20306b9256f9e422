"""Per-base quality on the GPU: the head kernel's quality units, the fused
vote scatter and the quality consensus kernel against the numpy reference
(roko_amd/quality.py; exact integer equality after the one rounding step),
overflow reporting, the serving slot in quality mode, and FASTQ end to end
over the three device routes."""

import numpy as np
import pytest
import torch

from roko_amd import config as C

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs ROCm GPU"
)

QUIET = lambda *a, **k: None  # noqa: E731


# -- head ---------------------------------------------------------------------

@requires_gpu
def test_head_quality_units_match_reference():
    """T=90, B=3: 270 rows, two 256-thread blocks, the second ragged. A third
    of the rows are zero (logits = b4, which holds an exact tie), a third are
    small (near-uniform posteriors), a third are large (one class ahead by
    more than 16, units saturate)."""
    from roko_amd.ops import ext
    from roko_amd.quality import phred_units

    g = torch.Generator().manual_seed(5)
    T, B = 90, 3
    scale = torch.tensor([0.0, 0.005, 3.0]).repeat(T).view(T, B, 1)
    hseq = (torch.randn(T, B, 256, generator=g) * scale).to(torch.bfloat16)
    w4 = torch.randn(5, 256, generator=g).to(torch.bfloat16)
    b4 = torch.tensor([0.25, -0.5, 0.25, 0.0, -0.125])
    args = (hseq.cuda(), w4.cuda(), b4.cuda())
    logits0, amax0 = ext().head_fwd(*args, True, True)
    logits, amax, qv = ext().head_fwd(*args, True, True, True)
    torch.cuda.synchronize()
    assert qv.dtype == torch.uint8 and qv.shape == (B, T, 5)
    # the other outputs do not depend on the quality output
    assert torch.equal(logits, logits0) and torch.equal(amax, amax0)

    ref_logits = (hseq.float().view(T * B, 256) @ w4.float().T + b4) \
        .view(T, B, 5).transpose(0, 1)
    want = phred_units(ref_logits.numpy()).astype(np.int64)
    got = qv.cpu().numpy().astype(np.int64)
    # the inputs do cover the three regimes, one per batch row
    z = np.sort(ref_logits.numpy(), axis=2)  # (B, T, 5)
    assert (z[0, :, 4] == z[0, :, 3]).all()            # exact ties
    assert ((z[1, :, 4] - z[1, :, 0]) < 1.5).all()     # near-uniform
    assert (z[1, :, 4] != z[1, :, 3]).all()
    assert ((z[2, :, 4] - z[2, :, 3]) > 16).sum() > 20  # saturating rows
    assert (want[2] == 255).sum() > 20
    diff = np.abs(got - want)
    print(f"head units: max |diff| {diff.max()}, "
          f"{np.count_nonzero(diff)} of {diff.size} differ")
    # one unit is the rounding step: fp32 against float64 can only move a
    # value across a .5 boundary
    assert diff.max() <= 1
    # tied classes get equal units, whatever the rounding
    assert (got[0, :, 0] == got[0, :, 2]).all()  # the zero rows: logits = b4


# -- scatter ------------------------------------------------------------------

@pytest.fixture(scope="module")
def scattered():
    """The 49-window / 200-base setup of test_gpu_votes.py through the fused
    scatter: two calls (32 windows, then 17), rows with pos = -1, slots hit
    up to 6 times, random classes and random units."""
    from roko_amd.ops.votes import DeviceVotes
    from tests.test_gpu_votes import CONTIG_LEN, _draw_positions

    rng = np.random.default_rng(43)
    positions = _draw_positions(rng, 49, free_tail=15)
    positions[[5, 30, 31, 47, 48]] = -1  # rows that must not vote
    preds = rng.integers(0, C.NUM_CLASSES, (49, C.WINDOW_COLS)).astype(np.uint8)
    units = rng.integers(0, 256, (49, C.WINDOW_COLS, C.NUM_CLASSES)) \
        .astype(np.uint8)
    dv = DeviceVotes({"c": CONTIG_LEN}, quality=True)
    dv.scatter("c", preds[:32], positions[:32], units[:32])
    dv.scatter("c", preds[32:], positions[32:], units[32:])
    return dv, positions, preds, units


@requires_gpu
def test_fused_scatter_matches_host_tables_exactly(scattered):
    from roko_amd.ops.votes import DeviceVotes
    from roko_amd.quality import accumulate_quality
    from tests.test_gpu_votes import CONTIG_LEN, _host_table

    dv, positions, preds, units = scattered
    live = positions[..., 0] >= 0
    keys, counts = _host_table(positions, preds)
    qkeys, sums = accumulate_quality(positions[live][None], units[live][None])
    assert counts.sum(axis=1).max() == 6  # the multiplicity bound is reached
    got_keys, got_counts = dv.counts("c")
    np.testing.assert_array_equal(got_keys, keys)
    np.testing.assert_array_equal(got_counts, counts)
    got_qkeys, got_sums = dv.sums("c")
    assert got_qkeys.dtype == np.int64 and got_sums.dtype == np.int64
    np.testing.assert_array_equal(got_qkeys, qkeys)
    np.testing.assert_array_equal(got_sums, sums)
    # the count table is what the plain scatter produces
    plain = DeviceVotes({"c": CONTIG_LEN})
    plain.scatter("c", preds[:32], positions[:32])
    plain.scatter("c", preds[32:], positions[32:])
    plain.drain()
    assert torch.equal(plain.table("c"), dv.table("c"))


@requires_gpu
def test_quality_overflow_is_reported_not_silent():
    """17 votes on one slot, spread over the classes so that no count nibble
    passes 15, class 2 at 255 units in every vote: 17 x 255 passes the 12-bit
    field. 16 such votes read exactly 4080."""
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
        dv.sums("c")
    with pytest.raises(VoteOverflowError, match="host votes"):
        dv.consensus_quality("c")
    positions[0, 16] = -1
    dv = DeviceVotes({"c": CONTIG_LEN}, quality=True)
    dv.scatter("c", preds, positions, units)
    keys, sums = dv.sums("c")
    assert keys.tolist() == [5 << 3 | 2]
    assert sums.tolist() == [[48, 48, 4080, 48, 48]]
    _, counts = dv.counts("c")
    assert counts.tolist() == [[4, 3, 3, 3, 3]]
    maj, qual = dv.consensus_quality("c")
    assert maj[5 * 4 + 2] == 0 and qual[5 * 4 + 2] == 48 // (4 * 16)


# -- consensus ----------------------------------------------------------------

@requires_gpu
def test_quality_consensus_with_a_partial_last_group():
    """n_slots that is no multiple of the 4-slot vector group, tables built
    on the host, guard words beyond n_slots in both inputs, sentinels beyond
    it in both outputs."""
    from roko_amd.ops import ext
    from roko_amd.quality import dense_quality

    rng = np.random.default_rng(4)
    n_slots = 4 * 300 + 3  # more than one 256-thread block, ragged tail
    cnt = rng.integers(0, 4, (n_slots, C.NUM_CLASSES)).astype(np.int64)
    cnt[rng.random(n_slots) < 0.3] = 0
    n = cnt.sum(axis=1)
    assert n.max() <= 15
    # any sum a slot with n votes can hold: 0 .. 255 n per class
    sums = (rng.random((n_slots, C.NUM_CLASSES)) * (255 * n[:, None] + 1)) \
        .astype(np.int64)
    assert sums.max() < 4096 and (sums // np.maximum(4 * n, 1)[:, None]).max() > 60
    packed = np.zeros(n_slots + 8, dtype=np.uint32)
    qpacked = np.zeros(n_slots + 8, dtype=np.uint64)
    for c in range(C.NUM_CLASSES):
        packed[:n_slots] |= cnt[:, c].astype(np.uint32) << np.uint32(4 * c)
        qpacked[:n_slots] |= sums[:, c].astype(np.uint64) << np.uint64(12 * c)
    packed[n_slots:] = 0x11111  # beyond the tables in use: must be ignored
    qpacked[n_slots:] = 0x0FF0FF0FF0FF0FF
    table = torch.from_numpy(packed.view(np.int32)).cuda()
    qsum = torch.from_numpy(qpacked.view(np.int64)).cuda()
    maj = torch.full((n_slots + 8,), 0x77, dtype=torch.uint8, device="cuda")
    qual = torch.full((n_slots + 8,), 0x77, dtype=torch.uint8, device="cuda")
    maj0 = torch.full((n_slots + 8,), 0x77, dtype=torch.uint8, device="cuda")
    ext().vote_consensus(table, n_slots, maj0)
    ext().vote_consensus_q(table, qsum, n_slots, maj, qual)
    assert torch.equal(maj, maj0)
    got = qual.cpu().numpy()
    slots = np.flatnonzero(n)
    keys = (slots // 4) << 3 | (slots % 4)
    want = dense_quality(keys, cnt[slots], sums[slots], 301)[:n_slots]
    assert (want == 60).any() and (want == 0xFF).any() and (want < 60).any()
    np.testing.assert_array_equal(got[:n_slots], want)
    assert (got[n_slots:] == 0x77).all()
    assert (maj.cpu().numpy()[n_slots:] == 0x77).all()


# -- serving slot and end to end ------------------------------------------------

@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """The 3 kb and 9 kb assemblies and the briefly trained model of
    test_gpu_votes.py."""
    from roko_amd.config import FeatureConfig, TrainConfig
    from roko_amd.features import run as features_run
    from roko_amd.train import train
    from tests.test_gpu_e2e import _make_case

    out = {}
    for ref_len in (3000, 9000):
        d = tmp_path_factory.mktemp(f"qcase{ref_len}")
        case = _make_case(d, ref_len=ref_len, cov=25, seed=7)
        case["rkw"] = str(d / "infer.rkw")
        case["n"] = features_run(case["ref"], case["bam"], case["rkw"],
                                 workers=1, cfg=FeatureConfig(seed=1),
                                 log=QUIET)
        case["dir"] = d
        out[ref_len] = case
    d = out[3000]["dir"]
    train_rkw = str(d / "train.rkw")
    features_run(out[3000]["ref"], out[3000]["bam"], train_rkw,
                 bam_y=out[3000]["truth_bam"], workers=1,
                 cfg=FeatureConfig(seed=1), log=QUIET)
    model, _ = train(train_rkw, str(d / "ckpt"),
                     cfg=TrainConfig(batch_size=32, epochs=12, lr=2e-3,
                                     seed=0),
                     log=QUIET)
    out["model"] = model.eval()
    return out


@requires_gpu
def test_quality_slot_padding_rows_add_nothing(cases):
    """Slot batch 32, depth 1, quality=True: 32 windows, then 17 into the
    same slot. The slot's own amax and qv, read back, give the expected
    tables; rows 17..32 of the second run are stale and add nothing."""
    from roko_amd.ops.forward import InferencePipeline
    from roko_amd.ops.votes import DeviceVotes
    from roko_amd.quality import accumulate_quality
    from roko_amd.rkdata import RkwFile
    from tests.test_gpu_votes import CONTIG_LEN, _draw_positions, _host_table

    rng = np.random.default_rng(9)
    pipe = InferencePipeline(cases["model"], 32, depth=1, quality=True)
    dv = DeviceVotes({"c": CONTIG_LEN}, pipe, quality=True)
    positions = _draw_positions(rng, 49, free_tail=0)
    _, _, examples, _ = RkwFile(cases[3000]["rkw"]).group_arrays(0)
    x = np.array(examples[:49])
    preds = np.empty((49, C.WINDOW_COLS), dtype=np.uint8)
    units = np.empty((49, C.WINDOW_COLS, C.NUM_CLASSES), dtype=np.uint8)
    for lo, hi in ((0, 32), (32, 49)):
        xs, ps = dv.staging()
        xs[: hi - lo], ps[: hi - lo] = x[lo:hi], positions[lo:hi]
        dv.add_batch("c", hi - lo)
        dv.drain()
        preds[lo:hi] = pipe.slots[0].cpp.amax[: hi - lo].cpu().numpy()
        units[lo:hi] = pipe.slots[0].cpp.qv[: hi - lo].cpu().numpy()
    assert len(np.unique(preds)) > 1 and len(np.unique(units)) > 3
    keys, counts = _host_table(positions, preds)
    qkeys, sums = accumulate_quality(positions[None].reshape(1, -1, 2),
                                     units.reshape(1, -1, C.NUM_CLASSES))
    got_keys, got_counts = dv.counts("c")
    np.testing.assert_array_equal(got_keys, keys)
    np.testing.assert_array_equal(got_counts, counts)
    got_qkeys, got_sums = dv.sums("c")
    np.testing.assert_array_equal(got_qkeys, qkeys)
    np.testing.assert_array_equal(got_sums, sums)


@requires_gpu
def test_quality_needs_a_quality_pipeline(cases):
    from roko_amd.ops.forward import InferencePipeline
    from roko_amd.ops.votes import DeviceVotes

    pipe = InferencePipeline(cases["model"], 32, depth=1)
    assert pipe.slots[0].cpp.quality is False
    with pytest.raises(ValueError, match="quality=True"):
        DeviceVotes({"c": 200}, pipe, quality=True)


def _read(path):
    with open(path, "rb") as fh:
        return fh.read()


# (ref_len, slot batch, polish depth), see test_gpu_votes.py: one 32-slot
# used three times; four 32-slots adding into one table at once; the
# captured-graph body of the 256-slot with a full and then a padded replay
@requires_gpu
@pytest.mark.parametrize("ref_len,batch,depth",
                         [(3000, 32, 1), (9000, 32, 4), (9000, 256, 1)])
def test_fastq_over_the_device_routes(cases, ref_len, batch, depth):
    from roko_amd.config import FeatureConfig
    from roko_amd.inference import infer
    from roko_amd.io.fasta import read_fasta, read_fastq
    from roko_amd.polish import polish

    case, model = cases[ref_len], cases["model"]
    d = case["dir"]
    path = lambda name: str(d / f"{name}_{batch}_{depth}")  # noqa: E731
    common = dict(workers=1, batch_size=batch, model=model, log=QUIET,
                  depth=depth)
    plain = polish(case["ref"], case["bam"], None, path("plain.fasta"),
                   cfg=FeatureConfig(seed=1), **common)
    got = polish(case["ref"], case["bam"], None, path("pol.fasta"),
                 cfg=FeatureConfig(seed=1), out_fastq=path("pol.fastq"),
                 **common)
    assert got == plain and plain["ctg1"] != case["draft"]
    assert _read(path("pol.fasta")) == _read(path("plain.fasta"))
    recs = list(read_fastq(path("pol.fastq")))
    assert [(n, s) for n, s, _ in recs] == \
        list(read_fasta(path("plain.fasta")))
    quals = "".join(q for _, _, q in recs)
    assert all("!" <= ch <= chr(93) for ch in quals)
    assert len(set(quals)) > 1

    got_inf = infer(case["rkw"], None, None, batch_size=batch, model=model,
                    log=QUIET, votes="device", depth=depth,
                    out_fastq=path("inf.fastq"))
    assert got_inf == plain
    assert _read(path("inf.fastq")) == _read(path("pol.fastq"))

    counter = FeatureConfig(seed=1, sampler="counter")
    polish(case["ref"], case["bam"], None, None, cfg=counter,
           out_fastq=path("hostc.fastq"), **common)
    polish(case["ref"], case["bam"], None, None, cfg=counter,
           out_fastq=path("dev.fastq"), extract="device", **common)
    assert _read(path("dev.fastq")) == _read(path("hostc.fastq"))


@requires_gpu
def test_infer_fastq_with_host_votes_on_a_gpu_raises(cases):
    from roko_amd.inference import infer

    with pytest.raises(ValueError, match="votes='device'"):
        infer(cases[3000]["rkw"], None, None, model=cases["model"],
              log=QUIET, votes="host",
              out_fastq=str(cases[3000]["dir"] / "never.fastq"))
