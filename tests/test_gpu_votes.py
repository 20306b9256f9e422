"""Device votes on the GPU: the scatter and consensus kernels against the
host vote table (exact integer equality), overflow reporting, and the votes
mode of the serving slots end to end (polish == infer(device) == infer(host),
byte for byte)."""

import numpy as np
import pytest
import torch

from roko_amd import config as C

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs ROCm GPU"
)

QUIET = lambda *a, **k: None  # noqa: E731
CONTIG_LEN = 200  # 800 slots


def _draw_positions(rng, n, free_tail, cap=6):
    """(n, 90, 2) positions drawn without replacement from `cap` copies of
    every slot of the contig (but its last `free_tail` bases): slots are hit
    several times within a batch and at most `cap` times in total — the
    extractor's bound, which the 4-bit counters must hold."""
    slots = np.arange((CONTIG_LEN - free_tail) * (C.MAX_INS + 1))
    pool = rng.permutation(np.repeat(slots, cap))[: n * C.WINDOW_COLS]
    assert len(pool) == n * C.WINDOW_COLS
    pos = np.stack([pool // (C.MAX_INS + 1), pool % (C.MAX_INS + 1)], axis=1)
    return pos.reshape(n, C.WINDOW_COLS, 2).astype(np.int32)


def _host_table(positions, preds):
    from roko_amd.inference import accumulate_votes

    live = positions[..., 0] >= 0
    return accumulate_votes(positions[live][None], preds[live][None])


@pytest.fixture(scope="module")
def scattered():
    """One table filled through the direct vote_scatter binding with given
    random classes: two calls (32 windows, then 17), rows marked pos = -1
    in both, every slot hit at most 6 times and many exactly 6."""
    from roko_amd.ops.votes import DeviceVotes

    rng = np.random.default_rng(42)
    positions = _draw_positions(rng, 49, free_tail=15)  # 60 slots stay empty
    positions[[5, 30, 31, 47, 48]] = -1  # rows that must not vote
    preds = rng.integers(0, C.NUM_CLASSES, (49, C.WINDOW_COLS)).astype(np.uint8)
    # a crafted tie, on a column nothing else touches: classes 1 and 3 twice
    tie_pos = CONTIG_LEN - 3
    positions[0, :4] = [[tie_pos, 0]] * 4
    preds[0, :4] = [3, 1, 3, 1]
    dv = DeviceVotes({"c": CONTIG_LEN})
    dv.scatter("c", preds[:32], positions[:32])
    dv.scatter("c", preds[32:], positions[32:])
    keys, counts = _host_table(positions, preds)
    return dv, keys, counts, tie_pos


@requires_gpu
def test_scatter_matches_host_table_exactly(scattered):
    dv, keys, counts, _ = scattered
    assert counts.sum(axis=1).max() == 6  # the multiplicity bound is reached
    assert (counts.sum(axis=1) > 1).sum() > 100  # shared columns
    assert np.count_nonzero(counts.sum(axis=0)) == C.NUM_CLASSES
    got_keys, got_counts = dv.counts("c")
    assert got_keys.dtype == np.int64 and got_counts.dtype == np.int64
    np.testing.assert_array_equal(got_keys, keys)
    np.testing.assert_array_equal(got_counts, counts)


@requires_gpu
def test_consensus_matches_dense_reference(scattered):
    from roko_amd.inference import NO_VOTE, SLOTS_PER_POS, dense_majority

    dv, keys, counts, tie_pos = scattered
    want = dense_majority(keys, counts, CONTIG_LEN)
    got = dv.consensus("c")
    assert got.dtype == np.uint8 and got.shape == (CONTIG_LEN * SLOTS_PER_POS,)
    np.testing.assert_array_equal(got, want)
    assert got[tie_pos * SLOTS_PER_POS] == 1  # 1 and 3 tie -> smallest id
    assert (got == NO_VOTE).sum() >= 56       # untouched slots
    assert (got != NO_VOTE).sum() == len(keys)


@requires_gpu
def test_consensus_handles_a_partial_last_group():
    """n_slots that is no multiple of the 4-slot vector group: the tail goes
    slot by slot and nothing past n_slots is written."""
    from roko_amd.ops import ext

    rng = np.random.default_rng(3)
    n_slots = 4 * 300 + 3  # more than one 256-thread block, ragged tail
    packed = np.zeros(n_slots + 8, dtype=np.uint32)
    cnt = rng.integers(0, 7, (n_slots, C.NUM_CLASSES)).astype(np.uint32)
    cnt[rng.random(n_slots) < 0.3] = 0
    for c in range(C.NUM_CLASSES):
        packed[:n_slots] |= cnt[:, c] << np.uint32(4 * c)
    packed[n_slots:] = 0x11111  # beyond the table in use: must be ignored
    table = torch.from_numpy(packed.view(np.int32)).cuda()
    maj = torch.full((n_slots + 8,), 0x77, dtype=torch.uint8, device="cuda")
    ext().vote_consensus(table, n_slots, maj)
    got = maj.cpu().numpy()
    want = np.where(cnt.sum(axis=1) == 0, 0xFF, cnt.argmax(axis=1)).astype(np.uint8)
    np.testing.assert_array_equal(got[:n_slots], want)
    assert (got[n_slots:] == 0x77).all()


@requires_gpu
def test_overflow_is_reported_not_silent():
    from roko_amd.ops.votes import DeviceVotes, VoteOverflowError

    positions = np.full((1, C.WINDOW_COLS, 2), -1, dtype=np.int32)
    preds = np.zeros((1, C.WINDOW_COLS), dtype=np.uint8)
    positions[0, :16] = [[5, 2]] * 16  # 16 votes, one class, one slot
    preds[0, :16] = 3
    dv = DeviceVotes({"c": CONTIG_LEN})
    dv.scatter("c", preds, positions)
    with pytest.raises(VoteOverflowError, match="host votes"):
        dv.counts("c")
    with pytest.raises(VoteOverflowError, match="host votes"):
        dv.consensus("c")
    # 15 votes are still exact
    positions[0, 15] = -1
    dv = DeviceVotes({"c": CONTIG_LEN})
    dv.scatter("c", preds, positions)
    keys, counts = dv.counts("c")
    assert keys.tolist() == [5 << 3 | 2] and counts.tolist() == [[0, 0, 0, 15, 0]]


@requires_gpu
def test_host_validation_rejects_out_of_range_positions():
    """Bad positions never reach the kernel: add_batch/scatter raise on the
    host before anything is uploaded."""
    from roko_amd.ops.votes import DeviceVotes

    dv = DeviceVotes({"c": CONTIG_LEN})
    preds = np.zeros((1, C.WINDOW_COLS), dtype=np.uint8)
    pos = np.zeros((1, C.WINDOW_COLS, 2), dtype=np.int32)
    pos[0, 7] = [CONTIG_LEN, 0]
    with pytest.raises(ValueError, match="position outside"):
        dv.scatter("c", preds, pos)
    pos[0, 7] = [3, C.MAX_INS + 1]
    with pytest.raises(ValueError, match="insertion slot outside"):
        dv.scatter("c", preds, pos)
    assert not dv.has_votes("c")


# -- votes mode end to end ----------------------------------------------------

@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """Two synthetic assemblies (3 kb and 9 kb) with their RKW files, and a
    model trained briefly on the small one so votes are not one class."""
    from roko_amd.config import FeatureConfig, TrainConfig
    from roko_amd.features import run as features_run
    from roko_amd.train import train
    from tests.test_gpu_e2e import _make_case

    out = {}
    for ref_len in (3000, 9000):
        d = tmp_path_factory.mktemp(f"case{ref_len}")
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
def test_slot_padding_rows_do_not_vote(cases):
    """Slot batch 32, depth 1: a full batch of 32, then 17 windows into the
    same slot. Rows 17..32 of the slot still hold the first batch, so the
    model predicts for them; they must not vote. The slot's own predictions
    (read back for the test only) give the expected table; real windows and
    the trained model make them a mixture of classes."""
    from roko_amd.ops.forward import InferencePipeline
    from roko_amd.ops.votes import DeviceVotes
    from roko_amd.rkdata import RkwFile

    rng = np.random.default_rng(9)
    pipe = InferencePipeline(cases["model"], 32, depth=1)
    dv = DeviceVotes({"c": CONTIG_LEN}, pipe)
    positions = _draw_positions(rng, 49, free_tail=0)
    _, _, examples, _ = RkwFile(cases[3000]["rkw"]).group_arrays(0)
    x = np.array(examples[:49])
    assert x.shape == (49, C.WINDOW_ROWS, C.WINDOW_COLS)
    preds = np.empty((49, C.WINDOW_COLS), dtype=np.uint8)
    for lo, hi in ((0, 32), (32, 49)):
        xs, ps = dv.staging()
        xs[: hi - lo], ps[: hi - lo] = x[lo:hi], positions[lo:hi]
        dv.add_batch("c", hi - lo)
        dv.drain()
        preds[lo:hi] = pipe.slots[0].cpp.amax[: hi - lo].cpu().numpy()
    assert len(np.unique(preds)) > 1
    keys, counts = _host_table(positions, preds)
    assert counts.sum(axis=1).max() == 6
    got_keys, got_counts = dv.counts("c")
    np.testing.assert_array_equal(got_keys, keys)
    np.testing.assert_array_equal(got_counts, counts)


def _read(path):
    with open(path, "rb") as fh:
        return fh.read()


# (ref_len, slot batch, polish depth). 3 kb gives ~100 windows: three runs
# of one 32-slot, or one padded batch of 256 (the captured-graph slot path
# is taken from batch 256 up). 9 kb gives ~300 windows: four 32-slots adding
# into one table at once, each used at least twice, and at depth 1 two runs
# of the 256-slot — a full batch, then a padded one through the replayed
# graph.
@requires_gpu
@pytest.mark.parametrize("ref_len,batch,depth",
                         [(3000, 32, 1), (9000, 32, 4), (3000, 256, 1),
                          (9000, 256, 1)])
def test_polish_equals_infer_device_equals_infer_host(cases, ref_len, batch,
                                                      depth):
    from roko_amd.config import FeatureConfig
    from roko_amd.inference import infer
    from roko_amd.polish import polish

    case, model = cases[ref_len], cases["model"]
    d = case["dir"]
    if batch == 32:
        assert -(-case["n"] // batch) >= 2 * depth  # every slot reused
    elif ref_len == 9000:
        assert batch < case["n"] < 2 * batch  # full batch, then a padded one
    host, dev, pol = (str(d / f"{way}{batch}.fasta")
                      for way in ("host", "dev", "polish"))
    want = infer(case["rkw"], None, host, batch_size=batch, model=model,
                 log=QUIET, votes="host", depth=4)
    got_dev = infer(case["rkw"], None, dev, batch_size=batch, model=model,
                    log=QUIET, votes="device", depth=max(depth, 1))
    got_pol = polish(case["ref"], case["bam"], None, pol, workers=1,
                     batch_size=batch, cfg=FeatureConfig(seed=1), model=model,
                     log=QUIET, depth=depth)
    assert want["ctg1"] != case["draft"]  # the model does change the draft
    assert got_dev == want
    assert got_pol == want
    assert _read(dev) == _read(host)
    assert _read(pol) == _read(host)
