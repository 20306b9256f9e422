"""The counter row sampler of the window builder and the packed-read export
(`_pileup.region_reads`) that feeds the GPU builder — CPU side."""

import numpy as np
import pytest

from roko_amd.io.bamio import write_bam
from roko_amd.ops import _pileup
from tests import window_cases as WC

M64 = (1 << 64) - 1
ROWS, COLS, STRIDE = 200, 90, 30
FILTER = 0xF04


def mix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def region_key(seed, tid, start):
    return mix64(seed ^ mix64(((tid << 32) ^ start) & M64))


def draw(key, w, r):
    return mix64(key ^ mix64(((w << 32) | r) & M64))


@pytest.fixture
def spanning(tmp_path):
    """12 reads over the whole contig, no N, each with its own random bases:
    every read is valid in every window, in read order."""
    rng = np.random.default_rng(5)
    reads = [WC.read(rng, f"r{i}", 0, "500M", flag=16 if i % 3 == 0 else 0,
                     tid=1) for i in range(12)]
    path = str(tmp_path / "spanning.bam")
    write_bam(path, [("other", 100), ("ctg", 500)], reads)
    return path, reads


def test_counter_sampler_rows(spanning):
    path, reads = spanning
    seed, start, end = 77, 30, 470
    pos, x = _pileup.generate_features(path, "ctg", start, end, seed=seed,
                                       sampler="counter")
    pos_mt, x_mt = _pileup.generate_features(path, "ctg", start, end,
                                             seed=seed)
    n = (end - start - COLS) // STRIDE + 1
    assert x.shape == (n, ROWS, COLS) and pos.shape == (n, COLS, 2)
    np.testing.assert_array_equal(pos, pos_mt)
    assert not np.array_equal(x, x_mt)  # another stream, same windows

    enc = np.array([["ACGT".index(c) + (6 if r.flag & 16 else 0)
                     for c in r.seq] for r in reads], dtype=np.uint8)
    key = region_key(seed, 1, start)
    assert _pileup.region_reads(path, "ctg", start, end, FILTER, 10,
                                seed)["region_key"] == key
    for w in range(n):
        c0 = start + w * STRIDE
        rows = enc[:, c0:c0 + COLS]
        assert len({r.tobytes() for r in rows}) == len(reads)
        picks = [draw(key, w, r) % len(reads) for r in range(ROWS)]
        np.testing.assert_array_equal(x[w], rows[picks])


def test_default_sampler_unchanged_by_keyword(spanning):
    path, _ = spanning
    a = _pileup.generate_features(path, "ctg", 0, 500, seed=3)
    b = _pileup.generate_features(path, "ctg", 0, 500, seed=3,
                                  sampler="mt19937")
    np.testing.assert_array_equal(a[1], b[1])


def test_unknown_sampler_raises(spanning):
    path, _ = spanning
    with pytest.raises(ValueError, match="sampler"):
        _pileup.generate_features(path, "ctg", 0, 500, sampler="xorshift")


def _kept(rec, min_mapq=10):
    _, flag, _, mapq, cig, seq = rec
    if flag & FILTER or (flag & 1 and not flag & 2) or mapq < min_mapq:
        return False
    return len(seq) > 0 and len(cig) > 0


def test_region_reads_matches_fetch_records(tmp_path):
    bam, contig, start, end = WC.crafted(tmp_path)
    pack = _pileup.region_reads(bam, contig, start, end, FILTER, 10, 9)
    recs = [r for r in _pileup.fetch_records(bam, contig, start, end)
            if _kept(r)]
    all_recs = _pileup.fetch_records(bam, contig, start, end)
    assert 0 < len(recs) < len(all_recs)  # the filters dropped some
    n = len(recs)
    assert (pack["start"], pack["end"], pack["tid"]) == (start, end, 0)
    assert pack["region_key"] == region_key(9, 0, start)
    for name, dt, size in (("ref_start", np.int32, n), ("ref_end", np.int32, n),
                           ("reverse", np.uint8, n),
                           ("cigar_off", np.uint32, n + 1),
                           ("seq_off", np.uint32, n + 1)):
        assert pack[name].dtype == dt and pack[name].shape == (size,), name
    assert pack["cigar"].dtype == np.uint32 and pack["seq4"].dtype == np.uint8
    co, so = pack["cigar_off"], pack["seq_off"]
    assert co[0] == 0 and so[0] == 0
    assert co[-1] == len(pack["cigar"]) and so[-1] == len(pack["seq4"])
    code = "=ACMGRSVTWYHKDBN"
    for i, (_, flag, pos, _, cig, seq) in enumerate(recs):
        np.testing.assert_array_equal(pack["cigar"][co[i]:co[i + 1]], cig)
        assert so[i + 1] - so[i] == (len(seq) + 1) // 2
        packed = pack["seq4"][so[i]:so[i + 1]]
        got = "".join(code[(packed[q >> 1] >> (0 if q & 1 else 4)) & 15]
                      for q in range(len(seq)))
        assert got == seq
        assert pack["reverse"][i] == (1 if flag & 16 else 0)
        assert pack["ref_start"][i] == pos
        span = sum(int(c) >> 4 for c in cig if (int(c) & 15) in (0, 2, 3, 7, 8))
        assert pack["ref_end"][i] == pos + span


def test_region_reads_clamps_and_empty(tmp_path):
    bam, contig, _, _ = WC.crafted(tmp_path)
    pack = _pileup.region_reads(bam, contig, -50, 10_000, FILTER, 10, 0)
    assert (pack["start"], pack["end"]) == (0, 600)
    assert len(pack["ref_start"]) > 0
    empty = _pileup.region_reads(bam, "empty", 0, 400, FILTER, 10, 0)
    assert len(empty["ref_start"]) == 0 and len(empty["cigar"]) == 0
    assert list(empty["cigar_off"]) == [0] and list(empty["seq_off"]) == [0]
    assert empty["tid"] == 1
    with pytest.raises(RuntimeError, match="contig"):
        _pileup.region_reads(bam, "nope", 0, 10, FILTER, 10, 0)


def test_generate_reads_worker_and_config(tmp_path):
    from roko_amd import features as F

    bam, contig, start, end = WC.crafted(tmp_path)
    cfg = F.FeatureConfig(seed=4, sampler="counter")
    c, s, e, pack = F.generate_reads((bam, contig, start, end, cfg))
    assert (c, s, e) == (contig, start, end)
    assert pack["region_key"] == region_key(4, 0, start)
    bad = F.generate_reads((bam, "nope", 0, 10, cfg))
    assert bad[0] == "__error__" and "nope" in bad[1]
    # FeatureConfig.sampler reaches the builder
    _, x = F._features_for_region(bam, contig, start, end, cfg)
    _, want = _pileup.generate_features(bam, contig, start, end, seed=4,
                                        sampler="counter")
    np.testing.assert_array_equal(x, want)
    assert F.FeatureConfig().sampler == "mt19937"


def test_polish_device_extract_needs_gpu(tiny_assembly):
    from roko_amd.model import RokoModel
    from roko_amd.polish import polish

    with pytest.raises(ValueError, match="GPU"):
        polish(tiny_assembly["draft_fasta"], tiny_assembly["reads_bam"], None,
               None, model=RokoModel(), device="cpu", extract="device",
               log=lambda *a, **k: None)
    with pytest.raises(ValueError, match="extract"):
        polish(tiny_assembly["draft_fasta"], tiny_assembly["reads_bam"], None,
               None, model=RokoModel(), device="cpu", extract="gpu")


def test_build_windows_refuses_other_geometry():
    from roko_amd.config import FeatureConfig
    from roko_amd.ops.windows import build_windows

    with pytest.raises(ValueError, match="compiled for"):
        build_windows({}, FeatureConfig(window_cols=60), "cuda")
