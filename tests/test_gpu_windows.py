"""Device window builder (ops/hip/windows.hip) against its exact oracle: the
C++ builder with the counter sampler, byte for byte, windows and positions.
The BAMs are the small cases of tests/window_cases.py."""

import numpy as np
import pytest
import torch

from tests import window_cases as WC

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs ROCm GPU"
)

QUIET = lambda *a, **k: None  # noqa: E731


def _both(case, seed=11):
    """(oracle positions, oracle windows, device positions, device windows)
    of one (bam, contig, start, end) case, as numpy arrays."""
    from roko_amd.config import FeatureConfig
    from roko_amd.ops import _pileup
    from roko_amd.ops.windows import build_windows

    bam, contig, start, end = case
    cfg = FeatureConfig(seed=seed)
    want_pos, want_x = _pileup.generate_features(
        bam, contig, start, end, seed=seed, sampler="counter")
    pack = _pileup.region_reads(bam, contig, start, end, cfg.filter_flag,
                                cfg.min_mapq, seed)
    x, pos = build_windows(pack, cfg, "cuda")
    assert x.is_cuda and pos.is_cuda
    assert x.dtype == torch.uint8 and pos.dtype == torch.int32
    return want_pos, want_x, pos.cpu().numpy(), x.cpu().numpy()


def _assert_same(case, seed=11):
    want_pos, want_x, pos, x = _both(case, seed)
    assert pos.shape == want_pos.shape and x.shape == want_x.shape
    np.testing.assert_array_equal(pos, want_pos)
    np.testing.assert_array_equal(x, want_x)
    return want_pos, want_x


@requires_gpu
def test_crafted_region(tmp_path):
    pos, x = _assert_same(WC.crafted(tmp_path))
    assert len(pos) == 13
    ins = pos[..., 1]
    assert ins.max() == 3  # insertions of 4 and 5 are capped
    assert list(pos[0, 0]) == [100, 0]  # nothing behind position 99
    assert list(pos[-1, -1]) == [499, 2]  # the insertion behind end - 1
    assert x.max() >= 6 and (x == 5).any() and (x == 4).any()


@requires_gpu
def test_empty_windows_are_skipped(tmp_path):
    pos, _ = _assert_same(WC.empty_windows(tmp_path))
    first = pos[:, 0, 0]
    n_all = (1000 - 90) // 30 + 1
    assert len(pos) < n_all  # some windows had no valid read
    assert not ((first >= 300) & (first <= 510)).any()
    assert (first < 300).any() and (first > 510).any()


@requires_gpu
def test_degenerate_regions(tmp_path):
    bam, contig, _, _ = WC.crafted(tmp_path)
    for case in ((bam, contig, 100, 150),   # fewer than 90 columns
                 (bam, "empty", 0, 400),    # no reads
                 (bam, contig, 700, 800)):  # clamped to nothing
        want_pos, want_x, pos, x = _both(case)
        assert want_x.shape == (0, 200, 90) and want_pos.shape == (0, 90, 2)
        assert x.shape == (0, 200, 90) and pos.shape == (0, 90, 2)


@requires_gpu
def test_wide_window(tmp_path):
    pos, x = _assert_same(WC.wide(tmp_path))
    assert len(pos) == 1


@requires_gpu
def test_long_cigar(tmp_path):
    pos, _ = _assert_same(WC.long_cigar(tmp_path))
    assert len(pos) > 20 and pos[..., 1].max() == 3


@requires_gpu
@pytest.mark.parametrize("seed", [21, 22, 23])
def test_random_regions(tmp_path, seed):
    pos, _ = _assert_same(WC.random_region(tmp_path, seed), seed=seed)
    assert len(pos) > 50


@requires_gpu
def test_geometry_and_device_are_checked(tmp_path):
    from roko_amd.config import FeatureConfig
    from roko_amd.ops import _pileup
    from roko_amd.ops.windows import build_windows

    bam, contig, start, end = WC.crafted(tmp_path)
    pack = _pileup.region_reads(bam, contig, start, end, 0xF04, 10, 0)
    with pytest.raises(ValueError, match="compiled for"):
        build_windows(pack, FeatureConfig(window_stride=45), "cuda")
    with pytest.raises(ValueError, match="GPU"):
        build_windows(pack, FeatureConfig(), "cpu")
    broken = dict(pack, cigar=pack["cigar"][:-1])
    with pytest.raises(ValueError, match="cigar_off"):
        build_windows(broken, FeatureConfig(), "cuda")


@requires_gpu
@pytest.mark.parametrize("workers", [1, 2])
def test_polish_device_extract_end_to_end(tmp_path, workers):
    """polish(extract="device") writes the FASTA of the host route with the
    counter sampler; the device vote table raises no range/overflow flag
    (consensus() checks it on the way)."""
    from roko_amd.config import FeatureConfig
    from roko_amd.model import RokoModel
    from roko_amd.polish import LAST_RUN, polish
    from tests.test_gpu_e2e import _make_case

    case = _make_case(tmp_path, ref_len=6000, cov=20)
    torch.manual_seed(0)
    model = RokoModel()
    kw = dict(workers=workers, batch_size=32, model=model, depth=4, log=QUIET)
    cfg = FeatureConfig(seed=3, sampler="counter", region_size=2500)
    host = polish(case["ref"], case["bam"], None, None, cfg=cfg,
                  extract="host", **kw)
    n_host = LAST_RUN["windows"]
    # the device route ignores cfg.sampler
    dev = polish(case["ref"], case["bam"], None, None,
                 cfg=FeatureConfig(seed=3, region_size=2500),
                 extract="device", **kw)
    assert LAST_RUN["windows"] == n_host > 100
    assert LAST_RUN["failed_regions"] == 0
    assert dev == host
    assert set(dev) == {"ctg1"}
