"""Truth labels on the GPU (ops/hip/windows.hip: truth_scan, label_windows)
against the numpy reference, and features.run(extract="device") against the
host route with the counter sampler, group for group. Cases and the dict-path
oracle: tests/label_cases.py."""

import numpy as np
import pytest
import torch

from tests import label_cases as LC
from tests.window_cases import read

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs ROCm GPU"
)


def _truth(case):
    from roko_amd.labels import get_aligns
    from roko_amd.ops.labels_device import TruthPack, scan_truth

    aligns = get_aligns(case["truth_bam"], case["contig"], 0,
                        case["draft_len"])
    truth = TruthPack(aligns, "cuda")
    return aligns, truth, scan_truth(truth.host)


def _device_labels(truth, pos, index, lo, hi):
    labels, keep, err = truth.label_windows(
        torch.from_numpy(np.ascontiguousarray(pos)).cuda(), index, lo, hi)
    assert labels.dtype == torch.uint8 and keep.dtype == torch.uint8
    return labels.cpu().numpy(), keep.cpu().numpy(), int(err)


@requires_gpu
@pytest.mark.parametrize("builder", LC.CASES_B + LC.CASES_C + (LC.two_records_n,),
                         ids=lambda f: f.__name__)
def test_label_kernel_equals_reference(tmp_path, builder):
    from roko_amd.ops.labels_device import (label_span,
                                            label_windows_reference,
                                            region_aligns)

    case = builder(tmp_path)
    aligns, truth, scan = _truth(case)
    # the device scan is the host scan, op for op (carry across 64-op chunks)
    np.testing.assert_array_equal(truth.err, [s.err for s in scan])
    np.testing.assert_array_equal(truth._dev[-2].cpu().numpy(),
                                  np.concatenate([s.rpos for s in scan]))
    np.testing.assert_array_equal(truth._dev[-1].cpu().numpy(),
                                  np.concatenate([s.qpos for s in scan]))
    total = 0
    for start, end in case["regions"]:
        for index, a in region_aligns(aligns, truth.host["ref_end"], start,
                                      end):
            lo, hi = max(start, a.start), min(end, a.end)
            span = label_span(truth.host, index, lo, hi, scan)
            if span is None or span[1] <= span[0]:
                continue
            pos = LC.window_positions(case, *span)
            # all windows, one window, no window
            for sub in (pos, pos[:1], pos[-1:], pos[:0]):
                want = label_windows_reference(sub, truth.host, index, lo, hi,
                                               scan)
                got = _device_labels(truth, sub, index, lo, hi)
                assert got[0].shape == (len(sub), 90)
                assert got[1].shape == (len(sub),)
                np.testing.assert_array_equal(got[0], want[0])
                np.testing.assert_array_equal(got[1], want[1])
                assert got[2] == want[2] == 0
            total += len(pos)
    assert total > 20


@requires_gpu
def test_scan_refusal_bits_on_device():
    from roko_amd.labels import TruthAlign
    from roko_amd.ops.labels_device import TruthPack, scan_truth

    def align(*ops):
        cig = np.array([(l << 4) | "MIDNSHP=X".index(op) for l, op in ops],
                       dtype=np.uint32)
        q = sum(l for l, op in ops if op in "MIS=X")
        return TruthAlign("t", 0, 5, 60, cig, "A" * q)

    many = [(2, "M"), (1, "I")] * 70  # clip behind two full scan chunks
    truth = TruthPack([
        align((3, "H"), (4, "S"), (50, "M"), (2, "I"), (6, "S"), (1, "H")),
        align((50, "M"), (0, "I"), (50, "M")),
        align((50, "M"), (3, "S"), (50, "M")),
        align((2, "S"), (50, "M"), (1, "P"), (2, "I"), (50, "M")),
        align(*many, (3, "S"), (5, "M")),
        align(*many, (5, "M"), (3, "S")),
    ], "cuda")
    want = [s.err for s in scan_truth(truth.host)]
    assert want == [0, 1, 2, 2, 2, 0]
    np.testing.assert_array_equal(truth.err, want)
    with pytest.raises(ValueError, match="refused"):
        truth.label_windows(torch.zeros((1, 90, 2), dtype=torch.int32,
                                        device="cuda"), 1, 5, 50)


@requires_gpu
def test_column_outside_the_span_sets_the_error_bit(tmp_path):
    from roko_amd.ops.labels_device import (LABEL_ERR_RANGE,
                                            label_windows_reference)

    case = LC.one_op(tmp_path)
    _, truth, scan = _truth(case)
    pos = LC.window_positions(case, 0, 1200)
    want = label_windows_reference(pos, truth.host, 0, 100, 1100, scan)
    got = _device_labels(truth, pos, 0, 100, 1100)
    assert got[2] == want[2] == LABEL_ERR_RANGE
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])


# ---------------------------------------------------------------------------
# end to end

def _groups(path):
    from roko_amd.rkdata import RkwFile

    f = RkwFile(path)
    out = []
    for gi in range(len(f.groups)):
        g, pos, ex, lab = f.group_arrays(gi)
        out.append(((g["contig"], g["start"], g["end"], g["size"]),
                    np.array(pos), np.array(ex),
                    None if lab is None else np.array(lab)))
    return out


def _assert_same_file(dev_path, host_path):
    dev, host = _groups(dev_path), _groups(host_path)
    assert [g[0] for g in dev] == [g[0] for g in host]
    for d, h in zip(dev, host):
        assert d[1].dtype == h[1].dtype
        np.testing.assert_array_equal(d[1], h[1])
        np.testing.assert_array_equal(d[2], h[2])
        assert (d[3] is None) == (h[3] is None)
        if d[3] is not None:
            np.testing.assert_array_equal(d[3], h[3])
    return sum(g[0][3] for g in host)


def _run_both(tmp_path, ref, reads, truth, cfg_kw, workers=1, tag=""):
    """(device file, host file, device log lines)."""
    from roko_amd import features
    from roko_amd.config import FeatureConfig

    lines = []
    dev, host = str(tmp_path / f"dev{tag}.rkw"), str(tmp_path / f"host{tag}.rkw")
    n_host = features.run(ref, reads, host, bam_y=truth, workers=1,
                          cfg=FeatureConfig(sampler="counter", **cfg_kw),
                          log=lambda *a: None)
    # the device route ignores cfg.sampler
    n_dev = features.run(ref, reads, dev, bam_y=truth, workers=workers,
                         cfg=FeatureConfig(**cfg_kw), extract="device",
                         log=lambda *a: lines.append(" ".join(map(str, a))))
    assert n_dev == n_host
    return dev, host, lines


@pytest.fixture(scope="module")
def assembly(tmp_path_factory):
    from tests.simple_align import build_assembly

    return build_assembly(np.random.default_rng(5),
                          tmp_path_factory.mktemp("asm"), length=6000, cov=20)


@requires_gpu
@pytest.mark.parametrize("workers", [1, 2])
def test_features_device_training_end_to_end(tmp_path, assembly, workers):
    dev, host, _ = _run_both(tmp_path, assembly["draft_fasta"],
                             assembly["reads_bam"], assembly["truth_bam"],
                             dict(seed=3, region_size=2500), workers)
    assert _assert_same_file(dev, host) > 100


@requires_gpu
def test_features_device_inference_end_to_end(tmp_path, assembly):
    dev, host, _ = _run_both(tmp_path, assembly["draft_fasta"],
                             assembly["reads_bam"], None,
                             dict(seed=3, region_size=2500))
    assert _assert_same_file(dev, host) > 100


def _draft(tmp_path, case):
    from roko_amd.io.fasta import write_fasta

    rng = np.random.default_rng(1)
    path = str(tmp_path / "draft.fasta")
    write_fasta(path, [(case["contig"], "".join(
        "ACGT"[int(b)] for b in rng.integers(0, 4, case["draft_len"])))])
    return path


@requires_gpu
def test_two_truth_records_with_unknown_bases(tmp_path):
    case = LC.two_records_n(tmp_path)
    dev, host, _ = _run_both(tmp_path, _draft(tmp_path, case),
                             case["reads_bam"], case["truth_bam"],
                             dict(seed=3, region_size=900, region_overlap=100))
    n = _assert_same_file(dev, host)
    # windows were dropped for the N bases, and both records label windows
    n_inf = _assert_same_file(*_run_both(
        tmp_path, _draft(tmp_path, case), case["reads_bam"], None,
        dict(seed=3, region_size=900, region_overlap=100), tag="i")[:2])
    assert 20 < n < n_inf


@requires_gpu
def test_refused_region_is_built_on_the_host(tmp_path):
    """A read with a zero-length CIGAR op: the device builder refuses its
    region (the existing error flag), that region alone comes from the host
    functions, and the file is still the oracle's."""
    rng = np.random.default_rng(9)
    case = LC._write(tmp_path, "zero", 2200, [(0, LC.SHAPES_CIGAR, None)],
                     [(0, 2200)],
                     extra_reads=[read(rng, "zero", 100, "50M0M2I50M")])
    for truth in (case["truth_bam"], None):
        dev, host, lines = _run_both(
            tmp_path, _draft(tmp_path, case), case["reads_bam"], truth,
            dict(seed=3, region_size=900, region_overlap=100),
            tag="t" if truth else "i")
        assert _assert_same_file(dev, host) > 30
        fell_back = [l for l in lines if "built on the host" in l]
        assert len(fell_back) == 1 and "zero-length" in fell_back[0]
        assert len(_groups(dev)) == 3  # the other two regions: device


@requires_gpu
def test_refused_truth_is_labelled_on_the_host(tmp_path):
    """A truth record with a soft clip between aligned ops: truth_scan
    flags it, its regions are built by the host functions."""
    cig = [(600, "M"), (3, "S"), (2, "I"), (700, "M")]
    case = LC._write(tmp_path, "clip", 1300, [(0, cig, None)], [(0, 1300)])
    dev, host, lines = _run_both(tmp_path, _draft(tmp_path, case),
                                 case["reads_bam"], case["truth_bam"],
                                 dict(seed=3))
    assert _assert_same_file(dev, host) > 20
    assert sum("built on the host" in l for l in lines) == 1
