"""The device label rule on the CPU: ops/labels_device.py's numpy reference,
span and pack against the dict path of labels.get_pos_and_labels +
features._generate_train (tests/label_cases.py holds cases and oracle)."""

import numpy as np
import pytest

from roko_amd import config as C
from tests import label_cases as LC


def _check_case(case):
    """Every region of a case: spans and labels of the reference equal the
    dict path's. Returns (windows, dropped windows, spans that moved)."""
    from roko_amd.labels import get_aligns
    from roko_amd.ops.labels_device import (label_span,
                                            label_windows_reference,
                                            pack_truth, region_aligns,
                                            scan_truth)

    every = get_aligns(case["truth_bam"], case["contig"], 0,
                   case["draft_len"])
    pack = pack_truth(every)
    scan = scan_truth(pack)
    assert all(s.err == 0 for s in scan)
    total = dropped = moved = 0
    for start, end in case["regions"]:
        want = LC.oracle_spans(case, start, end)
        got = region_aligns(every, pack["ref_end"], start, end)
        # the same alignments, in the same order, clipped alike
        assert [(i, a.start, a.end) for i, a in got] == \
            [(i, a.start, a.end) for i, a, _, _, _ in want]
        for index, a, lo, hi, span in want:
            assert label_span(pack, index, lo, hi, scan) == span
            # a small chunk walks the same ends in more steps
            assert label_span(pack, index, lo, hi, scan, chunk=3) == span
            if span is None or span[1] <= span[0]:
                continue
            moved += span[0] != lo
            pos = LC.window_positions(case, *span)
            labels, keep, err = label_windows_reference(pos, pack, index, lo,
                                                        hi, scan)
            want_labels, want_keep = LC.dict_labels(a, start, end, pos)
            assert err == 0
            np.testing.assert_array_equal(labels, want_labels)
            np.testing.assert_array_equal(keep, want_keep)
            total += len(pos)
            dropped += int((keep == 0).sum())
    return total, dropped, moved


@pytest.mark.parametrize("builder", LC.CASES_B, ids=lambda f: f.__name__)
def test_reference_equals_dict_path(tmp_path, builder):
    total, _, _ = _check_case(builder(tmp_path))
    assert total > 20


def test_shapes_case_has_the_columns_it_names(tmp_path):
    """The hand-written case really puts insertion columns where the rule
    has something to say."""
    from roko_amd.labels import get_aligns
    from roko_amd.ops.labels_device import (label_windows_reference,
                                            pack_truth)

    case = LC.shapes(tmp_path)
    pack = pack_truth(get_aligns(case["truth_bam"], case["contig"], 0,
                   case["draft_len"]))
    pos = LC.window_positions(case, 0, 2200)
    labels, _, _ = label_windows_reference(pos, pack, 0, 0, 2200)
    flat = {(int(p), int(s)): int(l) for (p, s), l in
            zip(pos.reshape(-1, 2), labels.reshape(-1))}
    # behind the D, 2I 3I (three slots labelled), 5I (three), behind the N
    for p, n_labelled in ((301, 2), (699, 3), (999, 3), (1003, 1), (1699, 3)):
        slots = [flat[(p, s)] for s in (1, 2, 3)]
        assert sum(l < C.LABEL_GAP for l in slots) == n_labelled, (p, slots)
    assert flat[(300, 0)] == flat[(1001, 0)] == C.LABEL_GAP  # D, N
    # region [500, 1700): the insertion behind 499 is outside, the one
    # behind 1699 is in; the windows end before sub_end = 1699 though
    pos = LC.window_positions(case, 500, 1699)
    assert pos[..., 0].min() == 500 and 1600 < pos[..., 0].max() <= 1698


def test_reference_tiny_assembly(tiny_assembly):
    case = {"reads_bam": tiny_assembly["reads_bam"],
            "truth_bam": tiny_assembly["truth_bam"], "contig": "ctg1",
            "regions": [(0, len(tiny_assembly["draft"])), (700, 2100)],
            "draft_len": len(tiny_assembly["draft"])}
    total, _, _ = _check_case(case)
    assert total > 100


@pytest.mark.parametrize("builder", LC.CASES_C, ids=lambda f: f.__name__)
def test_reference_with_unknown_bases(tmp_path, builder):
    total, dropped, moved = _check_case(builder(tmp_path))
    assert 0 < dropped < total
    assert moved >= 2  # N at the start of both regions' spans


def test_two_records_with_n(tmp_path):
    total, dropped, _ = _check_case(LC.two_records_n(tmp_path))
    assert 0 < dropped < total


def test_pack_round_trip(tmp_path):
    from roko_amd.labels import get_aligns
    from roko_amd.ops.labels_device import pack_truth, unpack_truth

    for builder in (LC.two_records, LC.with_n, LC.long_cigar):
        case = builder(tmp_path)
        aligns = get_aligns(case["truth_bam"], case["contig"], 0,
                   case["draft_len"])
        pack = pack_truth(aligns)
        assert len(pack["ref_start"]) == len(aligns)
        for i, a in enumerate(aligns):
            cigar, seq = unpack_truth(pack, i)
            np.testing.assert_array_equal(cigar, a.cigar)
            assert seq == a.seq.upper()
            assert pack["ref_start"][i] == a.reference_start
            assert pack["ref_end"][i] == a.reference_end


def test_scan_refusal_bits():
    from roko_amd.labels import TruthAlign
    from roko_amd.ops.labels_device import (TRUTH_ERR_CLIP,
                                            TRUTH_ERR_ZERO_OP, pack_truth,
                                            scan_truth)

    def align(*ops):
        cig = np.array([(l << 4) | "MIDNSHP=X".index(op) for l, op in ops],
                       dtype=np.uint32)
        q = sum(l for l, op in ops if op in "MIS=X")
        return TruthAlign("t", 0, 5, 60, cig, "A" * q)

    scans = scan_truth(pack_truth([
        align((3, "H"), (4, "S"), (50, "M"), (2, "I"), (6, "S"), (1, "H")),
        align((50, "M"), (0, "I"), (50, "M")),
        align((50, "M"), (3, "S"), (50, "M")),
        align((2, "S"), (50, "M"), (1, "P"), (2, "I"), (50, "M")),
    ]))
    assert [s.err for s in scans] == [0, TRUTH_ERR_ZERO_OP, TRUTH_ERR_CLIP,
                                      TRUTH_ERR_CLIP]


def test_reference_flags_columns_outside_the_span(tmp_path):
    from roko_amd.labels import get_aligns
    from roko_amd.ops.labels_device import (LABEL_ERR_RANGE,
                                            label_windows_reference,
                                            pack_truth)

    case = LC.one_op(tmp_path)
    pack = pack_truth(get_aligns(case["truth_bam"], case["contig"], 0,
                   case["draft_len"]))
    pos = LC.window_positions(case, 0, 1200)
    _, _, err = label_windows_reference(pos, pack, 0, 100, 1100)
    assert err == LABEL_ERR_RANGE


def test_plan_matches_the_host_route(tmp_path):
    """What the parent computes before fanning out: per region the spans
    _generate_train would build windows over."""
    from roko_amd.config import FeatureConfig
    from roko_amd.features import _plan_device, generate_regions

    case = LC.two_records_n(tmp_path)
    cfg = FeatureConfig(seed=3, region_size=900, region_overlap=100)
    refs = [(case["contig"], "A" * case["draft_len"])]
    regions, truths = _plan_device(refs, case["reads_bam"],
                                   case["truth_bam"], cfg, cfg)
    want = []
    for start, end in generate_regions(case["draft_len"], 900, 100):
        spans = [(i, lo, hi) + span
                 for i, _, lo, hi, span in LC.oracle_spans(case, start, end)
                 if span is not None and span[1] > span[0]]
        if spans:
            want.append((start, end, spans))
    assert [(r["start"], r["end"], r["spans"]) for r in regions] == want
    assert len(want) >= 3 and any(len(s) == 2 for _, _, s in want)


def test_device_route_needs_a_gpu(tiny_assembly, tmp_path):
    from roko_amd import features

    with pytest.raises(ValueError, match="extract='host'"):
        features.run(tiny_assembly["draft_fasta"], tiny_assembly["reads_bam"],
                     str(tmp_path / "o.rkw"),
                     bam_y=tiny_assembly["truth_bam"], extract="device",
                     device="cpu")
    with pytest.raises(ValueError, match="extract must be"):
        features.run(tiny_assembly["draft_fasta"], tiny_assembly["reads_bam"],
                     str(tmp_path / "o.rkw"), extract="gpu")
