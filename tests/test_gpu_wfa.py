"""The wavefront aligner on the GPU (ops/hip/wfa.hip): its op string must equal
the C++ route's (`_pileup.wfa_ops`) byte for byte.

The step kernel gives one thread a diagonal and one 256-thread workgroup 256
of them; a lane compares PROBE bytes alone, then its wave extends the run
COOP bytes a round; the driver enqueues the scores in chunks whose bounds are
`wfa.chunk_bounds()`. The cases below are chosen against those numbers."""

import numpy as np
import pytest
import torch

from roko_amd import accuracy, wfa
from roko_amd.wfa import COOP, PROBE

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs ROCm GPU"
)

OTHER = {"A": "C", "C": "G", "G": "T", "T": "A"}


def _rand(rng, alphabet, n):
    return "".join(rng.choice(list(alphabet), n)) if n else ""


def _sub(seq, positions):
    s = list(seq)
    for p in positions:
        s[p] = OTHER[s[p]]
    return "".join(s)


def _check(q, t):
    """Device ops against the C++ route; returns the device result."""
    from roko_amd.ops import pileup_ext

    want = pileup_ext().wfa_ops(q, t)
    got = wfa.align(q, t, device=True)
    assert got["route"] == "device"
    assert got["ops"] == want, (len(q), len(t), len(want))
    return got


@requires_gpu
def test_constants_match_kernel():
    from roko_amd import ops

    ext = ops.ext()
    assert (ext.wfa_probe(), ext.wfa_coop()) == (PROBE, COOP)
    assert ext.wfa_pad() >= COOP and ext.wfa_pad() == wfa.PAD
    for n, m, s0, s1 in [(0, 0, 0, 1), (5, 900, 0, 64), (900, 5, 64, 192),
                         (300, 300, 192, 301)]:
        assert ext.wfa_dir_cells(n, m, s0, s1) == wfa.dir_cells(n, m, s0, s1)


@requires_gpu
def test_identical_prefix_suffix(rng):
    for n in (0, 1, PROBE - 1, PROBE + 1, COOP - 1, COOP, COOP + 1,
              8 * COOP + 1):
        s = _rand(rng, "ACGT", n)
        assert _check(s, s)["ops"] == b""
        full = s + _rand(rng, "ACGT", 5)
        assert _check(s, full)["ops"] == b"D" * 5      # strict prefix
        full = "G" + _rand(rng, "ACGT", 4) + s
        assert _check(s, full)["ops"] == b"D" * 5      # strict suffix
        assert _check(full, s)["ops"] == b"I" * 5


@requires_gpu
def test_one_edit_of_each_kind(rng):
    t = _rand(rng, "ACGT", 1000)
    for p in (0, 1, COOP - 1, COOP, len(t) - 1):
        assert _check(_sub(t, [p]), t)["edit_distance"] == 1
        assert _check(t[:p] + t[p + 1:], t)["ops"] == b"D"
        assert _check(t[:p] + OTHER[t[p]] + t[p:], t)["ops"] == b"I"


@requires_gpu
def test_match_runs_between_edits(rng):
    t = _rand(rng, "ACGT", 1500)
    for run in (PROBE - 1, PROBE, PROBE + 1, COOP - 1, COOP, COOP + 1,
                2 * COOP + 1):
        for start in (0, 37):
            # exactly `run` matching bases between two substitutions
            q = _sub(t, [start, start + run + 1])
            assert _check(q, t)["edit_distance"] == 2
            q = t[:start] + t[start + 1:start + run + 1] + t[start + run + 2:]
            assert _check(q, t)["edit_distance"] == 2
    # two runs open in one wave in the same step: at score 1 diagonal 0 (X)
    # runs COOP bases and diagonal 1 (D) COOP + 1
    q = "A" * (COOP + 1) + "GT"
    assert _check(q, "C" + q)["ops"] == b"D"
    q = "A" * (2 * COOP + 1) + "GT"
    _check(q, "C" + q[:-2] + "AGT")
    _check("C" + q[:-2] + "AGT", q)


@requires_gpu
def test_low_complexity_pairs(rng):
    for it in range(200):
        n, m = (int(x) for x in rng.integers(0, 301, 2))
        kind = it % 4
        if kind == 0:      # unrelated AC
            q, t = _rand(rng, "AC", n), _rand(rng, "AC", m)
        elif kind == 1:    # homopolymers
            q, t = "A" * n, "A" * m
        elif kind == 2:    # homopolymer runs of differing lengths
            q = "".join(c * int(rng.integers(1, 12))
                        for c in _rand(rng, "AC", n // 6))
            t = "".join(c * int(rng.integers(1, 12))
                        for c in _rand(rng, "AC", m // 6))
        else:              # related AC
            q = _rand(rng, "AC", n)
            t = list(q)
            for _ in range(int(rng.integers(0, 10))):
                t.insert(int(rng.integers(len(t) + 1)), "AC"[it // 4 % 2])
            t = "".join(t)[:300]
        _check(q, t)


@requires_gpu
def test_clipped_wavefronts(rng):
    _check(_rand(rng, "ACGT", 400), _rand(rng, "ACGT", 400))
    short, long_ = _rand(rng, "ACGT", 50), _rand(rng, "ACGT", 2000)
    assert _check(short, long_)["edit_distance"] >= 1950
    assert _check(long_, short)["edit_distance"] >= 1950


@requires_gpu
def test_chunk_bounds(rng):
    from roko_amd.ops import pileup_ext

    it = wfa.chunk_bounds()
    bounds = [next(it) for _ in range(3)]
    t = _rand(rng, "ACGT", 16 * (bounds[-1] + 2))
    for b in bounds:
        for dist in (b - 1, b, b + 1):
            q = _sub(t, range(5, 5 + 16 * dist, 16))
            # isolated substitutions: the distance is their number
            assert len(pileup_ext().wfa_ops(q, t)) == dist
            assert _check(q, t)["ops"] == b"X" * dist


@requires_gpu
def test_wavefront_wider_than_workgroups(rng):
    got = _check(_rand(rng, "ACGT", 1500), _rand(rng, "ACGT", 1400))
    assert got["edit_distance"] > 640


@pytest.fixture(scope="module")
def pair_200k():
    from tests.simple_align import EditScript

    rng = np.random.default_rng(99)
    truth = _rand(rng, "ACGT", 200_000)
    # 1.4 % in the sub/ins/del mix of the draft generator
    return EditScript(rng, truth, 0.007, 0.0035, 0.0035).draft, truth


@requires_gpu
def test_200kb_pair(pair_200k):
    draft, truth = pair_200k
    cpu = wfa.align(draft, truth, device=False)
    dev = _check(draft, truth)
    assert 2000 < dev["edit_distance"] < 3600
    assert {k: v for k, v in dev.items() if k != "route"} == \
        {k: v for k, v in cpu.items() if k != "route"}
    st = accuracy.seq_stats(draft, truth, aligner="wfa")
    assert st["route"] == "device"
    want = accuracy._rates(cpu, len(truth))
    assert {k: st[k] for k in want} == want
    assert st["band"] == 0 and st["aligner"] == "wfa"


@requires_gpu
def test_budget_and_limits(rng):
    t = _rand(rng, "ACGT", 3000)
    q = _sub(t, range(3, 3 + 20 * 100, 20))  # distance 100: two chunks
    first = wfa.dir_cells(len(q), len(t), 0, wfa.CHUNK_FIRST)
    with pytest.raises(wfa.BudgetError):
        wfa.align(q, t, device=True, budget_bytes=first - 1)
    with pytest.raises(wfa.BudgetError):   # the second chunk does not fit
        wfa.align(q, t, device=True, budget_bytes=first)
    assert _check(q, t)["edit_distance"] == 100
    with pytest.raises(wfa.ScoreLimitError):
        wfa.align(q, t, device=True, max_score=99)
    assert wfa.align(q, t, device=True, max_score=100)["ops"] == b"X" * 100
    # below DEVICE_MIN_SCORE the C++ route is the faster one and the default
    assert wfa.DEVICE_MIN_SCORE > 100
    assert wfa.align(q, t)["route"] == "cpu"
    assert _check(q, t)["edit_distance"] == 100


@requires_gpu
def test_invalid_input_raises_before_upload():
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for bad in ("AC\x01GT", "AC\x00GT", b"AC\xffGT", "AC\nGT"):
        with pytest.raises(ValueError):
            wfa.align(bad, "ACGT", device=True)
        with pytest.raises(ValueError):
            wfa.align("ACGT", bad, device=True)
    assert torch.cuda.memory_allocated() == before
