"""xg_gemm4 is xg_gemm3 with the tiles strung into one slice stream per
persistent workgroup, in two forms: "stream" (xg_gemm3's tile, both K) and
"wstat" (K = 256: W stationary in LDS, 256-row tiles, one workgroup per CU).
Same MFMA chain, same k order, same fp32 bias add, one bf16 round: every
comparison here is bitwise against xg_gemm3, into sentinel-filled outputs,
at the smallest shapes where the walk, the XCD placement and the tile
boundary can go wrong."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.serve_plan_cases import expected_plan

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs ROCm GPU"
)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _operands(M, kreal, kp, seed):
    """A zero-padded to kp columns (the layer-0 form when kreal = 500), the
    padded non-symmetric W image, bias."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    A = torch.zeros(M, kp, dtype=torch.bfloat16, device="cuda")
    A[:, :kreal] = torch.randn(M, kreal, device="cuda", generator=g).bfloat16()
    Wp = torch.zeros(768, kp, dtype=torch.bfloat16, device="cuda")
    Wp[:, :kreal] = (torch.randn(768, kreal, device="cuda", generator=g)
                     * 0.05).bfloat16()
    bias = (torch.randn(768, device="cuda", generator=g) * 0.1).bfloat16()
    return A, Wp, bias


def _sentinel(M):
    # a pattern no bf16 output of these operands reproduces row after row
    s = torch.arange(M * 768, device="cuda", dtype=torch.int32) % 251 + 1000
    return s.to(torch.bfloat16).view(M, 768).contiguous()


class _Refs:
    """Operands and the xg_gemm3 output per (M, kreal, kp): computed once,
    shared by every case, never written again."""

    def __init__(self):
        self._d = {}

    def get(self, M, kreal, kp):
        key = (M, kreal, kp)
        if key not in self._d:
            from roko_amd.ops import _hip_ops as ext

            A, Wp, bias = _operands(M, kreal, kp, seed=1000 * kp + M)
            ref = ext.xg_gemm3(A, Wp, bias, out=_sentinel(M))
            torch.cuda.synchronize()
            self._d[key] = (A, Wp, bias, ref)
        return self._d[key]


@pytest.fixture(scope="module")
def refs():
    return _Refs()


# Tiles: M = 128 -> 6 (one m-tile; with the default grid and with max_wgs = 7
# the cap exceeds the tile count), 256 -> 12, 2304 -> 108. max_wgs = 1 walks
# every tile in one workgroup and so crosses every boundary kind (n -> n + 1
# and an m-tile change); 2 / 5 / 7 give unequal runs and workgroup counts
# below and not dividing the 8 XCDs; 0 is the default grid. 20 is the one
# count here with several workgroups per XCD (3, 3, 3, 3, 2, 2, 2, 2) AND
# several tiles per workgroup: the strided walk inside an XCD's tile range.
#
# The W-stationary form exists for K = 256 and M % 256 == 0 only, and caps
# its grid at 6 x max(1, max_wgs // 6) workgroups: 1 / 2 / 5 / 7 are one
# walker per n-tile over every m-tile, 20 is three, 0 is one per m-tile.
def _cases():
    out = []
    for M in (128, 256, 2304):
        for kreal, kp in ((500, 512), (256, 256)):
            for max_wgs in (1, 2, 5, 7, 20, 0):
                out.append((M, kreal, kp, max_wgs, "stream"))
                if kp == 256 and M % 256 == 0:
                    out.append((M, kreal, kp, max_wgs, "wstat"))
    return out


@requires_gpu
@pytest.mark.parametrize("M,kreal,kp,max_wgs,form", _cases())
def test_bitwise_equal_to_xg_gemm3(refs, M, kreal, kp, max_wgs, form):
    from roko_amd.ops import _hip_ops as ext

    A, Wp, bias, ref = refs.get(M, kreal, kp)
    out = _sentinel(M)
    sent = out.clone()
    got = ext.xg_gemm4(A, Wp, bias, out=out, max_wgs=max_wgs, form=form)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    unwritten = (got == sent).all(dim=1).sum().item()
    assert torch.equal(got, ref), (
        M, kp, max_wgs, form, (got != ref).float().mean().item(), unwritten)


@requires_gpu
@pytest.mark.parametrize("M,max_wgs", [(2304, 48), (5888, 96)])
def test_wstat_xcd_walk(refs, M, max_wgs):
    """Walker counts that are a multiple of 8 take the XCD placement: each
    XCD a contiguous eighth of the m-tiles. 9 m-tiles on 8 walkers: one XCD
    has two tiles, seven have one. 23 on 16: two walkers per XCD striding
    through ranges of 3, ..., 3, 2 tiles, so one walker walks two tiles and
    its partner one."""
    from roko_amd.ops import _hip_ops as ext

    A, Wp, bias, ref = refs.get(M, 256, 256)
    got = ext.xg_gemm4(A, Wp, bias, out=_sentinel(M), max_wgs=max_wgs,
                       form="wstat")
    assert torch.equal(got, ref)


@requires_gpu
def test_auto_form(refs):
    """No keyword at all: W-stationary where it applies, else the stream;
    a shape the W-stationary form cannot take is refused, not rerouted."""
    from roko_amd.ops import _hip_ops as ext

    assert ext.xg_gemm4_cus() >= 1
    for M, kreal, kp in ((2304, 256, 256), (128, 256, 256), (256, 500, 512)):
        A, Wp, bias, ref = refs.get(M, kreal, kp)
        assert torch.equal(ext.xg_gemm4(A, Wp, bias), ref)
    A, Wp, bias, _ = refs.get(128, 256, 256)
    with pytest.raises((ValueError, RuntimeError)):
        ext.xg_gemm4(A, Wp, bias, form="wstat")


@requires_gpu
@pytest.mark.parametrize("form", ["stream", "wstat"])
@pytest.mark.parametrize("max_wgs", [1, 5, 0])
def test_a_with_leading_dimension(refs, max_wgs, form):
    """A as a column slice of a wider NaN-filled buffer (rows 16-B aligned,
    stride 640): the same bytes as the contiguous copy. A look-ahead that
    strays out of its tile's columns would pull a NaN in."""
    from roko_amd.ops import _hip_ops as ext

    A, Wp, bias, ref = refs.get(256, 256, 256)
    wide = torch.full((256, 640), float("nan"), dtype=torch.bfloat16,
                      device="cuda")
    wide[:, 128:384] = A
    got = ext.xg_gemm4(wide[:, 128:384], Wp, bias, out=_sentinel(256),
                       max_wgs=max_wgs, form=form)
    assert torch.equal(got, ref)


@requires_gpu
def test_layer0_padded_form_matches_xg_gemm2(refs):
    """The 512-stride zero-padded layer-0 form against the kernel that reads
    the unpadded 500-stride rows: the chain back to xg_gemm2 holds."""
    from roko_amd.ops import _hip_ops as ext

    A, Wp, bias, _ = refs.get(256, 500, 512)
    ref2 = ext.xg_gemm2(A[:, :500].contiguous(), Wp, bias)
    got = ext.xg_gemm4(A, Wp, bias, out=_sentinel(256), max_wgs=5,
                       form="stream")
    assert torch.equal(got, ref2)


@requires_gpu
@pytest.mark.parametrize("kreal,kp,form", [(500, 512, "stream"),
                                           (256, 256, "stream"),
                                           (256, 256, "wstat")])
def test_schedule_screen(kreal, kp, form):
    """The barrier structure at the tile boundary is new: 25 launches on
    fresh random operands at a fixed small shape, each equal to xg_gemm3.
    max_wgs = 5: the stream walks 108 tiles on 5 workgroups (21 or 22
    boundaries each), the W-stationary form 9 m-tiles on one walker per
    n-tile (8 boundaries each). A screen of a correct schedule, not a
    stress loop."""
    from roko_amd.ops import _hip_ops as ext

    M = 2304
    bad = []
    for i in range(25):
        A, Wp, bias = _operands(M, kreal, kp, seed=7000 + 31 * i + kp)
        ref = ext.xg_gemm3(A, Wp, bias)
        got = ext.xg_gemm4(A, Wp, bias, out=_sentinel(M), max_wgs=5,
                           form=form)
        if not torch.equal(got, ref):
            bad.append(i)
    assert not bad, bad


_CHILD = r"""
import json
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import torch
from roko_amd.model import RokoModel
from roko_amd.ops.forward import InferencePipeline
torch.manual_seed(9)
model = RokoModel().cuda().eval()
g = torch.Generator().manual_seed(13)
xs = [torch.randint(0, 12, (128, 200, 90), generator=g,
                    dtype=torch.uint8).cuda() for _ in range(2)]
pipe = InferencePipeline(model, 128, depth=2, coalesce=2)
assert pipe.coalesce == 2 and len(pipe.slots) == 1
print("plan", json.dumps(pipe.slots[0].cpp.plan))
tickets = [pipe.submit(x, copy_out=True) for x in xs]
preds = torch.stack([t().clone() for t in tickets])
assert preds.shape == (2, 128, 90)
np.save(sys.argv[2], preds.cpu().numpy())
print("child ok")
"""


@requires_gpu
def test_switch_parity(tmp_path):
    """ROKO_XG4=0 (xg_gemm3), =stream, =wstat and the default serve identical
    predictions. One slot of width 256: 1,080 tiles of the stream on 512
    workgroups and 90 m-tiles on 40 walkers, so every workgroup of either
    grid walks more than one tile. (The default takes the W-stationary
    kernel only from eight rounds per walker up, i.e. at the shipped width
    1024, which tests/test_gpu_coalesce.py serves against narrow
    references.) Fresh children: the switch is read when a slot is built,
    and each run starts from a clean process as serving does; the four run
    side by side so the test costs one start-up, not four."""
    flags = ("0", "stream", "wstat", None)
    procs = []
    for flag in flags:
        env = dict(os.environ)
        env.pop("ROKO_XG4", None)
        if flag is not None:
            env["ROKO_XG4"] = flag
        path = str(tmp_path / f"preds_{flag}.npy")
        procs.append((path, subprocess.Popen(
            [sys.executable, "-c", _CHILD, ROOT, path], env=env,
            stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)))
    # what each child's slot (width 256) must have chosen, so that equal
    # predictions mean different kernels agreed
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    want = {"0": ["xg3"] * 3, "stream": ["stream"] * 3,
            "wstat": ["xg3", "wstat", "wstat"],
            None: expected_plan(256, cus)["xg"]}
    preds = []
    for flag, (path, proc) in zip(flags, procs):
        stdout, stderr = proc.communicate(timeout=300)
        assert proc.returncode == 0, stderr[-2000:]
        assert "child ok" in stdout
        plan = json.loads(next(l for l in stdout.splitlines()
                               if l.startswith("plan "))[5:])
        assert plan["xg"] == want[flag], (flag, plan)
        preds.append(np.load(path))
    assert preds[0].shape == (2, 128, 90)
    assert np.array_equal(preds[0], preds[1])
    assert np.array_equal(preds[0], preds[2])
    assert np.array_equal(preds[0], preds[3])
