"""The transposed eval GRU kernel (gru_layer_fwd impl=2, the default) against
the LDS-staged 16-row kernel (impl=1) on the same inputs: hseq must agree byte
for byte (same MFMAs in the same k order with the operand roles swapped, the
same gate expressions, one bf16 round)."""

import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from roko_amd import ops

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs ROCm GPU"
)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OLD, NEW = 1, 2
# a bf16 NaN with a payload: every h is a blend of values in [-1, 1], and a
# NaN a kernel computes carries no such payload
SENTINEL = 0x7FA5

_IN = {}


def _inputs(T, B):
    """xg ~ N(0, 0.3^2), U ~ N(0, 0.2^2), bhh ~ N(0, 1) as
    scripts/gru_timing.py draws them; one fixed set per shape, shared and
    never modified."""
    if (T, B) not in _IN:
        g = torch.Generator().manual_seed(1000 * T + B)
        xg = (torch.randn(T, B, 2, 384, generator=g) * 0.3).to(torch.bfloat16)
        u = (torch.randn(2, 384, 128, generator=g) * 0.2).to(torch.bfloat16)
        bhh = torch.randn(2, 384, generator=g)
        _IN[(T, B)] = (xg.cuda(), u.cuda(), bhh.cuda())
    return _IN[(T, B)]


def _run(xg, u, bhh, impl):
    """One launch into a sentinel-filled buffer; asserts every element was
    written."""
    T, B = xg.shape[:2]
    out = torch.empty(T, B, 2, 128, dtype=torch.bfloat16, device="cuda")
    out.view(torch.int16).fill_(SENTINEL)
    (got,) = ops.ext().gru_layer_fwd(xg, u, bhh, False, 0, impl=impl, out=out)
    assert got.data_ptr() == out.data_ptr()
    left = int((out.view(torch.int16) == SENTINEL).sum())
    assert left == 0, f"impl={impl}: {left} elements never written"
    return out


@requires_gpu
@pytest.mark.parametrize("T,B", [(1, 16), (2, 16), (3, 16), (4, 32), (5, 48),
                                 (7, 16), (90, 16), (90, 128)])
def test_equals_old_kernel(T, B):
    """Every tail of the unrolled loop and the clamped prefetch at both ends
    of both directions (T = 1..7), one tile, an odd tile count (B = 48), the
    workload's T."""
    xg, u, bhh = _inputs(T, B)
    old = _run(xg, u, bhh, OLD)
    new = _run(xg, u, bhh, NEW)
    for d, name in ((0, "forward"), (1, "reverse")):
        assert torch.equal(new[:, :, d], old[:, :, d]), (
            f"{name} direction differs at T={T} B={B}: "
            f"{int((new[:, :, d] != old[:, :, d]).sum())} elements")


@requires_gpu
@pytest.mark.parametrize("impl", [3, 4])
@pytest.mark.parametrize("T,B", [(1, 16), (3, 16), (5, 48), (90, 32)])
def test_timing_variants_equal_old_kernel(impl, T, B):
    """The two forms only scripts/gru_eval2_timing.py launches (3: hseq
    stored from registers, 4: xg staged through LDS) compute the same
    bytes."""
    xg, u, bhh = _inputs(T, B)
    assert torch.equal(_run(xg, u, bhh, impl), _run(xg, u, bhh, OLD))


@requires_gpu
def test_default_is_new_kernel():
    ext = ops.ext()
    if os.environ.get("ROKO_GRU_EVAL") == "v1" or \
            os.environ.get("ROKO_GRU_MB") == "32":
        assert ext.gru_eval_impl(128) == OLD
    else:
        assert ext.gru_eval_impl(128) == NEW
    assert ext.gru_eval_impl(128, impl=OLD) == OLD
    assert ext.gru_eval_impl(128, impl=NEW) == NEW


@requires_gpu
def test_one_tile_against_all():
    """B = 64, then rows 16-31 alone as a B = 16 call on a contiguous copy:
    a tile depends on nothing but its own rows (b0 addressing)."""
    xg, u, bhh = _inputs(6, 64)
    full = _run(xg, u, bhh, NEW)
    part = _run(xg[:, 16:32].contiguous(), u, bhh, NEW)
    for d, name in ((0, "forward"), (1, "reverse")):
        assert torch.equal(part[:, :, d], full[:, 16:32, d]), name


@requires_gpu
def test_vs_torch_gru():
    """Against torch.nn.GRU in fp32, inputs and tolerances of
    test_gru_layer_fwd_vs_torch (T = 90, B = 32)."""
    torch.manual_seed(2)
    T, B, H = 90, 32, 128
    gru = torch.nn.GRU(256, H, num_layers=1, batch_first=False,
                       bidirectional=True)
    x = torch.randn(T, B, 256) * 0.5
    with torch.no_grad():
        ref, _ = gru(x)
    w_ih = torch.cat([gru.weight_ih_l0, gru.weight_ih_l0_reverse], 0)
    b_ih = torch.cat([gru.bias_ih_l0, gru.bias_ih_l0_reverse])
    xg = (x.reshape(T * B, 256) @ w_ih.t() + b_ih).view(T, B, 2, 384)
    u = torch.stack([gru.weight_hh_l0, gru.weight_hh_l0_reverse])
    bhh = torch.stack([gru.bias_hh_l0, gru.bias_hh_l0_reverse])
    hseq = _run(xg.to(torch.bfloat16).cuda().contiguous(),
                u.to(torch.bfloat16).cuda().contiguous(),
                bhh.float().cuda().contiguous(), NEW)
    err = (hseq.view(T, B, 256).float().cpu() - ref).abs()
    assert err.max().item() < 0.1, err.max().item()
    assert err.mean().item() < 0.01, err.mean().item()


_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import torch
from roko_amd import ops
ext = ops.ext()
g = torch.Generator().manual_seed(5)
xg = (torch.randn(5, 32, 2, 384, generator=g) * 0.3).to(torch.bfloat16).cuda()
u = (torch.randn(2, 384, 128, generator=g) * 0.2).to(torch.bfloat16).cuda()
bhh = torch.randn(2, 384, generator=g).cuda()
assert ext.gru_eval_impl(32) == 1, ext.gru_eval_impl(32)
assert ext.gru_eval_impl(32, impl=2) == 2
# mask 2 (no cache store) is a mask of the old kernel only: the new kernel
# refuses it, so this call succeeds only if the default is the old kernel
(dflt,) = ext.gru_layer_fwd(xg, u, bhh, False, 2)
(old,) = ext.gru_layer_fwd(xg, u, bhh, False, 0, impl=1)
(new,) = ext.gru_layer_fwd(xg, u, bhh, False, 0, impl=2)
try:
    ext.gru_layer_fwd(xg, u, bhh, False, 2, impl=2)
except (ValueError, RuntimeError):
    pass
else:
    raise AssertionError("impl=2 accepted a mask of the old kernel")
torch.cuda.synchronize()
assert torch.equal(dflt, old) and torch.equal(new, old)
print("child ok")
"""


@requires_gpu
def test_toggle_selects_old_kernel():
    """impl= selects what it says, and ROKO_GRU_EVAL=v1 (read once per
    process, hence the fresh child) makes the old kernel the default."""
    ext = ops.ext()
    xg, u, bhh = _inputs(2, 16)
    with pytest.raises((ValueError, RuntimeError)):
        ext.gru_layer_fwd(xg, u, bhh, False, 2, impl=NEW)
    ext.gru_layer_fwd(xg, u, bhh, False, 2, impl=OLD)  # accepted
    env = dict(os.environ, ROKO_GRU_EVAL="v1")
    env.pop("ROKO_GRU_MB", None)
    out = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=env,
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "child ok" in out.stdout
