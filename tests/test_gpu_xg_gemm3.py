"""xg_gemm3 (the serving xg projection at the coalesced width) must compute
exactly what xg_gemm2 computes: same MFMA, same k order, same fp32 bias add,
one bf16 round — so every comparison here is bitwise, never a tolerance."""

import pytest
import torch

from roko_amd.model import RokoModel

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs ROCm GPU"
)


def _operands(M, kreal, kp, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    A = torch.randn(M, kreal, device="cuda", generator=g).bfloat16()
    # random W is non-symmetric: a transposed tile cannot hide
    W = (torch.randn(768, kreal, device="cuda", generator=g) * 0.05).bfloat16()
    bias = (torch.randn(768, device="cuda", generator=g) * 0.1).bfloat16()
    Wp = torch.zeros(768, kp, dtype=torch.bfloat16, device="cuda")
    Wp[:, :kreal] = W
    return A.contiguous(), Wp.contiguous(), bias


def _sentinel(M):
    # a pattern no bf16 output of these operands reproduces row after row
    s = torch.arange(M * 768, device="cuda", dtype=torch.int32) % 251 + 1000
    return s.to(torch.bfloat16).view(M, 768).contiguous()


# Workgroup counts of the 128x128 tile, which the XCD remap must map one to
# one onto tiles: M = 256 -> 12, M = 2304 -> 108 = 8 * 13 + 4 (above 8 and no
# multiple of 8, the case the naive remap gets wrong), M = 11520 (the b=128
# serving shape) -> 540 = 8 * 67 + 4. Fewer workgroups than XCDs (6) is
# test_single_m_tile below.
@requires_gpu
@pytest.mark.parametrize("M", [256, 2304, 11520])
@pytest.mark.parametrize("kreal,kp", [(500, 512), (256, 256)])
def test_bitwise_equal_to_xg_gemm2(M, kreal, kp):
    from roko_amd.ops import _hip_ops as ext

    A, Wp, bias = _operands(M, kreal, kp, seed=1000 * kp + M)
    ref = ext.xg_gemm2(A, Wp, bias)
    if kreal == kp:
        a3 = A
    else:
        # the same values in a zero-padded 512-stride buffer
        a3 = torch.zeros(M, kp, dtype=torch.bfloat16, device="cuda")
        a3[:, :kreal] = A
    out = _sentinel(M)
    sent = out.clone()
    got = ext.xg_gemm3(a3, Wp, bias, out=out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    unwritten = (got == sent).all(dim=1).sum().item()
    assert torch.equal(got, ref), (
        M, kreal, (got != ref).float().mean().item(), unwritten)


@requires_gpu
def test_single_m_tile():
    """M = 128: six workgroups, fewer than XCDs. xg_gemm2 needs M % 256 == 0,
    so it runs on 256 rows and the first 128 are compared (an output row
    depends on its own A row only)."""
    from roko_amd.ops import _hip_ops as ext

    A, Wp, bias = _operands(256, 256, 256, seed=17)
    ref = ext.xg_gemm2(A, Wp, bias)[:128]
    out = _sentinel(128)
    got = ext.xg_gemm3(A[:128], Wp, bias, out=out)
    assert torch.equal(got, ref)


@requires_gpu
def test_a_with_leading_dimension():
    """A as a column slice of a wider buffer (rows 16-B aligned, stride 640)
    gives the same bytes as the contiguous copy."""
    from roko_amd.ops import _hip_ops as ext

    M = 512  # xg_gemm2, the reference, needs M % 256 == 0
    A, Wp, bias = _operands(M, 256, 256, seed=7)
    wide = torch.full((M, 640), float("nan"), dtype=torch.bfloat16,
                      device="cuda")
    wide[:, 128:384] = A
    got = ext.xg_gemm3(wide[:, 128:384], Wp, bias)
    assert torch.equal(got, ext.xg_gemm2(A, Wp, bias))


@requires_gpu
def test_front_leading_dimension():
    """embed_mlp_fwd3 into a zero-filled (90, 32, 512) buffer: the first 500
    columns equal the stride-500 output byte for byte and the pad columns
    are left untouched."""
    from roko_amd.ops import _hip_ops as ext
    from roko_amd.ops.forward import _bf16_weights

    torch.manual_seed(3)
    model = RokoModel().cuda().eval()
    w = _bf16_weights(model)
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(0, 12, (32, 200, 90), generator=g,
                        dtype=torch.uint8).cuda()
    args = (ids, w["w1g"], w["b1"], w["w2"], w["b2"], w["emb"])
    ref = ext.embed_mlp_fwd3(*args)
    assert ref.shape == (90, 32, 500)
    buf = torch.zeros(90, 32, 512, dtype=torch.bfloat16, device="cuda")
    got = ext.embed_mlp_fwd3(*args, ldo=512, out=buf)
    assert got.data_ptr() == buf.data_ptr()
    assert torch.equal(got[..., :500], ref)
    assert (got[..., 500:].view(torch.int16) == 0).all()
    # without `out` the padded result is allocated zero-filled
    got2 = ext.embed_mlp_fwd3(*args, ldo=512)
    assert torch.equal(got2.view(torch.int16), got.view(torch.int16))


@requires_gpu
def test_switch_parity(monkeypatch):
    """ROKO_XG3=0 (xg_gemm2, 500-stride front output) and the default
    (xg_gemm3, 512-stride) serve identical predictions, and the slot's plan
    shows that the switch did select the other kernel."""
    from roko_amd.ops.forward import InferencePipeline
    from tests.serve_plan_cases import expected_plan

    torch.manual_seed(9)
    model = RokoModel().cuda().eval()
    g = torch.Generator().manual_seed(13)
    x = torch.randint(0, 12, (128, 200, 90), generator=g,
                      dtype=torch.uint8).cuda()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    preds = []
    for flag in ("0", None):
        if flag is None:
            monkeypatch.delenv("ROKO_XG3", raising=False)
        else:
            monkeypatch.setenv("ROKO_XG3", flag)
        pipe = InferencePipeline(model, 128, depth=1)
        plan = pipe.slots[0].cpp.plan
        if flag == "0":
            assert plan["xg"] == ["xg2"] * 3 and plan["seq_ld"] == 500
        else:
            assert plan["xg"][0] == "xg3" and plan["seq_ld"] == 512
            assert plan["xg"] == expected_plan(128, cus)["xg"]
        preds.append(pipe.submit(x, copy_out=True)().clone())
        del pipe
    assert preds[0].shape == (128, 90)
    assert torch.equal(preds[0], preds[1])
