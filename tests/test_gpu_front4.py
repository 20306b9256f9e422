"""The persistent three-waves-per-SIMD eval front (embed_mlp_fwd4) against
embed_mlp_fwd3 on the same inputs and weights: the two must agree byte for
byte (same MFMA, same k order per output, fp32 bias, relu, one bf16 round)."""

import pytest
import torch

from roko_amd.model import RokoModel

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from roko_amd import ops
    from roko_amd.ops import forward as fwd

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs ROCm GPU"
)

_W = {}


def _weights():
    """One weight set (fixed seed) shared by every test; never modified."""
    if not _W:
        torch.manual_seed(41)
        _W["m"] = RokoModel().eval().cuda()
        _W["w"] = fwd._bf16_weights(_W["m"])
    return _W["w"]


def _args(ids):
    w = _weights()
    return (ids, w["w1g"], w["b1"], w["w2"], w["b2"], w["emb"])


def _rand_ids(B, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 12, (B, 200, 90), generator=g,
                         dtype=torch.uint8).cuda()


@requires_gpu
@pytest.mark.parametrize("B", [3, 5])
@pytest.mark.parametrize("max_blocks", [0, 2])
def test_window_loop(B, max_blocks):
    """Random ids; with max_blocks=2 a workgroup walks 2-3 windows, so what
    it carries between windows (un-scattered hot tile, zero row, prefetched
    ids) is exercised. 90 columns over 12 waves leave a six-column tail on
    waves 0 to 5 in every case."""
    ext = ops.ext()
    a = _args(_rand_ids(B, 100 + B))
    ref = ext.embed_mlp_fwd3(*a)
    got = ext.embed_mlp_fwd4(*a, max_blocks=max_blocks)
    assert got.shape == ref.shape and got.dtype == ref.dtype
    assert torch.equal(got, ref)


@requires_gpu
@pytest.mark.parametrize("case", ["all0", "all11", "alternate"])
def test_degenerate_columns(case):
    """B = 2: every read of class 0, every read of class 11, and one window
    alternating 0 and 11 by read."""
    ext = ops.ext()
    ids = torch.zeros(2, 200, 90, dtype=torch.uint8)
    if case == "all11":
        ids[:] = 11
    elif case == "alternate":
        ids[0] = _rand_ids(1, 7)[0].cpu()
        ids[1, 1::2, :] = 11
    a = _args(ids.cuda())
    assert torch.equal(ext.embed_mlp_fwd4(*a), ext.embed_mlp_fwd3(*a))


@requires_gpu
def test_output_strides():
    """ldo = 500, and ldo = 512 into a sentinel-filled caller buffer: columns
    0-499 equal v3's, columns 500-511 still hold the sentinel."""
    ext = ops.ext()
    B = 3
    a = _args(_rand_ids(B, 11))
    ref = ext.embed_mlp_fwd3(*a)
    assert torch.equal(ext.embed_mlp_fwd4(*a, ldo=500), ref)
    sentinel = -7.0
    buf = torch.full((90, B, 512), sentinel, dtype=torch.bfloat16,
                     device="cuda")
    got = ext.embed_mlp_fwd4(*a, ldo=512, out=buf)
    assert got.data_ptr() == buf.data_ptr()
    assert torch.equal(buf[:, :, :500], ref)
    assert torch.equal(buf[:, :, 500:], torch.full_like(buf[:, :, 500:],
                                                        sentinel))


@requires_gpu
def test_repeat_same_buffer():
    """Two consecutive calls into one buffer give identical bytes."""
    ext = ops.ext()
    B = 5
    a = _args(_rand_ids(B, 12))
    buf = torch.zeros(90, B, 512, dtype=torch.bfloat16, device="cuda")
    ext.embed_mlp_fwd4(*a, ldo=512, out=buf, max_blocks=2)
    first = buf.clone()
    ext.embed_mlp_fwd4(*a, ldo=512, out=buf, max_blocks=2)
    assert torch.equal(buf, first)
    assert torch.equal(buf[:, :, :500], ext.embed_mlp_fwd3(*a))


@requires_gpu
def test_v4_vs_torch():
    """Against the fp32 torch reference, with the tolerances of
    test_embed_mlp_fwd_v2_v3_vs_torch (B = 32)."""
    torch.manual_seed(21)
    m = RokoModel().eval()
    B = 32
    x = torch.randint(0, 12, (B, 200, 90))
    with torch.no_grad():
        e = m.embedding(x)
        t = torch.relu(m.fc1(e.permute(0, 2, 3, 1)))
        t = torch.relu(m.fc2(t))
        ref = t.reshape(B, 90, 500).transpose(0, 1)

    m = m.cuda()
    w = fwd._bf16_weights(m)
    ext = ops.ext()
    out = ext.embed_mlp_fwd4(x.to(torch.uint8).cuda(), w["w1g"], w["b1"],
                             w["w2"], w["b2"], w["emb"])
    got = out.float().cpu()
    err = (got - ref).abs()
    scale = ref.abs().mean().item() + 1e-6
    assert err.max().item() < 0.08, err.max().item()
    assert err.mean().item() / scale < 0.02
