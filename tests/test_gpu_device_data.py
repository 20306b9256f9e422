"""The device data route on the GPU: gather_batch against torch indexing
(bit for bit, 64-bit row offsets included), the resident upload against the
file reader, train(data="device") batch by batch against the host arrays,
and evaluate_device against evaluate()."""

import glob
import os

import numpy as np
import pytest
import torch

from roko_amd import config as C
from tests.device_data_cases import two_file_dir, write_rkw

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs ROCm GPU"
)


def _ext():
    from roko_amd import ops

    return ops.ext()


def _gather(X, Y, idx):
    """gather_batch into buffers pre-filled with 0xFF / -1, so an unwritten
    row tail (the last 16-byte vector, label column 89) would show."""
    B = idx.numel()
    out_x = torch.full((B, C.WINDOW_ROWS, C.WINDOW_COLS), 0xFF,
                       dtype=torch.uint8, device="cuda")
    out_y = torch.full((B, C.WINDOW_COLS), -1, dtype=torch.int64,
                       device="cuda")
    _ext().gather_batch(X, Y, idx, out_x, out_y)
    return out_x, out_y


@requires_gpu
def test_gather_is_exact():
    g = torch.Generator().manual_seed(0)
    N = 300
    X = torch.randint(0, C.NUM_BASE_IDS, (N, C.WINDOW_ROWS, C.WINDOW_COLS),
                      generator=g, dtype=torch.uint8).cuda()
    Y = torch.randint(0, C.NUM_CLASSES, (N, C.WINDOW_COLS), generator=g,
                      dtype=torch.uint8).cuda()
    cases = [[0], [N - 1]]  # B = 1 holds one row: both ends in turn
    for B in (7, 32, 33):
        rows = torch.randint(0, N, (B,), generator=g).tolist()
        rows[0], rows[1], rows[-1] = N - 1, 0, rows[2]  # ends + a repeat
        cases.append(rows)
    for rows in cases:
        idx = torch.tensor(rows, dtype=torch.int32, device="cuda")
        out_x, out_y = _gather(X, Y, idx)
        sel = idx.long()
        assert torch.equal(out_x, X[sel]), len(rows)
        assert torch.equal(out_y, Y[sel].long()), len(rows)


@requires_gpu
def test_gather_binding_rejects_mismatches():
    X = torch.zeros((4, C.WINDOW_ROWS, C.WINDOW_COLS), dtype=torch.uint8,
                    device="cuda")
    Y = torch.zeros((4, C.WINDOW_COLS), dtype=torch.uint8, device="cuda")
    idx = torch.zeros(2, dtype=torch.int32, device="cuda")
    ox = torch.zeros((2, C.WINDOW_ROWS, C.WINDOW_COLS), dtype=torch.uint8,
                     device="cuda")
    oy = torch.zeros((2, C.WINDOW_COLS), dtype=torch.int64, device="cuda")
    ext = _ext()
    ext.gather_batch(X, Y, idx, ox, oy)
    with pytest.raises(RuntimeError, match="dtype"):
        ext.gather_batch(X, Y, idx.long(), ox, oy)
    with pytest.raises(RuntimeError, match="dtype"):
        ext.gather_batch(X, Y, idx, ox, oy.int())
    with pytest.raises(RuntimeError, match="GPU"):
        ext.gather_batch(X, Y, idx.cpu(), ox, oy)
    with pytest.raises(RuntimeError, match="contiguous"):
        ext.gather_batch(X, Y, idx, ox, oy.t().contiguous().t())
    with pytest.raises(RuntimeError, match=r"\(B, 200, 90\)"):
        ext.gather_batch(X, Y, idx, ox[:1], oy)
    row = C.WINDOW_ROWS * C.WINDOW_COLS
    shifted = X.view(-1)[8:8 + 3 * row].view(3, C.WINDOW_ROWS, C.WINDOW_COLS)
    with pytest.raises(RuntimeError, match="16-byte"):
        ext.gather_batch(shifted, Y[:3], idx, ox, oy)


@requires_gpu
def test_gather_64bit_row_offsets():
    """Rows past 238,609 start beyond 2^32 bytes. The big tensor is left
    uninitialised but for the 100 rows read, so allocation is the only
    cost."""
    free, _ = torch.cuda.mem_get_info()
    if free < 6 << 30:
        pytest.skip(f"needs 6 GB of free device memory, {free >> 30} GB free")
    N, lo, n = 238_700, 238_600, 100
    assert lo * C.WINDOW_ROWS * C.WINDOW_COLS < 2**32 \
        < (N - 1) * C.WINDOW_ROWS * C.WINDOW_COLS
    X = torch.empty((N, C.WINDOW_ROWS, C.WINDOW_COLS), dtype=torch.uint8,
                    device="cuda")
    Y = torch.empty((N, C.WINDOW_COLS), dtype=torch.uint8, device="cuda")
    g = torch.Generator().manual_seed(1)
    px = torch.randint(0, 256, (n, C.WINDOW_ROWS, C.WINDOW_COLS), generator=g,
                       dtype=torch.uint8).cuda()
    py = torch.randint(0, 256, (n, C.WINDOW_COLS), generator=g,
                       dtype=torch.uint8).cuda()
    X[lo:lo + n] = px
    Y[lo:lo + n] = py
    order = torch.randperm(n, generator=g)
    idx = (order + lo).to(torch.int32).cuda()
    out_x, out_y = _gather(X, Y, idx)
    assert torch.equal(out_x, px[order.cuda()])
    assert torch.equal(out_y, py[order.cuda()].long())


@requires_gpu
def test_device_train_data_equals_reader(tmp_path, rng):
    from roko_amd.ops.device_data import (WINDOW_BYTES, DeviceTrainData,
                                          load_rkw_arrays)

    d = two_file_dir(tmp_path, rng)
    chunks = list(load_rkw_arrays(d))
    x = np.concatenate([c[0] for c in chunks])
    y = np.concatenate([c[1] for c in chunks])
    data = DeviceTrainData(d, torch.device("cuda", 0))
    assert len(data) == 9 and data.nbytes == 9 * WINDOW_BYTES
    assert data.x.dtype == torch.uint8 and data.y.dtype == torch.uint8
    assert np.array_equal(data.x.cpu().numpy(), x)
    assert np.array_equal(data.y.cpu().numpy(), y)
    # the one range check of an epoch is on the host, before the upload
    for bad in ([0, 9], [-1, 3]):
        with pytest.raises(ValueError, match="outside"):
            data.upload_indices(np.array(bad))
    with pytest.raises(ValueError, match="--data host"):
        DeviceTrainData(d, torch.device("cuda", 0), n_other=10**12)


@requires_gpu
def test_upload_crosses_staging_chunks(tmp_path, rng, monkeypatch):
    """With staging buffers smaller than a group, the upload splits blobs
    across both buffers and wraps round them several times."""
    from roko_amd.ops import device_data as DD

    d = two_file_dir(tmp_path, rng)
    monkeypatch.setattr(DD, "STAGE_BYTES", 10_000)
    data = DD.DeviceTrainData(d, torch.device("cuda", 0))
    chunks = list(DD.load_rkw_arrays(d))
    assert np.array_equal(data.x.cpu().numpy(),
                          np.concatenate([c[0] for c in chunks]))
    assert np.array_equal(data.y.cpu().numpy(),
                          np.concatenate([c[1] for c in chunks]))


@requires_gpu
def test_train_route_draws_the_epoch_permutation(tmp_path, rng, monkeypatch):
    import roko_amd.ops.train as OT
    from roko_amd.config import TrainConfig
    from roko_amd.ops.device_data import epoch_indices, load_rkw_arrays
    from roko_amd.train import train

    path = write_rkw(str(tmp_path / "t.rkw"), [200, 61], rng)
    chunks = list(load_rkw_arrays(path))
    hx = np.concatenate([c[0] for c in chunks])
    hy = np.concatenate([c[1] for c in chunks])

    seen = []
    real_step = OT.fused_train_step

    def recorder(model, x, y, opt=None, reducer=None):
        seen.append((x.clone(), y.clone()))
        return real_step(model, x, y, opt, reducer)

    monkeypatch.setattr(OT, "fused_train_step", recorder)
    out = str(tmp_path / "ckpt")
    logs = []
    seed = 3
    cfg = TrainConfig(batch_size=32, epochs=2, seed=seed, data="device")
    _, hist = train(path, out, cfg=cfg, log=logs.append)

    assert len(hist) == 2 and len(seen) == 16  # 261 // 32 = 8 steps an epoch
    for e in (1, 2):
        idx = epoch_indices(261, 32, seed, e)
        for k in range(8):
            x, y = seen[8 * (e - 1) + k]
            assert x.dtype == torch.uint8 and y.dtype == torch.int64
            rows = idx[32 * k:32 * k + 32]
            assert np.array_equal(x.cpu().numpy(), hx[rows]), (e, k)
            assert np.array_equal(y.cpu().numpy(), hy[rows].astype(np.int64)), \
                (e, k)
    text = "\n".join(str(m) for m in logs)
    assert "data: device (261 windows" in text, text
    assert "fused HIP step" in text, text
    assert glob.glob(os.path.join(out, "rnn_model_*.pth"))
    assert os.path.exists(os.path.join(out, "train_state.pt"))


@requires_gpu
def test_evaluate_device_matches_evaluate(tmp_path, rng):
    from torch.utils.data import DataLoader

    from roko_amd.datasets import TrainDataset
    from roko_amd.model import RokoModel
    from roko_amd.ops.device_data import DeviceTrainData, evaluate_device
    from roko_amd.train import evaluate

    path = write_rkw(str(tmp_path / "v.rkw"), [60, 40], rng)
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = RokoModel().to(dev).eval()
    ref_acc, ref_loss = evaluate(
        model, DataLoader(TrainDataset(path), batch_size=32), dev)
    model.eval()
    acc, loss = evaluate_device(model, DeviceTrainData(path, dev), 32)
    print(f"acc {acc!r} vs {ref_acc!r}; loss {loss!r} vs {ref_loss!r}")
    assert 0.0 < ref_acc < 1.0
    assert acc == ref_acc
    assert abs(loss - ref_loss) < 1e-4


@requires_gpu
def test_eval_metrics_ties_and_accumulation():
    """Five tied classes predict class 0 (the smallest id, as head.hip); the
    buffer accumulates over calls: counts add, per-batch mean losses add."""
    ext = _ext()
    acc = torch.zeros(2, dtype=torch.int64, device="cuda")
    logits = torch.full((4, C.WINDOW_COLS, C.NUM_CLASSES), 0.25, device="cuda")
    n = 4 * C.WINDOW_COLS
    zeros = torch.zeros((4, C.WINDOW_COLS), dtype=torch.uint8, device="cuda")
    ext.eval_metrics(logits, zeros, 1.0 / n, acc)
    host = acc.cpu()
    assert int(host[0]) == n
    assert abs(float(host.view(torch.float64)[1]) - np.log(5.0)) < 1e-6
    for cls in range(1, C.NUM_CLASSES):
        ext.eval_metrics(logits, zeros + cls, 1.0 / n, acc)
    host = acc.cpu()
    assert int(host[0]) == n  # no other class is predicted on a tie
    assert abs(float(host.view(torch.float64)[1]) - 5 * np.log(5.0)) < 1e-5
