"""Training data resident in device memory (kernels: ops/hip/batch.hip).

The host routes of roko_amd.train feed the step through a DataLoader: one
Python `__getitem__` per window, every window widened from uint8 to int64
(144 KB instead of 18 KB), collated on the host and sent over PCIe each step.
Here the set is uploaded once, as it is stored in the file — 18,090 bytes per
window, one million windows = 18 GB of the MI355X's 288 GB — and then

  * a step's batch is one `gather_batch` launch from the epoch's permutation
    (uploaded once per epoch) into a reused (x uint8, y int64) pair,
  * validation walks the resident arrays as views and scores each batch with
    `eval_metrics`, one D2H copy of 16 bytes at the end,

so nothing crosses PCIe per step. Under torchrun every rank loads the WHOLE
set onto its own GPU and draws its own slice of the shared permutation.
"""

from __future__ import annotations

import time
from typing import Iterator, Tuple

import numpy as np

from .. import config as C
from ..rkdata import RkwFile, list_rkw_files

#: bytes of one window as stored: (200, 90) uint8 ids + 90 uint8 labels
WINDOW_BYTES = C.WINDOW_ROWS * C.WINDOW_COLS + C.WINDOW_COLS
#: size of each of the two pinned staging buffers of the upload
STAGE_BYTES = 64 << 20
#: share of the free device memory the resident sets may take
FIT_FRACTION = 0.8


def _train_files(path: str):
    files = []
    for p in list_rkw_files(path):
        f = RkwFile(p)
        if f.inference:
            raise ValueError(f"{p} is an inference file (no labels)")
        files.append(f)
    return files


def count_rkw_windows(path: str) -> int:
    """Windows in a training file or directory (footers only)."""
    return sum(f.num_windows for f in _train_files(path))


def load_rkw_arrays(path: str) -> Iterator[Tuple[np.ndarray, np.ndarray]]:
    """Yield (x uint8 (n, 200, 90), y uint8 (n, 90)) per window group of a
    training file or directory, in TrainDataset's order: files sorted, then
    groups, then offset. The arrays are views of the file's memmap — a
    group's blobs whole, no per-window Python. An inference file raises the
    ValueError TrainDataset raises, before anything is yielded."""
    files = _train_files(path)

    def groups():
        for f in files:
            for gi in range(len(f.groups)):
                _, _, ex, lab = f.group_arrays(gi)
                yield ex, lab

    return groups()


def epoch_indices(n: int, batch: int, seed: int, epoch: int, rank: int = 0,
                  world: int = 1) -> np.ndarray:
    """Window ids of one rank's epoch, int32, a whole number of batches.

    One permutation of range(n) from default_rng((seed, epoch)) is shared by
    all ranks; rank r takes perm[r::world], cut to the largest multiple of
    `batch` that EVERY rank can fill (equal step counts, drop_last). It
    depends on (seed, epoch) only, so a resumed run draws at epoch k what an
    uninterrupted one would."""
    if batch < 1 or world < 1 or not 0 <= rank < world:
        raise ValueError(f"bad batch/rank/world: {batch}/{rank}/{world}")
    if n > np.iinfo(np.int32).max:
        raise ValueError(f"{n} windows do not fit the int32 index")
    steps = (n // world) // batch  # the shortest slice has n // world windows
    if steps == 0:
        raise ValueError(
            f"{n} windows over {world} rank(s) do not fill one batch of "
            f"{batch}")
    perm = np.random.default_rng((seed, epoch)).permutation(n)
    return np.ascontiguousarray(perm[rank::world][: steps * batch],
                                dtype=np.int32)


def _upload(dst, arrays, bufs) -> None:
    """Fill the flat uint8 device tensor `dst` with the concatenation of the
    flat uint8 numpy `arrays` through the two pinned buffers `bufs`: the host
    fills one while the async copy of the other is in flight."""
    import torch

    chunk = bufs[0].numel()
    views = [b.numpy() for b in bufs]
    events = [None, None]
    k = fill = off = 0
    for a in arrays:
        p = 0
        while p < a.size:
            m = min(chunk - fill, a.size - p)
            views[k][fill:fill + m] = a[p:p + m]
            fill += m
            p += m
            if fill == chunk:
                dst[off:off + fill].copy_(bufs[k][:fill], non_blocking=True)
                events[k] = torch.cuda.Event()
                events[k].record()
                off += fill
                fill = 0
                k ^= 1
                if events[k] is not None:
                    events[k].synchronize()
    if fill:
        dst[off:off + fill].copy_(bufs[k][:fill], non_blocking=True)
        off += fill
    if off != dst.numel():
        raise RuntimeError(f"uploaded {off} of {dst.numel()} bytes")
    torch.cuda.current_stream().synchronize()


class DeviceTrainData:
    """A training file or directory as two device tensors: `x` (N, 200, 90)
    uint8 and `y` (N, 90) uint8, in TrainDataset's window order.

    `n_other` counts windows of further sets the caller will load beside
    this one (the validation set), so the fit check covers both."""

    def __init__(self, path: str, device, n_other: int = 0):
        import torch

        from . import ext

        self.ext = ext()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(
                f"DeviceTrainData needs a GPU device (got "
                f"{self.device.type!r}); use data='host'")
        t0 = time.time()
        n = count_rkw_windows(path)
        if n == 0:
            raise ValueError(f"{path} holds no windows")
        need = (n + n_other) * WINDOW_BYTES
        free, _ = torch.cuda.mem_get_info(self.device)
        if need > FIT_FRACTION * free:
            raise ValueError(
                f"{n + n_other} windows need {need / 1e9:.1f} GB of device "
                f"memory, more than {FIT_FRACTION:.0%} of the "
                f"{free / 1e9:.1f} GB free; use --data host")
        with torch.cuda.device(self.device):
            self.x = torch.empty((n, C.WINDOW_ROWS, C.WINDOW_COLS),
                                 dtype=torch.uint8, device=self.device)
            self.y = torch.empty((n, C.WINDOW_COLS), dtype=torch.uint8,
                                 device=self.device)
            bufs = [torch.empty(STAGE_BYTES, dtype=torch.uint8,
                                pin_memory=True) for _ in range(2)]
            _upload(self.x.view(-1),
                    (ex.reshape(-1) for ex, _ in load_rkw_arrays(path)), bufs)
            _upload(self.y.view(-1),
                    (lab.reshape(-1) for _, lab in load_rkw_arrays(path)),
                    bufs)
        self.nbytes = n * WINDOW_BYTES
        self.load_seconds = time.time() - t0

    def __len__(self) -> int:
        return self.x.shape[0]

    def upload_indices(self, idx: np.ndarray):
        """Check 0 <= idx < N on the host and upload: the one range check of
        an epoch — the gather kernel trusts what it is given."""
        import torch

        idx = np.ascontiguousarray(idx, dtype=np.int32)
        if idx.ndim != 1 or idx.size == 0:
            raise ValueError("idx must be a non-empty 1-D array")
        if idx.min() < 0 or idx.max() >= len(self):
            raise ValueError(
                f"window index outside [0, {len(self)}) "
                f"(min {int(idx.min())}, max {int(idx.max())})")
        return torch.from_numpy(idx).to(self.device)

    def batch(self, idx_dev, out_x, out_y) -> None:
        """out_x[b] = x[idx[b]] (uint8), out_y[b] = y[idx[b]] (int64) on the
        current stream; `idx_dev` comes from `upload_indices`."""
        self.ext.gather_batch(self.x, self.y, idx_dev, out_x, out_y)


def evaluate_device(model, data: DeviceTrainData, batch: int, rank: int = 0,
                    world: int = 1) -> Tuple[float, float]:
    """train.evaluate() over a resident set: (accuracy, mean of per-batch
    mean losses). Sequential batches are views of data.x / data.y (the last
    may be short), sharded round-robin over ranks; each is scored on the
    device by eval_metrics and the two sums come back in one D2H copy."""
    import torch
    import torch.distributed as dist

    acc = torch.zeros(2, dtype=torch.int64, device=data.device)
    total = batches = 0
    model.eval()
    with torch.no_grad():
        for i, s in enumerate(range(0, len(data), batch)):
            if world > 1 and i % world != rank:
                continue
            y = data.y[s:s + batch]
            logits = model(data.x[s:s + batch])
            data.ext.eval_metrics(logits.contiguous(), y, 1.0 / y.numel(),
                                  acc)
            total += y.numel()
            batches += 1
    model.train()
    host = acc.cpu()
    correct = int(host[0])
    loss_sum = float(host.view(torch.float64)[1])
    if world > 1 and dist.is_initialized():
        t = torch.tensor([correct, total, loss_sum, batches],
                         dtype=torch.float64, device=data.device)
        dist.all_reduce(t)
        correct, total, loss_sum, batches = t.tolist()
    if total == 0:
        return 0.0, 0.0
    return correct / total, loss_sum / max(batches, 1)
