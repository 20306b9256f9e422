"""Feature windows built on the GPU from packed reads (kernels:
ops/hip/windows.hip).

`_pileup.region_reads` gives a region's filtered reads as BAM stores them —
4-bit bases, CIGAR words, bounds, strand; `build_windows` uploads them (a few
MB per 100 kb region, against ~60 MB of windows) and returns the window
tensor and its positions in device memory, ready for the serving slots'
votes mode. Rows are sampled with the counter sampler (ops/cpp/pileup.h);
`generate_features(..., sampler="counter")` gives the same bytes.
"""

from __future__ import annotations

from typing import Tuple

import numpy as np
import torch

from .. import config as C

#: the geometry windows.hip is compiled for
GEOMETRY = (C.WINDOW_ROWS, C.WINDOW_COLS, C.WINDOW_STRIDE, C.MAX_INS)

_CIGAR_INS = 1
_FIELDS = (("ref_start", np.int32), ("ref_end", np.int32),
           ("reverse", np.uint8), ("cigar_off", np.uint32),
           ("seq_off", np.uint32), ("cigar", np.uint32), ("seq4", np.uint8))


def check_geometry(cfg) -> None:
    got = (cfg.window_rows, cfg.window_cols, cfg.window_stride, cfg.max_ins)
    if got != GEOMETRY:
        raise ValueError(
            "the device window builder is compiled for (rows, cols, stride, "
            f"max_ins) = {GEOMETRY}, got {got}; use the host extractor")


def _checked(pack: dict) -> dict:
    """The pack's arrays, contiguous and of the right type, after the checks
    the kernels rely on: offsets ascending, inside their arrays, below 2^31."""
    a = {}
    for name, dt in _FIELDS:
        v = np.ascontiguousarray(pack[name])
        if v.dtype != dt or v.ndim != 1:
            raise ValueError(f"pack[{name!r}] must be a 1-d {np.dtype(dt)} array")
        a[name] = v
    n = len(a["ref_start"])
    if len(a["ref_end"]) != n or len(a["reverse"]) != n:
        raise ValueError("pack: per-read arrays disagree on the read count")
    for off, flat in (("cigar_off", "cigar"), ("seq_off", "seq4")):
        o = a[off].astype(np.int64)
        if len(o) != n + 1 or o[0] != 0 or o[-1] != len(a[flat]) \
                or (np.diff(o) < 0).any() or len(a[flat]) >= 1 << 31:
            raise ValueError(f"pack[{off!r}] does not index pack[{flat!r}]")
    if n and (np.diff(a["cigar_off"].astype(np.int64)) == 0).any():
        raise ValueError("pack: a read without CIGAR ops")
    if (a["ref_end"] < a["ref_start"]).any():
        raise ValueError("pack: ref_end before ref_start")
    return a


def build_windows(pack: dict, cfg, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """Packed reads of one region -> (x (n, 200, 90) uint8, pos (n, 90, 2)
    int32) on `device`, built on the current stream. Only non-empty windows
    are returned, in order."""
    from . import ext

    check_geometry(cfg)
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError("build_windows needs a GPU device, got "
                         f"{device.type!r}")
    a = _checked(pack)
    start, end = int(pack["start"]), int(pack["end"])
    span = max(end - start, 0)
    # a position has insertion columns only if some read has an I op there
    n_ins = int(np.count_nonzero((a["cigar"] & 0xF) == _CIGAR_INS))
    ncols_max = span + cfg.max_ins * min(span, n_ins)
    dev = {k: torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v)
           .to(device) for k, v in a.items()}
    with torch.cuda.device(device):
        x, pos = ext().build_windows(
            dev["ref_start"], dev["ref_end"], dev["reverse"],
            dev["cigar_off"], dev["seq_off"], dev["cigar"], dev["seq4"],
            start, end, int(pack["region_key"]), ncols_max, *GEOMETRY)
    return x, pos
