"""Device-resident majority vote (kernels: ops/hip/votes.hip).

The host vote path brings every prediction over PCIe and folds it into
(keys, counts) tables with numpy group-bys. Here the predictions never leave
the GPU: each serving slot adds its batch's votes into a dense per-contig
table in device memory, and only the per-slot majority — one byte — is
copied back, once per contig.

Table layout: one 32-bit word per column slot, slot = pos * (MAX_INS + 1) +
ins, five 4-bit class counters per word (16 B per draft base). The window
extractor gives a column at most 6 votes (docs/KERNELS.md), so 4 bits hold
it; a counter that would pass 15 sets an error flag and `counts()` /
`consensus()` raise instead of returning a corrupted table.

Quality (`quality=True`, roko_amd/quality.py): a second table `qsum` beside
each count table, one 64-bit word per slot (8 B per slot, 32 B per draft
base), class k in the 12-bit field at bits [12k, 12k+12) holding the sum of
that class's quarter-Phred units over the slot's votes. 16 votes x 255 = 4080
< 4096, so whatever the count table holds fits; a field that would pass 4095
sets the same overflow flag.

Edits (`edits()`, kernels: ops/hip/edits.hip, contract: roko_amd/edits.py):
from both tables and the draft, the slots at which the polished sequence
differs from the draft, compacted on the device in slot order; only they are
copied back.

Stitch (`stitch()`, kernels: ops/hip/stitch.hip, contract: roko_amd/
stitch.py): the polished sequence and its quality string written on the
device from the same tables and the draft, with edits below `min_qual`
rejected and uncovered draft bases kept on request; one byte per polished
base (two with quality) comes back instead of two per column slot.
"""

from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

from .. import config as C

SLOTS_PER_POS = C.MAX_INS + 1
_KEY_SHIFT = 3  # VoteTable key = pos << 3 | ins (inference.py)
_NIBBLE = 4
_QFIELD = 12  # bits per class in a qsum word
_ERR_RANGE = 1
_ERR_OVERFLOW = 2
_I64_MAX = (1 << 63) - 1
# device edit record (ops/hip/edits.hip): the fields of edits.EDIT_DTYPE in 16
# bytes
_EDIT_RECORD = np.dtype({"names": ["pos", "ins", "ref", "alt", "qual"],
                         "formats": ["<i8", "u1", "u1", "u1", "u1"],
                         "offsets": [0, 8, 9, 10, 11], "itemsize": 16})


class VoteOverflowError(RuntimeError):
    """A column received more votes for one class than a 4-bit counter
    holds, or more quality units than a 12-bit field holds; the device
    tables are not usable."""


class DeviceVotes:
    """Per-contig vote tables in device memory.

    `contig_lens` maps contig name -> draft length. Tables are allocated
    zeroed on a contig's first batch and released by `free()`. With a
    `pipe` (ops.forward.InferencePipeline built with coalesce=1) batches go
    through its serving slots in votes mode: fill `staging()`, then
    `add_batch(contig, n)`.
    `scatter()` adds given predictions directly (tests, merging).
    With `quality=True` (and a pipe built with quality=True) every vote
    also adds its quality units into the contig's `qsum` table.
    """

    def __init__(self, contig_lens: Dict[str, int], pipe=None,
                 device: Optional[torch.device] = None,
                 quality: bool = False):
        from . import ext

        self.ext = ext()
        self.lens = dict(contig_lens)
        self.pipe = pipe
        self.quality = bool(quality)
        if self.quality and pipe is not None and \
                not getattr(pipe, "quality", False):
            raise ValueError("quality votes need a pipeline built with "
                             "quality=True")
        if device is None:
            device = (next(pipe.model.parameters()).device if pipe is not None
                      else torch.device("cuda", torch.cuda.current_device()))
        self.device = device
        self.tables: Dict[str, torch.Tensor] = {}
        self.qsums: Dict[str, torch.Tensor] = {}
        self.err_flag = torch.zeros(1, dtype=torch.int32, device=device)
        self._stage = None

    # -- tables --------------------------------------------------------------
    def n_slots(self, contig: str) -> int:
        return self.lens[contig] * SLOTS_PER_POS

    def table(self, contig: str) -> torch.Tensor:
        t = self.tables.get(contig)
        if t is None:
            t = torch.zeros(self.n_slots(contig), dtype=torch.int32,
                            device=self.device)
            self.tables[contig] = t
            if self.quality:
                self.qsums[contig] = torch.zeros(
                    self.n_slots(contig), dtype=torch.int64,
                    device=self.device)
        return t

    def qsum(self, contig: str) -> Optional[torch.Tensor]:
        """The contig's quality table (allocated with its count table), or
        None without quality."""
        if not self.quality:
            return None
        self.table(contig)
        return self.qsums[contig]

    def has_votes(self, contig: str) -> bool:
        return contig in self.tables

    def free(self, contig: str) -> None:
        self.drain()
        self.tables.pop(contig, None)
        self.qsums.pop(contig, None)

    def _validate(self, contig: str, positions: np.ndarray) -> None:
        """Host-side range check before anything is uploaded; the kernel's
        own guard is only the second line of defence."""
        if positions.size == 0:
            return
        p, i = positions[..., 0], positions[..., 1]
        if p.min() < 0 or p.max() >= self.lens[contig]:
            raise ValueError(
                f"{contig}: window position outside [0, {self.lens[contig]})"
                f" (min {int(p.min())}, max {int(p.max())})")
        if i.min() < 0 or i.max() > C.MAX_INS:
            raise ValueError(
                f"{contig}: insertion slot outside [0, {C.MAX_INS}]"
                f" (min {int(i.min())}, max {int(i.max())})")

    # -- adding votes --------------------------------------------------------
    def staging(self) -> Tuple[np.ndarray, np.ndarray]:
        """Pinned (x, pos) staging of the next slot, safe to overwrite."""
        self._stage = self.pipe.votes_staging()
        return self._stage

    def add_batch(self, contig: str, n: int) -> None:
        """Submit rows 0..n of the staging last returned by `staging()`."""
        if self._stage is None:
            raise RuntimeError("fill staging() before add_batch()")
        self._validate(contig, self._stage[1][:n])
        self._stage = None
        self.pipe.submit_votes(n, self.table(contig), self.n_slots(contig),
                               self.err_flag, self.qsum(contig))

    def add_device_batch(self, contig: str, x: torch.Tensor,
                         pos: torch.Tensor, n: int) -> None:
        """Submit rows 0..n of device tensors x (>=n, R, W) u8 and pos (>=n,
        W, 2) i32 (ops/windows.py), n <= the pipeline's batch. Nothing
        crosses PCIe, so there is no host range check here: the vote kernel
        drops and flags an out-of-range position, and `_check()` raises on
        that flag before any table is read."""
        self.pipe.submit_votes_device(x, pos, n, self.table(contig),
                                      self.n_slots(contig), self.err_flag,
                                      self.qsum(contig))

    def scatter(self, contig: str, preds, positions, units=None) -> None:
        """Add given predictions (N, W) u8 at positions (N, W, 2) i32 on the
        current stream. Rows with pos < 0 do not vote. With quality, `units`
        (N, W, 5) u8 are the votes' quality units."""
        positions = np.ascontiguousarray(positions, dtype=np.int32)
        preds = np.ascontiguousarray(preds, dtype=np.uint8)
        live = positions[positions[..., 0] >= 0]
        self._validate(contig, live)
        if preds.size and preds.max() >= C.NUM_CLASSES:
            raise ValueError("prediction class outside [0, NUM_CLASSES)")
        if self.quality != (units is not None):
            raise ValueError("units are given exactly when the tables were "
                             "built with quality=True")
        if units is not None:
            units = np.ascontiguousarray(units, dtype=np.uint8)
            if units.shape != preds.shape + (C.NUM_CLASSES,):
                raise ValueError("units must be preds.shape + (NUM_CLASSES,)")
            self.ext.vote_scatter_q(
                torch.from_numpy(preds).to(self.device),
                torch.from_numpy(units).to(self.device),
                torch.from_numpy(positions).to(self.device),
                self.table(contig), self.qsum(contig), self.n_slots(contig),
                self.err_flag)
            return
        self.ext.vote_scatter(
            torch.from_numpy(preds).to(self.device),
            torch.from_numpy(positions).to(self.device),
            self.table(contig), self.n_slots(contig), self.err_flag)

    # -- reading -------------------------------------------------------------
    def drain(self) -> None:
        if self.pipe is not None:
            self.pipe.drain()

    def _check(self) -> None:
        self.drain()
        flag = int(self.err_flag.item())
        if flag & _ERR_OVERFLOW:
            raise VoteOverflowError(
                "device vote table overflow: a column received more than 15 "
                "votes for one class (4-bit counters)"
                + (" or more quality units than a 12-bit field holds"
                   if self.quality else "")
                + "; rerun with host votes (votes='host')")
        if flag & _ERR_RANGE:
            raise RuntimeError(
                "device vote kernel dropped an out-of-range position or "
                "class; the table is incomplete — rerun with host votes")

    def counts(self, contig: str) -> Tuple[np.ndarray, np.ndarray]:
        """Unpack a table to the host VoteTable form: (keys int64 sorted,
        counts int64 (K, NUM_CLASSES)), key = pos << 3 | ins."""
        self._check()
        tab = self.table(contig).cpu().numpy().view(np.uint32)
        slots = np.flatnonzero(tab)
        keys = ((slots // SLOTS_PER_POS) << _KEY_SHIFT) | (slots % SLOTS_PER_POS)
        shifts = np.arange(C.NUM_CLASSES, dtype=np.uint32) * _NIBBLE
        counts = (tab[slots, None] >> shifts[None, :]) & 15
        return keys.astype(np.int64), counts.astype(np.int64)

    def consensus(self, contig: str) -> np.ndarray:
        """Majority class per slot (uint8, 0xFF = no votes), ties to the
        smallest class id: one kernel and one D2H of a byte per slot."""
        self._check()
        n = self.n_slots(contig)
        maj = torch.empty(n, dtype=torch.uint8, device=self.device)
        self.ext.vote_consensus(self.table(contig), n, maj)
        return maj.cpu().numpy()

    def _need_quality(self) -> None:
        if not self.quality:
            raise RuntimeError("these tables were built without quality "
                               "(DeviceVotes(..., quality=True))")

    def sums(self, contig: str) -> Tuple[np.ndarray, np.ndarray]:
        """Unpack the quality table to the host form of
        quality.accumulate_quality: (keys int64 sorted, sums int64 (K,
        NUM_CLASSES)) over the voted slots, the keys of `counts()`."""
        self._need_quality()
        self._check()
        tab = self.table(contig).cpu().numpy().view(np.uint32)
        q = self.qsum(contig).cpu().numpy().view(np.uint64)
        slots = np.flatnonzero(tab)
        keys = ((slots // SLOTS_PER_POS) << _KEY_SHIFT) | (slots % SLOTS_PER_POS)
        shifts = np.arange(C.NUM_CLASSES, dtype=np.uint64) * np.uint64(_QFIELD)
        sums = (q[slots, None] >> shifts[None, :]) \
            & np.uint64((1 << _QFIELD) - 1)
        return keys.astype(np.int64), sums.astype(np.int64)

    def consensus_quality(self, contig: str) -> Tuple[np.ndarray, np.ndarray]:
        """(maj, qual) per slot, both uint8: `consensus()` and the Phred of
        the majority class (quality.NO_QUAL = 0xFF where no votes). One
        kernel and two bytes per slot of D2H."""
        self._need_quality()
        self._check()
        n = self.n_slots(contig)
        maj = torch.empty(n, dtype=torch.uint8, device=self.device)
        qual = torch.empty(n, dtype=torch.uint8, device=self.device)
        self.ext.vote_consensus_q(self.table(contig), self.qsum(contig), n,
                                  maj, qual)
        return maj.cpu().numpy(), qual.cpu().numpy()

    def edits(self, contig: str, draft: str) -> np.ndarray:
        """What polishing changes in `draft`: edits.dense_edits(draft,
        *consensus_quality(contig)) computed on the device (ops/hip/
        edits.hip), in slot order, as an array of edits.EDIT_DTYPE. The draft
        goes up once (a byte per base); what comes back is three words and
        then 16 bytes per edit, never the dense arrays."""
        from ..edits import EDIT_DTYPE

        self._need_quality()
        self._check()
        n_pos = self.lens[contig]
        if len(draft) != n_pos:
            raise ValueError(f"{contig}: draft of {len(draft)} bases for "
                             f"tables of {n_pos}")
        if n_pos == 0 or not self.has_votes(contig):
            return np.empty(0, dtype=EDIT_DTYPE)
        n = self.n_slots(contig)
        table, qsum = self.table(contig), self.qsum(contig)
        d = torch.from_numpy(
            np.frombuffer(bytearray(draft, "ascii"), dtype=np.uint8)
        ).to(self.device)
        # {first voted ins == 0 slot, last voted slot, number of edits}
        state = torch.tensor([_I64_MAX, -1, 0], dtype=torch.int64) \
            .to(self.device)
        offsets = torch.empty(self.ext.edit_num_blocks(n_pos),
                              dtype=torch.int64, device=self.device)
        self.ext.edit_count(table, d, n, state, offsets)
        total = int(state.cpu()[2])
        if total == 0:
            return np.empty(0, dtype=EDIT_DTYPE)
        records = torch.empty(2 * total, dtype=torch.int64,
                              device=self.device)
        self.ext.edit_write(table, qsum, d, n, state, offsets, records, total)
        rec = records.cpu().numpy().view(_EDIT_RECORD)
        out = np.empty(total, dtype=EDIT_DTYPE)
        for name in EDIT_DTYPE.names:
            out[name] = rec[name]
        return out

    def stitch(self, contig: str, draft: str, min_qual: int = 0,
               keep_uncovered: bool = False) -> Tuple[str, Optional[str]]:
        """The polished contig under the quality filter:
        stitch.stitch_filtered(draft, *consensus_quality(contig), min_qual,
        keep_uncovered) computed on the device (ops/hip/stitch.hip). Returns
        (sequence, Phred+33 quality string); on tables built without quality
        the quality string is None and `min_qual` must be 0. The draft goes
        up once (a byte per base); what comes back is three words and then
        one byte per polished base, and a second one with quality."""
        from ..quality import unpolished_quality
        from ..stitch import check_filter

        min_qual, keep_uncovered = check_filter(min_qual, keep_uncovered)
        self._check()
        if min_qual > 0:
            self._need_quality()
        n_pos = self.lens[contig]
        if len(draft) != n_pos:
            raise ValueError(f"{contig}: draft of {len(draft)} bases for "
                             f"tables of {n_pos}")
        as_draft = (draft, unpolished_quality(draft) if self.quality
                    else None)
        if n_pos == 0 or not self.has_votes(contig):
            return as_draft
        n = self.n_slots(contig)
        table, qsum = self.table(contig), self.qsum(contig)
        d = torch.from_numpy(
            np.frombuffer(bytearray(draft, "ascii"), dtype=np.uint8)
        ).to(self.device)
        # {first voted ins == 0 slot, last voted slot, polished length}
        state = torch.tensor([_I64_MAX, -1, 0], dtype=torch.int64) \
            .to(self.device)
        offsets = torch.empty(self.ext.edit_num_blocks(n_pos),
                              dtype=torch.int64, device=self.device)
        self.ext.stitch_count(table, qsum, d, n, state, offsets, min_qual,
                              keep_uncovered)
        s0, _, total = (int(v) for v in state.cpu())
        if s0 == _I64_MAX:  # no voted ins == 0 slot: nothing is stitched
            return as_draft
        seq = torch.empty(total, dtype=torch.uint8, device=self.device)
        qual = torch.empty(total, dtype=torch.uint8, device=self.device) \
            if self.quality else None
        self.ext.stitch_write(table, qsum, d, n, state, offsets, min_qual,
                              keep_uncovered, seq, qual, total)
        return (seq.cpu().numpy().tobytes().decode("ascii"),
                None if qual is None
                else qual.cpu().numpy().tobytes().decode("ascii"))
