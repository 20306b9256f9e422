"""Inference CLI: RKW windows + .pth checkpoint -> polished FASTA.

Role-equivalent to the reference's roko/inference.py:90-154, with two
deliberate re-designs for MI355X-scale throughput:

  * the per-(pos, ins) majority vote is a vectorised numpy group-by over all
    windows of a contig instead of a Python dict-of-Counters per base (the
    reference's CPU bottleneck, inference.py:119-124);
  * contig groups are sharded across ranks (one process per GPU); partial
    vote tables are gathered to rank 0, which merges (votes are associative
    counts) and stitches.

Stitch semantics match the reference (inference.py:129-147): sort voted
columns, drop leading insertion-only columns, take the draft prefix before
the first voted position, emit the majority base per column skipping GAP,
then append the draft suffix after the last voted position.
"""

from __future__ import annotations

import argparse
import time
from collections import defaultdict
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.distributed as dist
from torch.utils.data import DataLoader

from . import config as C
from .datasets import InferenceDataset
from .io.fasta import write_fasta, write_fastq
from .model import RokoModel
from .parallel.ddp import init_distributed
from .rkdata import RkwFile
from .utils.metrics import Meter, trace_range

#: vote tables: contig -> (keys int64 (K,), counts int64 (K, NUM_CLASSES))
VoteTable = Dict[str, Tuple[np.ndarray, np.ndarray]]

_KEY_SHIFT = 3  # key = pos << 3 | ins  (ins <= MAX_INS < 8)


def accumulate_votes(
    positions: np.ndarray, preds: np.ndarray
) -> Tuple[np.ndarray, np.ndarray]:
    """Group (N, W, 2) positions + (N, W) class predictions into per-column
    class counts. Returns (unique keys sorted, counts (K, NUM_CLASSES))."""
    pos = positions.reshape(-1, 2).astype(np.int64)
    keys = (pos[:, 0] << _KEY_SHIFT) | pos[:, 1]
    cls = preds.reshape(-1).astype(np.int64)
    combo = keys * C.NUM_CLASSES + cls
    uniq, cnt = np.unique(combo, return_counts=True)
    ukeys = uniq // C.NUM_CLASSES
    ucls = uniq % C.NUM_CLASSES
    out_keys, inv = np.unique(ukeys, return_inverse=True)
    counts = np.zeros((len(out_keys), C.NUM_CLASSES), dtype=np.int64)
    counts[inv, ucls] += cnt
    return out_keys, counts


class StreamingVotes:
    """Bounded-memory vote accumulation (VERDICT r1 item 7 / BASELINE
    config 5): windows are buffered per contig and folded into a per-contig
    (keys, counts) table every `chunk_windows`, so peak host memory is the
    vote table (O(contig positions)) plus one chunk — NOT all windows'
    positions+predictions (~7 GB transient for a chr1-sized contig in the
    round-1 design; the reference's per-base Python Counter loop is
    inference.py:119-124)."""

    def __init__(self, chunk_windows: int = 4096):
        self.chunk = chunk_windows
        self.tables: VoteTable = {}
        self._pos: Dict[str, List[np.ndarray]] = defaultdict(list)
        self._pred: Dict[str, List[np.ndarray]] = defaultdict(list)

    def add(self, contig: str, positions: np.ndarray, preds: np.ndarray) -> None:
        """One window: positions (W, 2), preds (W,)."""
        self._pos[contig].append(positions)
        self._pred[contig].append(preds)
        if len(self._pos[contig]) >= self.chunk:
            self._flush(contig)

    def _flush(self, contig: str) -> None:
        if not self._pos[contig]:
            return
        t = accumulate_votes(np.stack(self._pos[contig]),
                             np.stack(self._pred[contig]))
        self._pos[contig].clear()
        self._pred[contig].clear()
        prev = self.tables.get(contig)
        self.tables[contig] = t if prev is None else merge_votes([prev, t])

    def buffered(self, contig: str) -> int:
        return len(self._pos[contig])

    def finalize(self) -> VoteTable:
        for contig in list(self._pos):
            self._flush(contig)
        return self.tables


def merge_votes(tables: List[Tuple[np.ndarray, np.ndarray]]) -> Tuple[np.ndarray, np.ndarray]:
    tables = [t for t in tables if len(t[0])]
    if not tables:
        return np.empty(0, dtype=np.int64), np.empty((0, C.NUM_CLASSES), dtype=np.int64)
    all_keys = np.concatenate([t[0] for t in tables])
    out_keys, inv = np.unique(all_keys, return_inverse=True)
    counts = np.zeros((len(out_keys), C.NUM_CLASSES), dtype=np.int64)
    off = 0
    for keys, cnts in tables:
        counts[inv[off : off + len(keys)]] += cnts
        off += len(keys)
    return out_keys, counts


def stitch_contig(draft: str, keys: np.ndarray, counts: np.ndarray) -> str:
    """Majority-vote consensus spliced into the draft (reference:
    inference.py:129-147). Ties resolve to the smallest class id
    (deterministic; the reference inherits Counter insertion order)."""
    if len(keys) == 0:
        return draft
    maj = counts.argmax(axis=1)
    pos = (keys >> _KEY_SHIFT).astype(np.int64)
    ins = (keys & ((1 << _KEY_SHIFT) - 1)).astype(np.int64)
    # drop leading insertion-only columns (reference: inference.py:134)
    first = 0
    while first < len(keys) and ins[first] != 0:
        first += 1
    if first == len(keys):
        return draft
    pos, ins, maj = pos[first:], ins[first:], maj[first:]
    base_chars = np.array(list(C.LABEL_ALPHABET[: C.NUM_CLASSES]))
    keep = maj != C.LABEL_GAP
    mid = "".join(base_chars[maj[keep]])
    return draft[: pos[0]] + mid + draft[pos[-1] + 1 :]


#: dense consensus arrays (DeviceVotes.consensus / dense_majority): one byte
#: per column slot, slot = pos * SLOTS_PER_POS + ins
SLOTS_PER_POS = C.MAX_INS + 1
NO_VOTE = 0xFF


def dense_majority(keys: np.ndarray, counts: np.ndarray,
                   contig_len: int) -> np.ndarray:
    """(keys, counts) vote table -> dense uint8 majority array of
    contig_len * SLOTS_PER_POS slots: the majority class per voted slot
    (ties to the smallest class id, as in stitch_contig), NO_VOTE elsewhere.
    The CPU reference of the consensus kernel (ops/hip/votes.hip)."""
    maj = np.full(contig_len * SLOTS_PER_POS, NO_VOTE, dtype=np.uint8)
    if len(keys):
        keys = np.asarray(keys, dtype=np.int64)
        slot = (keys >> _KEY_SHIFT) * SLOTS_PER_POS \
            + (keys & ((1 << _KEY_SHIFT) - 1))
        maj[slot] = counts.argmax(axis=1).astype(np.uint8)
    return maj


_BASE_BYTES = np.frombuffer(
    C.LABEL_ALPHABET[: C.NUM_CLASSES].encode("ascii"), dtype=np.uint8)


def stitch_dense(draft: str, maj: np.ndarray) -> str:
    """stitch_contig over a dense majority array (see dense_majority): the
    voted slots in slot order are exactly the sorted vote-table keys, so the
    same four steps apply — drop leading insertion-only columns, draft
    prefix, majority base per voted column skipping GAP, draft suffix."""
    voted = np.flatnonzero(maj != NO_VOTE)
    if len(voted) == 0:
        return draft
    on_pos = np.flatnonzero(voted % SLOTS_PER_POS == 0)
    if len(on_pos) == 0:
        return draft
    voted = voted[on_pos[0]:]
    m = maj[voted]
    mid = _BASE_BYTES[m[m != C.LABEL_GAP]].tobytes().decode("ascii")
    first = int(voted[0]) // SLOTS_PER_POS
    last = int(voted[-1]) // SLOTS_PER_POS
    return draft[:first] + mid + draft[last + 1:]


def _infer_device_votes(rkw, dl, model, batch_size, depth, meter,
                        quality=False, edits=None, min_qual=0,
                        keep_uncovered=False, stitch="host"):
    """RKW windows -> DeviceVotes: predictions and vote tables stay on the
    GPU; returns ({contig: polished}, windows, {contig: quality string} or
    None). Positions are fetched per batch from the mmap in runs of one
    window group. With a dict `edits` (needs quality) every voted contig's
    edits (roko_amd/edits.py), compacted on the device, are put into it.
    `min_qual` and `keep_uncovered` (not at their defaults: needs quality)
    filter the stitch and the edits (roko_amd/stitch.py); stitch="device"
    writes the sequences on the GPU (DeviceVotes.stitch)."""
    from .ops.forward import InferencePipeline
    from .ops.votes import DeviceVotes

    lens = {c["name"]: int(c["len"]) for c in rkw.meta["contigs"]}
    # votes mode runs one batch per slot (coalesce=1)
    pipe = InferencePipeline(model, batch_size, depth=depth, coalesce=1,
                             quality=quality)
    dv = DeviceVotes(lens, pipe, quality=quality)
    group_contig = [g["contig"] for g in rkw.groups]
    n_windows = 0
    for gis, js, x in dl:
        gis, js, x = gis.numpy(), js.numpy(), x.numpy()
        # runs of one group (hence one contig, consecutive window offsets)
        cuts = np.flatnonzero(np.diff(gis)) + 1
        starts = np.concatenate([[0], cuts])
        ends = np.concatenate([cuts, [len(gis)]])
        # a slot batch votes into one contig's table: split at contig changes
        lo = 0
        while lo < len(starts):
            contig = group_contig[int(gis[starts[lo]])]
            hi = lo
            while hi < len(starts) and \
                    group_contig[int(gis[starts[hi]])] == contig:
                hi += 1
            a, b = int(starts[lo]), int(ends[hi - 1])
            xs, ps = dv.staging()
            xs[: b - a] = x[a:b]
            for r in range(lo, hi):
                _, pos_arr, _, _ = rkw.group_arrays(int(gis[starts[r]]))
                s, e = int(starts[r]), int(ends[r])
                ps[s - a : e - a] = pos_arr[int(js[s]) : int(js[e - 1]) + 1]
            dv.add_batch(contig, b - a)
            lo = hi
        n_windows += len(gis)
        meter.add(windows=len(gis), bases=len(gis) * C.WINDOW_STRIDE)
    out: Dict[str, str] = {}
    quals: Optional[Dict[str, str]] = {} if quality else None
    for name in rkw.contig_names():
        draft = rkw.contig_seq(name)
        if not dv.has_votes(name):
            out[name] = draft
            continue
        if edits is not None:
            from .stitch import applied_edits

            edits[name] = applied_edits(dv.edits(name, draft), min_qual,
                                        keep_uncovered)
        if stitch == "device":
            out[name], qual = dv.stitch(name, draft, min_qual,
                                        keep_uncovered)
            if quality:
                quals[name] = qual
            dv.free(name)
        elif quality:
            from .quality import stitch_dense_qual
            from .stitch import is_default, stitch_filtered

            if is_default(min_qual, keep_uncovered):
                out[name], quals[name] = stitch_dense_qual(
                    draft, *dv.consensus_quality(name))
            else:
                out[name], quals[name] = stitch_filtered(
                    draft, *dv.consensus_quality(name), min_qual,
                    keep_uncovered)
            dv.free(name)
        else:
            out[name] = stitch_dense(draft, dv.consensus(name))
            dv.free(name)
    return out, n_windows, quals


def _write_outputs(out: Dict[str, str], quals: Optional[Dict[str, str]],
                   out_path: Optional[str], out_fastq: Optional[str],
                   log, out_vcf: Optional[str] = None, refs=None,
                   edits=None, vcf_header=()) -> None:
    """FASTA and/or FASTQ of the polished contigs, sorted by name. A contig
    without an entry in `quals` came through as draft: all Q0. With
    `out_vcf`, the VCF of `edits` ({contig: edits.EDIT_DTYPE array}) over
    `refs` ((name, draft) pairs in the draft's order); a contig without an
    entry has no records, only its ##contig line; `vcf_header` lines
    (stitch.vcf_header) go into its header."""
    if out_path:
        write_fasta(out_path, sorted(out.items()))
        log(f"wrote {len(out)} polished contigs to {out_path}")
    if out_fastq:
        from .quality import unpolished_quality

        write_fastq(out_fastq,
                    [(name, seq, quals.get(name) or unpolished_quality(seq))
                     for name, seq in sorted(out.items())])
        log(f"wrote {len(out)} polished contigs with qualities to "
            f"{out_fastq}")
    if out_vcf:
        from .edits import contig_vcf_records, write_vcf

        n = write_vcf(out_vcf, [(name, len(seq)) for name, seq in refs],
                      contig_vcf_records(refs, edits), vcf_header)
        log(f"wrote {n} records of "
            f"{sum(len(e) for e in edits.values())} edits to {out_vcf}")


def infer(
    data_path: str,
    model_path: str,
    out_path: Optional[str],
    batch_size: int = C.BATCH_SIZE,
    workers: int = 0,
    device: Optional[torch.device] = None,
    model: Optional[RokoModel] = None,
    log=print,
    votes: Optional[str] = None,
    depth: int = 48,
    out_fastq: Optional[str] = None,
    out_vcf: Optional[str] = None,
    min_qual: int = 0,
    keep_uncovered: bool = False,
    stitch: str = "host",
) -> Dict[str, str]:
    """Polish the draft in `data_path` (RKW inference file) and return
    {contig: polished sequence}. Writes FASTA if `out_path` is given.

    Under torchrun (WORLD_SIZE > 1) the window groups are sharded across
    ranks round-robin and partial vote tables gathered to rank 0; only rank 0
    returns sequences / writes the FASTA.

    votes="device" keeps predictions and vote tables on the GPU
    (ops/votes.py); single process, GPU only. `depth` is the number of
    in-flight batches of the GPU pipeline. `votes` left at None means
    "host", except that `out_fastq` or `out_vcf` on a GPU selects "device".

    `out_fastq` also writes a FASTQ with a Phred quality per polished base
    (roko_amd/quality.py). Single process only. On a GPU the qualities are
    computed on the device and need votes="device"; on the CPU the host
    route computes them.

    `out_vcf` also writes a VCF of the edits between the draft and the
    polished sequence (roko_amd/edits.py), under the rules of `out_fastq`:
    single process; on a GPU the edits are compacted on the device from the
    vote tables and need votes="device"; on the CPU the numpy reference runs.

    `min_qual` (0..60) applies only the edits of at least that quality and
    `keep_uncovered` keeps draft bases no window covered (roko_amd/
    stitch.py). Either turns the quality tables on and falls under the rules
    of `out_fastq`; the VCF then lists only the applied edits.
    `stitch="device"` writes the polished sequences on the GPU
    (DeviceVotes.stitch): it needs a GPU and votes="device" (or votes unset).
    """
    from .stitch import check_filter, is_default, vcf_header

    if votes not in (None, "host", "device"):
        raise ValueError(f"votes must be 'host' or 'device', got {votes!r}")
    if stitch not in ("host", "device"):
        raise ValueError(f"stitch must be 'host' or 'device', got {stitch!r}")
    min_qual, keep_uncovered = check_filter(min_qual, keep_uncovered)
    filtered = not is_default(min_qual, keep_uncovered)
    rank, local_rank, world = init_distributed()
    if min_qual > 0 and world > 1:
        raise ValueError("min_qual is single-process only "
                         f"(WORLD_SIZE={world}); run one process")
    if keep_uncovered and world > 1:
        raise ValueError("keep_uncovered is single-process only "
                         f"(WORLD_SIZE={world}); run one process")
    if stitch == "device" and world > 1:
        raise ValueError("stitch='device' is single-process only "
                         f"(WORLD_SIZE={world}); use stitch='host'")
    if out_fastq and world > 1:
        raise ValueError("out_fastq is single-process only "
                         f"(WORLD_SIZE={world}); run one process")
    if out_vcf and world > 1:
        raise ValueError("out_vcf is single-process only "
                         f"(WORLD_SIZE={world}); run one process")
    if votes == "device" and world > 1:
        raise ValueError("votes='device' is single-process only "
                         f"(WORLD_SIZE={world}); use votes='host'")
    if device is None:
        device = (
            torch.device("cuda", local_rank)
            if torch.cuda.is_available()
            else torch.device("cpu")
        )
    device = torch.device(device)
    if stitch == "device":
        if device.type != "cuda":
            raise ValueError(
                "stitch='device' writes the polished sequence on the GPU "
                f"and needs a GPU device (got {device.type!r}); use "
                "stitch='host'")
        if votes == "host":
            raise ValueError("stitch='device' reads the device vote tables "
                             "and needs votes='device' (or leave votes "
                             "unset)")
        votes = "device"
    if (out_fastq or out_vcf or filtered) and device.type == "cuda":
        if votes == "host":
            what = ("out_fastq" if out_fastq else "out_vcf" if out_vcf
                    else "min_qual" if min_qual > 0 else "keep_uncovered")
            raise ValueError(
                f"{what} on a GPU "
                "computes the qualities on the device "
                "and needs votes='device' (or leave votes unset)")
        votes = "device"
    if votes is None:
        votes = "host"
    # the edits carry qualities, so a VCF turns the quality tables on; so
    # does a filter not at its defaults, which is decided per slot from them
    quality = bool(out_fastq or out_vcf or filtered)
    edits: Optional[Dict[str, np.ndarray]] = {} if out_vcf else None

    if model is None:
        model = RokoModel()
        model.load_reference_checkpoint(model_path)
    if votes == "device" and device.type != "cuda":
        raise RuntimeError("votes='device' needs a ROCm GPU (the vote tables "
                           "live in device memory); use votes='host'")
    model = model.to(device).eval()

    rkw = RkwFile(data_path)
    my_groups = [gi for gi in range(len(rkw.groups)) if gi % world == rank]
    ds = InferenceDataset(data_path, groups=my_groups)
    dl = DataLoader(ds, batch_size=batch_size, num_workers=workers,
                    pin_memory=torch.cuda.is_available())

    # streaming per-contig vote accumulation (bounded memory)
    if quality:
        from .quality import StreamingQualityVotes, phred_units, stitch_tables
        from .stitch import applied_edits, stitch_tables_filtered

        sv = StreamingQualityVotes()
    else:
        sv = StreamingVotes()

    def account(gis, js, preds, units=None):
        for k in range(len(gis)):
            g, pos_arr, _, _ = rkw.group_arrays(int(gis[k]))
            if units is None:
                sv.add(g["contig"], np.asarray(pos_arr[js[k]]), preds[k])
            else:
                sv.add(g["contig"], np.asarray(pos_arr[js[k]]), preds[k],
                       units[k])

    t0 = time.time()
    n_windows = 0
    meter = Meter("inference", rank=rank)
    pipe = None
    out: Optional[Dict[str, str]] = None
    quals: Optional[Dict[str, str]] = None
    if device.type == "cuda" and votes == "host":
        from .ops.forward import InferencePipeline

        pipe = InferencePipeline(model, batch_size, depth=depth)
    with torch.no_grad():
        if votes == "device":
            out, n_windows, quals = _infer_device_votes(
                rkw, dl, model, batch_size, depth, meter, quality, edits,
                min_qual, keep_uncovered, stitch)
        elif pipe is not None:
            # pipelined: keep `depth` batches in flight; votes are harvested
            # one pipeline-depth behind submission
            pending: List[tuple] = []
            for gis, js, x in dl:
                if len(pending) >= pipe.depth:
                    tk, pgis, pjs = pending.pop(0)
                    account(pgis, pjs, tk().numpy())
                with trace_range("submit"):
                    ticket = pipe.submit(x, copy_out=True)
                pending.append((ticket, gis.numpy(), js.numpy()))
                n_windows += len(gis)
                meter.add(windows=len(gis), bases=len(gis) * C.WINDOW_STRIDE)
            for tk, pgis, pjs in pending:
                account(pgis, pjs, tk().numpy())
        else:
            for gis, js, x in dl:
                x = x.to(device, non_blocking=True)
                logits = model(x.long())
                preds = logits.argmax(dim=2).to(torch.uint8).cpu().numpy()
                n_windows += len(gis)
                meter.add(windows=len(gis), bases=len(gis) * C.WINDOW_STRIDE)
                account(gis.numpy(), js.numpy(), preds,
                        phred_units(logits.cpu().numpy()) if quality
                        else None)
    meter.close()
    dt = time.time() - t0
    bases = n_windows * C.WINDOW_STRIDE
    log(
        f"rank {rank}: {n_windows} windows in {dt:.1f}s "
        f"({bases / max(dt, 1e-9):.0f} bases/s)"
    )

    refs = [(name, rkw.contig_seq(name)) for name in rkw.contig_names()] \
        if out_vcf else None
    if out is not None:
        _write_outputs(out, quals, out_path, out_fastq, log, out_vcf, refs,
                       edits, vcf_header(min_qual, keep_uncovered))
        return out

    if quality:
        tables, sums = sv.finalize()
    else:
        tables: VoteTable = sv.finalize()

    if world > 1:
        gathered: List[Optional[VoteTable]] = [None] * world if rank == 0 else None
        dist.gather_object(tables, gathered, dst=0)
        if rank != 0:
            return {}
        merged: VoteTable = {}
        names = set()
        for t in gathered:
            names.update(t.keys())
        for name in names:
            merged[name] = merge_votes([t[name] for t in gathered if name in t])
        tables = merged

    out = {}
    quals = {}
    for name in rkw.contig_names():
        draft = rkw.contig_seq(name)
        if name in tables and filtered:
            out[name], quals[name] = stitch_tables_filtered(
                draft, tables[name], sums[name], min_qual, keep_uncovered)
        elif name in tables:
            out[name] = stitch_contig(draft, *tables[name])
            if quality:
                seq, quals[name] = stitch_tables(draft, tables[name],
                                                 sums[name])
                if seq != out[name]:
                    raise RuntimeError(
                        f"{name}: the quality stitch disagrees with the "
                        "sequence stitch")
        else:
            out[name] = draft
        if name in tables and edits is not None:
            from .edits import table_edits

            edits[name] = applied_edits(
                table_edits(draft, tables[name], sums[name]), min_qual,
                keep_uncovered)
    _write_outputs(out, quals, out_path, out_fastq, log, out_vcf, refs, edits,
                   vcf_header(min_qual, keep_uncovered))
    return out


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("data", help="inference .rkw file")
    p.add_argument("model", help=".pth checkpoint (reference format)")
    p.add_argument("out", help="output FASTA path")
    p.add_argument("--t", type=int, default=0, help="DataLoader workers")
    p.add_argument("--b", type=int, default=C.BATCH_SIZE, help="batch size")
    p.add_argument("--fastq", default=None, metavar="PATH",
                   help="also write FASTQ with a Phred quality per polished "
                        "base (single process; on a GPU the votes run on "
                        "the device)")
    p.add_argument("--vcf", default=None, metavar="PATH",
                   help="also write VCF: the edits between the draft and "
                        "the polished sequence (single process; on a GPU "
                        "the votes run on the device)")
    p.add_argument("--min-qual", type=int, default=0, metavar="Q",
                   help="apply only edits of quality Q or more (0..60); a "
                        "rejected edit leaves the draft as it was, at Q0 "
                        "(single process; on a GPU the votes run on the "
                        "device)")
    p.add_argument("--keep-uncovered", action="store_true",
                   help="keep draft bases inside the polished span that no "
                        "window covered (Q0) instead of dropping them "
                        "(single process)")
    p.add_argument("--stitch", choices=("host", "device"), default="host",
                   help="where the polished sequence is put together: numpy "
                        "over the fetched consensus (host) or the GPU, from "
                        "the device vote tables (device)")
    a = p.parse_args(argv)
    infer(a.data, a.model, a.out, batch_size=a.b, workers=a.t,
          out_fastq=a.fastq, out_vcf=a.vcf, min_qual=a.min_qual,
          keep_uncovered=a.keep_uncovered, stitch=a.stitch)


if __name__ == "__main__":
    main()
