"""Feature-generation CLI: draft FASTA + reads BAM -> RKW window files.

Role-equivalent to the reference's roko/features.py:113-157: split every
contig into overlapping regions, fan regions out over worker processes, run
the C++ window builder per region, and (for training) join windows with
truth labels before writing.

Usage:
  python -m roko_amd.features <draft.fasta> <reads.bam> <out.rkw>
      [--Y truth.bam] [--t workers] [--seed N] [--sampler mt19937|counter]
      [--extract host|device]

With --extract device the workers only inflate, filter and pack the reads
(generate_reads); this process builds the windows on the GPU from those
(ops/windows.py) and, with --Y, labels them there too (ops/labels_device.py).
That route samples rows with the counter sampler whatever --sampler says;
`--extract host --sampler counter` writes the same file.
"""

from __future__ import annotations

import argparse
import dataclasses
import multiprocessing
import time
from multiprocessing import Pool
from typing import Iterator, Optional, Tuple

import numpy as np

from . import config as C
from .config import FeatureConfig
from .io.fasta import read_fasta
from .rkdata import RkwWriter


def generate_regions(
    ref_len: int, size: int = C.REGION_SIZE, overlap: int = C.REGION_OVERLAP
) -> Iterator[Tuple[int, int]]:
    """(start, end) spans of `size` with `overlap` between neighbours
    (reference: features.py:16-27)."""
    i = 0
    while i < ref_len:
        end = min(i + size, ref_len)
        yield i, end
        if i + size >= ref_len:
            break
        i = i + size - overlap


def _features_for_region(bam, contig, start, end, cfg: FeatureConfig):
    from .ops import _pileup

    return _pileup.generate_features(
        bam,
        contig,
        start,
        end,
        rows=cfg.window_rows,
        cols=cfg.window_cols,
        stride=cfg.window_stride,
        max_ins=cfg.max_ins,
        filter_flag=cfg.filter_flag,
        min_mapq=cfg.min_mapq,
        seed=cfg.seed,
        sampler=cfg.sampler,
    )


def _reads_for_region(bam, contig, start, end, cfg: FeatureConfig):
    from .ops import _pileup

    return _pileup.region_reads(
        bam,
        contig,
        start,
        end,
        filter_flag=cfg.filter_flag,
        min_mapq=cfg.min_mapq,
        seed=cfg.seed,
    )


def generate_reads(args):
    """Worker of the device extraction route: the region's filtered reads,
    still packed as BAM stores them (ops/windows.py builds the windows from
    them on the GPU). Failures are returned, not raised, as in
    generate_infer."""
    bam_x, contig, start, end, cfg = args
    try:
        pack = _reads_for_region(bam_x, contig, start, end, cfg)
    except Exception as e:  # noqa: BLE001 — deliberate region-level fence
        return ("__error__", f"{contig}:{start}-{end}", repr(e))
    return contig, start, end, pack


def generate_infer(args):
    """Inference worker: windows only (reference: features.py:97-110).
    Failures are returned, not raised: one bad region must not kill the
    whole run (the reference dies on any worker exception).
    """
    bam_x, contig, start, end, cfg = args
    try:
        positions, examples = _features_for_region(bam_x, contig, start, end, cfg)
    except Exception as e:  # noqa: BLE001 — deliberate region-level fence
        return ("__error__", f"{contig}:{start}-{end}", repr(e))
    return contig, start, end, positions, examples, None


def generate_train(args):
    """Training worker: windows joined with truth labels
    (reference: features.py:37-94). Failures are returned, not raised."""
    try:
        return _generate_train(args)
    except Exception as e:  # noqa: BLE001 — deliberate region-level fence
        _, _, contig, start, end, _ = args
        return ("__error__", f"{contig}:{start}-{end}", repr(e))


def _generate_train(args):
    bam_x, bam_y, contig, start, end, cfg = args
    from .labels import filter_aligns, get_aligns, get_pos_and_labels

    aligns = get_aligns(bam_y, contig, start, end)
    filtered = filter_aligns(aligns)
    if not filtered:
        return None

    def in_region(pos: int) -> bool:
        return any(a.start <= pos < a.end for a in filtered)

    out_pos, out_x, out_y = [], [], []
    for a in filtered:
        t_pos, t_labels = get_pos_and_labels(a, start, end)
        pos_labels = {}
        n_pos = set()
        for p, l in zip(t_pos, t_labels):
            if l == C.LABEL_UNKNOWN:
                n_pos.add(p)
            else:
                pos_labels[p] = l
        if not pos_labels:
            continue
        pos_sorted = sorted(pos_labels)
        # feature columns strictly inside the labeled span (reference:
        # features.py:62-63 builds "{first+1}-{last}" which htslib reads as
        # the 0-based half-open [first, last))
        sub_start, sub_end = pos_sorted[0][0], pos_sorted[-1][0]
        if sub_end <= sub_start:
            continue
        positions, examples = _features_for_region(bam_x, contig, sub_start, sub_end, cfg)

        for w in range(positions.shape[0]):
            P = positions[w]
            keep = True
            Y = np.empty(cfg.window_cols, dtype=np.uint8)
            for s in range(cfg.window_cols):
                p = (int(P[s, 0]), int(P[s, 1]))
                assert in_region(p[0]), f"window position {p} outside filtered truth aligns"
                if p in n_pos:
                    keep = False
                    break
                try:
                    Y[s] = pos_labels[p]
                except KeyError:
                    if p[1] != 0:
                        Y[s] = C.LABEL_GAP  # un-labeled insertion slot
                    else:
                        raise KeyError(f"no label for draft position {p}") from None
            if keep:
                out_pos.append(P)
                out_x.append(examples[w])
                out_y.append(Y)

    if not out_pos:
        return None
    return (
        contig,
        start,
        end,
        np.stack(out_pos),
        np.stack(out_x),
        np.stack(out_y),
    )


def run(
    ref_path: str,
    bam_x: str,
    out_path: str,
    bam_y: Optional[str] = None,
    workers: int = 1,
    cfg: Optional[FeatureConfig] = None,
    log=print,
    extract: str = "host",
    device=None,
) -> int:
    """Write the RKW file of `ref_path` + `bam_x` (+ truth `bam_y` for
    training); returns the window count. `extract="device"` builds windows
    and labels on the GPU `device` (counter sampler, whatever `cfg.sampler`
    says) and writes what `extract="host"` writes with sampler="counter"."""
    cfg = cfg or FeatureConfig()
    if extract not in ("host", "device"):
        raise ValueError(f"extract must be 'host' or 'device', got {extract!r}")
    if extract == "device":
        return _run_device(ref_path, bam_x, out_path, bam_y, workers, cfg,
                           log, device)
    inference = bam_y is None
    refs = list(read_fasta(ref_path))

    jobs = []
    for name, seq in refs:
        for start, end in generate_regions(len(seq), cfg.region_size, cfg.region_overlap):
            if inference:
                jobs.append((bam_x, name, start, end, cfg))
            else:
                jobs.append((bam_x, bam_y, name, start, end, cfg))
    func = generate_infer if inference else generate_train
    log(f"feature generation: {len(jobs)} region jobs, {workers} workers")

    n_windows = 0
    t0 = time.time()
    with RkwWriter(out_path, inference=inference) as writer:
        writer.write_contigs(refs)

        n_errors = 0

        def consume(result, job):
            nonlocal n_windows, n_errors
            if result is None:
                return
            if result[0] == "__error__":
                # one in-parent retry before giving the region up: transient
                # faults (an fs hiccup, a worker killed mid-region) should
                # not cost coverage (SURVEY.md §5.3 — the reference dies on
                # the first worker exception and has no retry at all)
                log(f"WARNING: region {result[1]} failed: {result[2]} "
                    "(retrying once)")
                result = func(job)
                if result is None:
                    return
                if result[0] == "__error__":
                    n_errors += 1
                    log(f"WARNING: region {result[1]} failed twice: "
                        f"{result[2]} (skipped)")
                    return
            contig, start, end, positions, examples, labs = result
            writer.store(contig, start, end, positions, examples, labs)
            n_windows += len(positions)

        if workers <= 1:
            for job in jobs:
                consume(func(job), job)
        else:
            with Pool(processes=workers) as pool:
                for result, job in zip(pool.imap(func, jobs), jobs):
                    consume(result, job)
    dt = time.time() - t0
    log(f"wrote {n_windows} windows to {out_path} in {dt:.1f}s "
        f"({n_windows / max(dt, 1e-9):.0f} windows/s)"
        + (f"; {n_errors} regions FAILED and were skipped" if n_errors else ""))
    return n_windows


# ---------------------------------------------------------------------------
# extract="device": windows and labels built on the GPU

def device_job(job):
    """Worker of the device route. ("reads", args): the packed reads of a
    span (generate_reads); ("host", args): a region the device does not take,
    built by the host functions."""
    kind, args = job
    if kind == "reads":
        return generate_reads(args)
    return generate_train(args) if len(args) == 6 else generate_infer(args)


def _device_type(device) -> str:
    """Type of the device the device route would run on, without creating
    it."""
    import torch

    if device is None:
        return "cuda" if torch.cuda.is_available() else "cpu"
    return torch.device(device).type


def _plan_device(refs, bam_x, bam_y, cfg, host_cfg):
    """Regions of the device route, in job order, and the truth of every
    contig. A region is a dict: contig, start, end, jobs (what the workers
    do for it), and in training mode spans: one (align index, lo, hi,
    sub_start, sub_end) per kept truth alignment that labels something, in
    the order _generate_train takes them. A region whose truth the label
    kernels refuse has one "host" job instead."""
    from .labels import get_aligns
    from .ops.labels_device import (label_span, pack_truth, region_aligns,
                                    scan_truth)

    regions, truths = [], {}
    for name, seq in refs:
        if bam_y is not None:
            aligns = get_aligns(bam_y, name, 0, len(seq))  # once per contig
            pack = pack_truth(aligns)
            scan = scan_truth(pack)
            truths[name] = (aligns, pack)
        for start, end in generate_regions(len(seq), cfg.region_size,
                                           cfg.region_overlap):
            region = {"contig": name, "start": start, "end": end,
                      "spans": None, "host": None}
            if bam_y is None:
                region["jobs"] = [("reads", (bam_x, name, start, end, cfg))]
                regions.append(region)
                continue
            kept = region_aligns(aligns, pack["ref_end"], start, end)
            if not kept:
                continue
            refused = [i for i, _ in kept if scan[i].err]
            if refused:
                region["host"] = (f"truth alignment {aligns[refused[0]].qname!r}"
                                  " has a zero-length or interior clip op")
                region["jobs"] = [("host", (bam_x, bam_y, name, start, end,
                                            host_cfg))]
                regions.append(region)
                continue
            spans = []
            for i, a in kept:
                lo, hi = max(start, a.start), min(end, a.end)
                sub = label_span(pack, i, lo, hi, scan) if lo < hi else None
                if sub is not None and sub[1] > sub[0]:
                    spans.append((i, lo, hi, sub[0], sub[1]))
            if not spans:
                continue
            region["spans"] = spans
            region["jobs"] = [("reads", (bam_x, name, s, e, cfg))
                              for _, _, _, s, e in spans]
            regions.append(region)
    return regions, truths


class _Refused(Exception):
    """The device builder does not take this region."""


class _Staging:
    """Two sets of pinned host buffers. A region's windows are copied into
    one on a side stream while the next region is built; the caller writes a
    set out before the one after next is staged."""

    def __init__(self, device, train: bool):
        import torch

        self.torch, self.device, self.train = torch, device, train
        self.stream = torch.cuda.Stream(device)
        self.sets = [None, None]
        self.turn = 0

    def _buffers(self, n: int):
        torch = self.torch
        cur = self.sets[self.turn]
        if cur is None or cur[0].shape[0] < n:
            cap = n + n // 4
            cur = [torch.empty((cap, C.WINDOW_ROWS, C.WINDOW_COLS),
                               dtype=torch.uint8, pin_memory=True),
                   torch.empty((cap, C.WINDOW_COLS, 2), dtype=torch.int32,
                               pin_memory=True),
                   torch.empty((cap, C.WINDOW_COLS), dtype=torch.uint8,
                               pin_memory=True) if self.train else None]
            self.sets[self.turn] = cur
        self.turn ^= 1
        return cur

    def put(self, parts):
        """parts: [(x, pos, labels or None)] device tensors -> (positions,
        examples, labels) numpy views of the staging and the event after
        which they hold the data."""
        torch = self.torch
        n = sum(int(x.shape[0]) for x, _, _ in parts)
        bx, bp, bl = self._buffers(n)
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(self.stream):
            off = 0
            for x, pos, lab in parts:
                k = int(x.shape[0])
                for dst, src in ((bx, x), (bp, pos), (bl, lab)):
                    if src is not None:
                        dst[off : off + k].copy_(src, non_blocking=True)
                        src.record_stream(self.stream)
                off += k
            done = torch.cuda.Event()
            done.record(self.stream)
        return (bp[:n].numpy(), bx[:n].numpy(),
                bl[:n].numpy() if self.train else None), done


def _build_region(region, results, cfg, device, truth):
    """One region on the GPU: windows of every span (build_windows), their
    labels (label_windows), UNKNOWN-labelled windows dropped. Returns
    [(x, pos, labels or None)] device tensors; raises _Refused when the
    window builder refuses a span."""
    from .ops.labels_device import LABEL_ERR_RANGE
    from .ops.windows import build_windows

    parts = []
    spans = region["spans"] or [None]
    for span, result in zip(spans, results):
        try:
            x, pos = build_windows(result[3], cfg, device)
        except RuntimeError as e:
            # zero-length CIGAR op, or more columns than the bound
            if "build_windows:" in str(e):
                raise _Refused(str(e).splitlines()[0]) from None
            raise
        if x.shape[0] == 0:
            continue
        if span is None:
            parts.append((x, pos, None))
            continue
        index, lo, hi, _, _ = span
        labels, keep, err = truth.label_windows(pos, index, lo, hi)
        if int(err) & LABEL_ERR_RANGE:
            raise RuntimeError(
                f"{region['contig']}:{region['start']}-{region['end']}: a "
                f"window column lies outside the label span [{lo}, {hi}) of "
                f"truth alignment {index}")
        if not bool(keep.all()):
            # windows with an UNKNOWN label are rare: torch's index_select
            # only runs for the spans that have one
            idx = keep.nonzero().squeeze(1)
            x, pos, labels = (t.index_select(0, idx) for t in (x, pos, labels))
        if x.shape[0]:
            parts.append((x, pos, labels))
    return parts


def _run_device(ref_path, bam_x, out_path, bam_y, workers, cfg, log, device):
    from .ops.windows import check_geometry

    dev_type = _device_type(device)
    if dev_type != "cuda":
        raise ValueError(
            "extract='device' builds the windows on the GPU and needs a GPU "
            f"device (got {dev_type!r}); use extract='host'")
    check_geometry(cfg)
    refs = list(read_fasta(ref_path))
    # the oracle, and what a refused region is rebuilt with
    host_cfg = dataclasses.replace(cfg, sampler="counter")

    # Start the workers first, in fresh interpreters: forking a process that
    # has initialised HIP is unsafe (and the caller may have done so
    # already), and only this process may hold the GPU.
    pool = None
    if workers > 1:
        pool = multiprocessing.get_context("spawn").Pool(processes=workers)
    try:
        return _extract_device(refs, bam_x, out_path, bam_y, workers, cfg,
                               host_cfg, log, device, pool)
    finally:
        if pool is not None:
            pool.terminate()
            pool.join()


def _extract_device(refs, bam_x, out_path, bam_y, workers, cfg, host_cfg, log,
                    device, pool) -> int:
    import torch

    from .ops.labels_device import TruthPack

    inference = bam_y is None
    t0 = time.time()
    regions, truths = _plan_device(refs, bam_x, bam_y, cfg, host_cfg)
    jobs = [job for region in regions for job in region["jobs"]]
    log(f"feature generation: {len(regions)} regions, {len(jobs)} jobs, "
        f"{workers} workers, windows on the device")
    device = torch.device("cuda" if device is None else device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    results = pool.imap(device_job, jobs) if pool is not None \
        else map(device_job, jobs)

    n_windows = n_errors = 0
    with torch.cuda.device(device), \
            RkwWriter(out_path, inference=inference) as writer:
        writer.write_contigs(refs)
        staging = _Staging(device, train=not inference)
        pending = None  # the staged region that is not written yet
        truth, truth_contig = None, None

        def flush():
            nonlocal pending, n_windows
            if pending is not None:
                region, (positions, examples, labs), done = pending
                done.synchronize()
                writer.store(region["contig"], region["start"], region["end"],
                             positions, examples, labs)
                n_windows += len(positions)
                pending = None

        def store_host(region, result):
            nonlocal n_windows
            flush()
            if result is None:
                return
            contig, start, end, positions, examples, labs = result
            writer.store(contig, start, end, positions, examples, labs)
            n_windows += len(positions)

        for region in regions:
            name = f"{region['contig']}:{region['start']}-{region['end']}"
            got, failed = [], False
            for job in region["jobs"]:
                result = next(results)
                if result is not None and result[0] == "__error__":
                    # same fence as the host route: one in-parent retry
                    log(f"WARNING: region {result[1]} failed: {result[2]} "
                        "(retrying once)")
                    result = device_job(job)
                    if result is not None and result[0] == "__error__":
                        log(f"WARNING: region {result[1]} failed twice: "
                            f"{result[2]} (skipped)")
                        failed = True
                got.append(result)
            if failed:
                n_errors += 1
                continue
            if region["host"]:
                log(f"region {name}: {region['host']}; built on the host")
                store_host(region, got[0])
                continue
            if not inference and region["contig"] != truth_contig:
                aligns, pack = truths[region["contig"]]
                truth = TruthPack(aligns, device, pack=pack)  # once a contig
                truth_contig = region["contig"]
            try:
                parts = _build_region(region, got, cfg, device, truth)
            except _Refused as e:
                log(f"region {name}: {e}; built on the host")
                args = (bam_x, region["contig"], region["start"],
                        region["end"], host_cfg)
                result = device_job(("host", args if inference else
                                     (bam_x, bam_y) + args[1:]))
                if result is not None and result[0] == "__error__":
                    n_errors += 1
                    log(f"WARNING: region {result[1]} failed: {result[2]} "
                        "(skipped)")
                    continue
                store_host(region, result)
                continue
            if not parts:
                continue
            staged = staging.put(parts)
            flush()  # the region before, while this one's copy runs
            pending = (region,) + staged
        flush()
    dt = time.time() - t0
    log(f"wrote {n_windows} windows to {out_path} in {dt:.1f}s "
        f"({n_windows / max(dt, 1e-9):.0f} windows/s)"
        + (f"; {n_errors} regions FAILED and were skipped" if n_errors else ""))
    return n_windows


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("ref", help="draft assembly FASTA")
    p.add_argument("X", help="reads-to-draft BAM (indexed)")
    p.add_argument("o", help="output .rkw path")
    p.add_argument("--Y", default=None, help="truth-to-draft BAM (training mode)")
    p.add_argument("--t", type=int, default=1, help="worker processes")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--sampler", choices=("mt19937", "counter"),
                   default="mt19937", help="row sampler (ops/cpp/pileup.h)")
    p.add_argument("--extract", choices=("host", "device"), default="host",
                   help="where windows (and labels) are built: the workers "
                        "(host) or the GPU, from packed reads (device: "
                        "counter sampler)")
    a = p.parse_args(argv)
    cfg = FeatureConfig(seed=a.seed, sampler=a.sampler)
    run(a.ref, a.X, a.o, bam_y=a.Y, workers=a.t, cfg=cfg, extract=a.extract)


if __name__ == "__main__":
    main()
