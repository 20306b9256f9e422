"""One-command polish: draft FASTA + reads BAM + .pth -> polished FASTA.

  python -m roko_amd.polish <draft.fasta> <reads.bam> <model.pth> <out.fasta>
      [--t workers] [--b batch] [--seed N] [--extract host|device]
      [--sampler mt19937|counter] [--fastq out.fastq] [--vcf out.vcf]
      [--min-qual Q] [--keep-uncovered] [--stitch host|device]

Does what `features` followed by `inference` does, and writes the same FASTA
byte for byte, without the RKW file between them: region windows stream from
the extractor workers straight into the serving slots. On a GPU the majority
vote happens on the device too (ops/votes.py) — predictions and vote tables
never cross PCIe; one byte per column comes back per contig. Without a GPU
the model's torch forward and the host vote tables are used, as in
`inference.infer`.

With --extract device the workers only inflate, filter and pack the reads
(features.generate_reads); the windows are built on the GPU from those
(ops/windows.py) and handed to the serving slots device to device, so no
window ever exists on the host. That route samples rows with the counter
sampler whatever --sampler says; `--extract host --sampler counter` writes
the same FASTA.

With --fastq PATH a FASTQ is written as well: the same sequences with a Phred
quality per polished base (roko_amd/quality.py), computed on the device on
every GPU route and by the numpy reference on the CPU route. Draft bases that
are copied through unpolished get Q0; a deleted base leaves no trace in the
quality string.

With --vcf PATH a VCF 4.2 of what polishing changed is written as well
(roko_amd/edits.py): every substituted, deleted or inserted draft base with
its quality, adjacent edits merged into one record. A draft base that the
stitch drops because no window covered it is a deletion flagged NOCOV. On
the GPU routes the edits are compacted on the device from the vote tables
(ops/hip/edits.hip) and only they come back; the CPU route runs the numpy
reference. The FASTA and FASTQ do not depend on it.

With --min-qual Q (0..60) only edits of quality Q or more are applied: a
rejected substitution or deletion leaves the draft base, at Q0, and a rejected
insertion leaves nothing. With --keep-uncovered a draft base inside the
polished span that no window covered is kept (Q0) instead of dropped. Either
option turns the quality tables on; the rules are roko_amd/stitch.py. The VCF
then lists only the applied edits, under a ##roko_filter header line, so
applying its records to the draft still gives the FASTA.

With --stitch device (GPU only) the polished sequence and its quality string
are written on the device from the vote tables (ops/hip/stitch.hip) under the
same filter, and only polished bytes come back; --stitch host, the default,
fetches the per-slot consensus and stitches in numpy. Both write the same
files.

Single process only; for multi-GPU runs use `features` + `inference` under
torchrun.
"""

from __future__ import annotations

import argparse
import multiprocessing
import time
from typing import Dict, List, Optional

import numpy as np

from . import config as C
from .config import FeatureConfig
from .features import generate_infer, generate_reads, generate_regions
from .io.fasta import read_fasta, write_fasta, write_fastq

# NOTE: torch (and everything that imports it) is imported inside polish():
# spawned extractor workers re-import this module when it is the program's
# main module, and must neither pay the torch import nor touch the GPU.


#: figures of the last polish() call in this process (scripts/polish_bench.py)
LAST_RUN: Dict[str, float] = {}


class _DeviceSink:
    """Windows -> serving slots in votes mode -> DeviceVotes. Region arrays
    are packed into the slots' pinned staging with slice copies; a contig is
    stitched from its consensus bytes as soon as its last region is in."""

    def __init__(self, model, batch: int, depth: int, lens: Dict[str, int],
                 quality: bool = False, want_edits: bool = False,
                 min_qual: int = 0, keep_uncovered: bool = False,
                 stitch: str = "host"):
        from .ops.forward import InferencePipeline
        from .ops.votes import DeviceVotes

        self.batch = batch
        # a filter not at its defaults needs quality
        self.filter = (min_qual, keep_uncovered)
        self.stitch = stitch
        self.quality = quality
        self.quals: Dict[str, str] = {}  # contig -> quality string
        self.want_edits = want_edits  # needs quality
        self.edits: Dict[str, np.ndarray] = {}  # contig -> edits.EDIT_DTYPE
        # votes mode runs one batch per slot (coalesce=1)
        self.dv = DeviceVotes(lens, InferencePipeline(model, batch,
                                                      depth=depth,
                                                      coalesce=1,
                                                      quality=quality),
                              quality=quality)
        self.x = self.pos = None
        self.fill = 0

    def add(self, contig: str, positions: np.ndarray,
            examples: np.ndarray) -> None:
        n, off = len(positions), 0
        while off < n:
            if self.fill == 0:
                # syncs the slot that owns this staging pair before reuse
                self.x, self.pos = self.dv.staging()
            k = min(self.batch - self.fill, n - off)
            self.x[self.fill : self.fill + k] = examples[off : off + k]
            self.pos[self.fill : self.fill + k] = positions[off : off + k]
            self.fill += k
            off += k
            if self.fill == self.batch:
                self._submit(contig)

    def _submit(self, contig: str) -> None:
        self.dv.add_batch(contig, self.fill)
        self.fill = 0

    def finish_contig(self, contig: str, draft: str) -> Optional[str]:
        from .inference import stitch_dense

        if self.fill:
            self._submit(contig)  # a slot batch votes into one contig's table
        if not self.dv.has_votes(contig):
            return draft
        if self.want_edits:
            from .stitch import applied_edits

            self.edits[contig] = applied_edits(
                self.dv.edits(contig, draft), *self.filter)  # drains first
        if self.stitch == "device":
            seq, qual = self.dv.stitch(contig, draft, *self.filter)
            self.dv.free(contig)
            if self.quality:
                self.quals[contig] = qual
            return seq
        if self.quality:
            from .quality import stitch_dense_qual
            from .stitch import is_default, stitch_filtered

            maj, qual = self.dv.consensus_quality(contig)  # drains first
            self.dv.free(contig)
            if is_default(*self.filter):
                seq, self.quals[contig] = stitch_dense_qual(draft, maj, qual)
            else:
                seq, self.quals[contig] = stitch_filtered(draft, maj, qual,
                                                          *self.filter)
            return seq
        maj = self.dv.consensus(contig)  # drains the pipeline first
        self.dv.free(contig)
        return stitch_dense(draft, maj)

    def finish(self) -> Dict[str, str]:
        return {}


class _DeviceBuildSink(_DeviceSink):
    """Packed reads -> windows built on the GPU (ops/windows.py) -> serving
    slots in votes mode, device to device, in slices of at most `batch`
    windows. A region's last slice may be short."""

    def __init__(self, model, batch, depth, lens, cfg, device,
                 quality=False, want_edits=False, min_qual=0,
                 keep_uncovered=False, stitch="host"):
        super().__init__(model, batch, depth, lens, quality, want_edits,
                         min_qual, keep_uncovered, stitch)
        self.cfg, self.device = cfg, device

    def add_reads(self, contig: str, pack: dict) -> int:
        from .ops.windows import build_windows

        x, pos = build_windows(pack, self.cfg, self.device)
        n = int(x.shape[0])
        for off in range(0, n, self.batch):
            k = min(self.batch, n - off)
            self.dv.add_device_batch(contig, x[off : off + k],
                                     pos[off : off + k], k)
        return n


class _HostSink:
    """CPU route: the model's torch forward + host vote tables, batched
    exactly as `infer` batches an RKW file (consecutive windows in job order,
    across contig boundaries), so both routes run the model on identical
    batches. Contigs are stitched at the end."""

    def __init__(self, model, batch: int, device, drafts: Dict[str, str],
                 quality: bool = False, want_edits: bool = False,
                 min_qual: int = 0, keep_uncovered: bool = False):
        from .inference import StreamingVotes

        self.model, self.batch, self.device = model, batch, device
        # a filter not at its defaults needs quality
        self.filter = (min_qual, keep_uncovered)
        self.drafts = drafts
        self.quality = quality
        self.quals: Dict[str, str] = {}  # contig -> quality string
        self.want_edits = want_edits  # needs quality
        self.edits: Dict[str, np.ndarray] = {}  # contig -> edits.EDIT_DTYPE
        if quality:
            from .quality import StreamingQualityVotes

            self.sv = StreamingQualityVotes()
        else:
            self.sv = StreamingVotes()
        self.buf: List[tuple] = []  # (contig, positions, examples) chunks
        self.n = 0

    def add(self, contig, positions, examples) -> None:
        if len(positions):
            self.buf.append((contig, positions, examples))
            self.n += len(positions)
        while self.n >= self.batch:
            self._run(self.batch)

    def _run(self, k: int) -> None:
        import torch

        take, rest, got = [], [], 0
        for contig, p, x in self.buf:
            m = min(len(p), k - got)
            if m:
                take.append((contig, p[:m], x[:m]))
                got += m
            if m < len(p):
                rest.append((contig, p[m:], x[m:]))
        self.buf, self.n = rest, self.n - got
        x = torch.from_numpy(np.concatenate([t[2] for t in take]))
        with torch.no_grad():
            logits = self.model(x.to(self.device).long())
        preds = logits.argmax(dim=2).to(torch.uint8).cpu().numpy()
        if self.quality:
            from .quality import phred_units

            units = phred_units(logits.cpu().numpy())
        row = 0
        for contig, p, _ in take:
            for j in range(len(p)):  # StreamingVotes takes single windows
                if self.quality:
                    self.sv.add(contig, np.asarray(p[j]), preds[row + j],
                                units[row + j])
                else:
                    self.sv.add(contig, np.asarray(p[j]), preds[row + j])
            row += len(p)

    def finish_contig(self, contig: str, draft: str) -> Optional[str]:
        return None  # stitched in finish()

    def finish(self) -> Dict[str, str]:
        from .inference import stitch_contig

        if self.n:
            self._run(self.n)
        if not self.quality:
            tables = self.sv.finalize()
            return {name: stitch_contig(self.drafts[name], *tables[name])
                    for name in tables}
        from .quality import stitch_tables
        from .stitch import (applied_edits, is_default,
                             stitch_tables_filtered)

        tables, sums = self.sv.finalize()
        out = {}
        for name in tables:
            if is_default(*self.filter):
                out[name] = stitch_contig(self.drafts[name], *tables[name])
                seq, self.quals[name] = stitch_tables(
                    self.drafts[name], tables[name], sums[name])
                if seq != out[name]:
                    raise RuntimeError(f"{name}: the quality stitch "
                                       "disagrees with the sequence stitch")
            else:
                out[name], self.quals[name] = stitch_tables_filtered(
                    self.drafts[name], tables[name], sums[name],
                    *self.filter)
            if self.want_edits:
                from .edits import table_edits

                self.edits[name] = applied_edits(
                    table_edits(self.drafts[name], tables[name], sums[name]),
                    *self.filter)
        return out


def polish(
    draft_fasta: str,
    reads_bam: str,
    model_path: Optional[str],
    out_fasta: Optional[str],
    workers: int = 1,
    batch_size: int = C.BATCH_SIZE,
    cfg: Optional[FeatureConfig] = None,
    device=None,
    model=None,
    log=print,
    depth: int = 16,
    extract: str = "host",
    out_fastq: Optional[str] = None,
    out_vcf: Optional[str] = None,
    min_qual: int = 0,
    keep_uncovered: bool = False,
    stitch: str = "host",
) -> Dict[str, str]:
    """Polish `draft_fasta` with the reads in `reads_bam`; returns {contig:
    polished sequence} and writes FASTA if `out_fasta` is given, FASTQ
    with a Phred quality per polished base if `out_fastq` is, and a VCF of
    the edits between draft and polished sequence if `out_vcf` is. Regions,
    FeatureConfig and seeding are those of `features.run`; `depth` is the
    number of in-flight batches on the GPU. `extract="device"` builds the
    windows on the GPU from packed reads (counter sampler, whatever
    `cfg.sampler` says); it needs a GPU. `min_qual` (0..60) applies only the
    edits of at least that quality and `keep_uncovered` keeps draft bases no
    window covered (roko_amd/stitch.py); either turns the quality tables on,
    and the VCF then lists only the applied edits. `stitch="device"` writes
    the polished sequence and qualities on the GPU (ops/hip/stitch.hip)
    instead of stitching the fetched consensus in numpy; it needs a GPU."""
    from .stitch import check_filter

    cfg = cfg or FeatureConfig()
    min_qual, keep_uncovered = check_filter(min_qual, keep_uncovered)
    if extract not in ("host", "device"):
        raise ValueError(f"extract must be 'host' or 'device', got {extract!r}")
    if stitch not in ("host", "device"):
        raise ValueError(f"stitch must be 'host' or 'device', got {stitch!r}")
    if stitch == "device" and _device_type(device) != "cuda":
        raise ValueError(
            "stitch='device' writes the polished sequence on the GPU and "
            f"needs a GPU device (got {_device_type(device)!r}); use "
            "stitch='host'")
    if extract == "device":
        from .ops.windows import check_geometry

        dev_type = _device_type(device)
        if dev_type != "cuda":
            raise ValueError(
                "extract='device' builds the windows on the GPU and needs a "
                f"GPU device (got {dev_type!r}); use extract='host'")
        check_geometry(cfg)
    refs = list(read_fasta(draft_fasta))
    jobs = []
    for name, seq in refs:
        for start, end in generate_regions(len(seq), cfg.region_size,
                                           cfg.region_overlap):
            jobs.append((reads_bam, name, start, end, cfg))

    # Start the extractor workers first, in fresh interpreters: forking a
    # process that has initialised HIP is unsafe (and the caller may have
    # done so already), and only this process may hold the GPU.
    pool = None
    if workers > 1 and jobs:
        pool = multiprocessing.get_context("spawn").Pool(processes=workers)
    try:
        return _polish(refs, jobs, pool, model_path, out_fasta, workers,
                       batch_size, device, model, log, depth, extract, cfg,
                       out_fastq, out_vcf, min_qual, keep_uncovered, stitch)
    finally:
        if pool is not None:
            pool.terminate()
            pool.join()


def _device_type(device) -> str:
    """Type of the device polish() would run on, without creating it."""
    import torch

    if device is None:
        return "cuda" if torch.cuda.is_available() else "cpu"
    return torch.device(device).type


def _polish(refs, jobs, pool, model_path, out_fasta, workers, batch_size,
            device, model, log, depth, extract, cfg,
            out_fastq=None, out_vcf=None, min_qual=0, keep_uncovered=False,
            stitch="host") -> Dict[str, str]:
    import torch

    from .model import RokoModel

    if device is None:
        device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    device = torch.device(device)
    if model is None:
        model = RokoModel()
        model.load_reference_checkpoint(model_path)
    model = model.to(device).eval()

    drafts = dict(refs)
    # the edits carry qualities, so a VCF turns the quality tables on; so
    # does a filter not at its defaults, which is decided per slot from them
    from .stitch import is_default, vcf_header

    quality = bool(out_fastq or out_vcf
                   or not is_default(min_qual, keep_uncovered))
    want_edits = bool(out_vcf)
    if extract == "device":
        sink = _DeviceBuildSink(model, batch_size, depth,
                                {n: len(s) for n, s in refs}, cfg, device,
                                quality, want_edits, min_qual, keep_uncovered,
                                stitch)
    elif device.type == "cuda":
        sink = _DeviceSink(model, batch_size, depth,
                           {n: len(s) for n, s in refs}, quality, want_edits,
                           min_qual, keep_uncovered, stitch)
    else:
        sink = _HostSink(model, batch_size, device, drafts, quality,
                         want_edits, min_qual, keep_uncovered)
    worker = generate_reads if extract == "device" else generate_infer
    log(f"polish: {len(jobs)} region jobs, {workers} workers, "
        f"batch {batch_size}, windows on {extract}, votes on {device.type}")

    out: Dict[str, str] = {}
    n_windows = n_errors = 0
    t0 = time.time()
    results = (pool.imap(worker, jobs) if pool is not None
               else map(worker, jobs))
    current = None  # contig being consumed; jobs are in contig order
    for result, job in zip(results, jobs):
        contig = job[1]
        if contig != current:
            if current is not None:
                seq = sink.finish_contig(current, drafts[current])
                if seq is not None:
                    out[current] = seq
            current = contig
        if result[0] == "__error__":
            # same fence as features.run: one in-parent retry, then skip
            log(f"WARNING: region {result[1]} failed: {result[2]} "
                "(retrying once)")
            result = worker(job)
            if result[0] == "__error__":
                n_errors += 1
                log(f"WARNING: region {result[1]} failed twice: "
                    f"{result[2]} (skipped)")
                continue
        if extract == "device":
            n_windows += sink.add_reads(contig, result[3])
            continue
        _, _, _, positions, examples, _ = result
        sink.add(contig, positions, examples)
        n_windows += len(positions)
    if current is not None:
        seq = sink.finish_contig(current, drafts[current])
        if seq is not None:
            out[current] = seq
    out.update(sink.finish())
    for name, seq in refs:  # contigs with no windows come out as the draft
        out.setdefault(name, seq)

    dt = time.time() - t0
    log(f"polished {len(out)} contigs: {n_windows} windows in {dt:.1f}s "
        f"({n_windows / max(dt, 1e-9):.0f} windows/s, "
        f"{n_windows * C.WINDOW_STRIDE / max(dt, 1e-9):.0f} bases/s)"
        + (f"; {n_errors} regions FAILED and were skipped" if n_errors
           else ""))
    LAST_RUN.update(windows=n_windows, seconds=dt, failed_regions=n_errors)
    if out_fasta:
        write_fasta(out_fasta, sorted(out.items()))
        log(f"wrote {len(out)} polished contigs to {out_fasta}")
    if out_fastq:
        from .quality import unpolished_quality

        # a contig the sink gave no qualities for came through as draft
        write_fastq(out_fastq,
                    [(name, seq,
                      sink.quals.get(name) or unpolished_quality(seq))
                     for name, seq in sorted(out.items())])
        log(f"wrote {len(out)} polished contigs with qualities to "
            f"{out_fastq}")
    if out_vcf:
        from .edits import contig_vcf_records, write_vcf

        # a contig without windows has no edits, only its ##contig line
        n = write_vcf(out_vcf, [(name, len(seq)) for name, seq in refs],
                      contig_vcf_records(refs, sink.edits),
                      vcf_header(min_qual, keep_uncovered))
        log(f"wrote {n} records of "
            f"{sum(len(e) for e in sink.edits.values())} edits to {out_vcf}")
    return out


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("draft", help="draft assembly FASTA")
    p.add_argument("bam", help="reads-to-draft BAM (indexed)")
    p.add_argument("model", help=".pth checkpoint (reference format)")
    p.add_argument("out", help="output FASTA path")
    p.add_argument("--t", type=int, default=4,
                   help="extractor worker processes (they never use the GPU)")
    p.add_argument("--b", type=int, default=C.BATCH_SIZE, help="batch size")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--extract", choices=("host", "device"), default="host",
                   help="where windows are built: extractor workers (host) "
                        "or the GPU, from packed reads (device)")
    p.add_argument("--sampler", choices=("mt19937", "counter"),
                   default="mt19937",
                   help="row sampler of --extract host (device: counter)")
    p.add_argument("--fastq", default=None, metavar="PATH",
                   help="also write FASTQ: the same sequences with a Phred "
                        "quality per polished base")
    p.add_argument("--vcf", default=None, metavar="PATH",
                   help="also write VCF: the edits between the draft and "
                        "the polished sequence, with their qualities")
    p.add_argument("--min-qual", type=int, default=0, metavar="Q",
                   help="apply only edits of quality Q or more (0..60); a "
                        "rejected edit leaves the draft as it was, at Q0")
    p.add_argument("--keep-uncovered", action="store_true",
                   help="keep draft bases inside the polished span that no "
                        "window covered (Q0) instead of dropping them")
    p.add_argument("--stitch", choices=("host", "device"), default="host",
                   help="where the polished sequence is put together: numpy "
                        "over the fetched consensus (host) or the GPU, so "
                        "that only polished bytes come back (device)")
    a = p.parse_args(argv)
    polish(a.draft, a.bam, a.model, a.out, workers=a.t, batch_size=a.b,
           cfg=FeatureConfig(seed=a.seed, sampler=a.sampler),
           extract=a.extract, out_fastq=a.fastq, out_vcf=a.vcf,
           min_qual=a.min_qual, keep_uncovered=a.keep_uncovered,
           stitch=a.stitch)


if __name__ == "__main__":
    main()
