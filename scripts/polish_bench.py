"""End-to-end polishing rate: draft + BAM -> FASTA, seven ways.

  python scripts/polish_bench.py [--ref-len N] [--cov C] [--t WORKERS]
      [--b BATCH] [--limit SECONDS] [--dir DIR] [--routes a,b,...]
      [--repeat N] [--fastq]

Builds a synthetic assembly (the generators of tests/test_gpu_e2e.py::
_make_case, size given by --ref-len), then times

  two_step      features -> RKW file -> infer(votes="host")
  infer_device  features -> RKW file -> infer(votes="device")
  polish        roko_amd.polish.polish (no file, votes on the device)
  polish_host_counter   polish with the counter row sampler
  polish_device         polish(extract="device"): workers pack reads, the
                        windows are built on the GPU (counter sampler)
  polish_device_vcf     polish_device with out_vcf: quality tables on, the
                        edits compacted on the GPU, the VCF written
  polish_device_stitch  polish_device with stitch="device" and a FASTQ: the
                        polished sequence and qualities written on the GPU

--routes picks a subset; --repeat N runs the chosen routes N times in turn
(a, b, a, b, ...), so that drift of the machine hits all of them alike.

Each way runs in a process of its own under `timeout` (--limit seconds), so
one that hangs or faults ends there and nothing is started after it. Each
prints one JSON line: wall time, windows/s, bases/s (draft bases per second
of wall time), and for the file routes the split between extraction and
inference. A last line says whether the FASTA files of the routes that ran
are identical within each sampler (the two samplers draw different rows).
The model is randomly initialised: rates do not depend on the weights.

--fastq makes every route but two_step (host votes) also write a FASTQ with
per-base qualities, which on the GPU turns on the quality output of the head
kernel, the fused vote scatter and the quality consensus; each JSON line then
carries "fastq": true and the device memory the quality tables add (8 bytes
per column slot, 32 per draft base). Run once with and once without to see
what the feature costs.
"""

import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = ("two_step", "infer_device", "polish")
COUNTER_STEPS = ("polish_host_counter", "polish_device",
                 "polish_device_vcf", "polish_device_stitch")
ALL_STEPS = STEPS + COUNTER_STEPS


def make_case(d, ref_len, cov, seed=7):
    import numpy as np

    from roko_amd.io.bamio import write_bam
    from roko_amd.io.fasta import write_fasta
    from tests.simple_align import BASES, EditScript

    rng = np.random.default_rng(seed)
    truth = "".join(BASES[int(b)] for b in rng.integers(0, 4, ref_len))
    es = EditScript(rng, truth, sub_rate=0.01, ins_rate=0.003, del_rate=0.003)
    write_fasta(os.path.join(d, "draft.fasta"), [("ctg1", es.draft)])
    reads, rlen = [], 400
    for i in range(max(1, cov * len(truth) // rlen)):
        s = int(rng.integers(0, max(1, len(truth) - rlen)))
        rec = es.align_substring(f"read{i}", s, s + rlen,
                                 flag=16 if i % 2 else 0)
        if rec is not None:
            reads.append(rec)
    reads.sort(key=lambda r: (r.tid, r.pos))
    write_bam(os.path.join(d, "reads.bam"), [("ctg1", len(es.draft))], reads)
    return len(es.draft)


def run_step(step, d, workers, batch, region, fastq=False):
    """One route, in this (child) process; prints its JSON line."""
    from roko_amd import config as C
    from roko_amd.config import FeatureConfig
    from roko_amd.features import run as features_run
    from roko_amd.inference import infer
    from roko_amd.io.fasta import read_fasta
    from roko_amd.polish import polish

    quiet = lambda *a, **k: None  # noqa: E731
    draft = os.path.join(d, "draft.fasta")
    bam = os.path.join(d, "reads.bam")
    ckpt = os.path.join(d, "model.pth")
    out = os.path.join(d, f"{step}.fasta")
    cfg = FeatureConfig(seed=1, region_size=region)
    draft_bases = sum(len(s) for _, s in read_fasta(draft))
    rec = {"step": step, "workers": workers, "batch": batch,
           "draft_bases": draft_bases}
    out_fastq = None
    if (fastq and step != "two_step") or step == "polish_device_stitch":
        out_fastq = os.path.join(d, f"{step}.fastq")
        rec.update(fastq=True,
                   qsum_bytes=8 * (C.MAX_INS + 1) * draft_bases)
    out_vcf = None
    if step == "polish_device_vcf":
        out_vcf = os.path.join(d, f"{step}.vcf")
        rec.update(vcf=True)
    t0 = time.time()
    if step.startswith("polish"):
        from roko_amd.polish import LAST_RUN

        if step != "polish":
            cfg.sampler = "counter"
        polish(draft, bam, ckpt, out, workers=workers, batch_size=batch,
               cfg=cfg, log=quiet,
               extract="device" if step.startswith("polish_device")
               else "host",
               out_fastq=out_fastq, out_vcf=out_vcf,
               stitch="device" if step == "polish_device_stitch" else "host")
        n = LAST_RUN["windows"]
    else:
        rkw = os.path.join(d, f"{step}.rkw")
        n = features_run(draft, bam, rkw, workers=workers, cfg=cfg, log=quiet)
        rec["features_s"] = round(time.time() - t0, 3)
        t1 = time.time()
        infer(rkw, ckpt, out, batch_size=batch, log=quiet,
              votes="host" if step == "two_step" else "device",
              out_fastq=out_fastq)
        rec["infer_s"] = round(time.time() - t1, 3)
    wall = time.time() - t0
    if out_vcf:
        with open(out_vcf) as fh:
            ne = [int(line.rsplit("NE=", 1)[1].split(";")[0]) for line in fh
                  if not line.startswith("#")]
        rec.update(vcf_records=len(ne), vcf_edits=sum(ne))
    rec.update(windows=n, wall_s=round(wall, 3),
               windows_per_s=round(n / wall, 1),
               bases_per_s=round(draft_bases / wall, 1),
               window_bases_per_s=round(n * C.WINDOW_STRIDE / wall, 1))
    print(json.dumps(rec), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--ref-len", type=int, default=200_000)
    p.add_argument("--cov", type=int, default=25)
    p.add_argument("--t", type=int, default=4, help="extractor workers")
    p.add_argument("--b", type=int, default=128, help="batch size")
    p.add_argument("--region", type=int, default=20_000,
                   help="region size (the unit of extractor parallelism)")
    p.add_argument("--limit", type=int, default=240,
                   help="time limit per route, seconds")
    p.add_argument("--dir", default=None, help="work directory")
    p.add_argument("--routes", default=",".join(ALL_STEPS),
                   help="comma-separated routes to run, in this order")
    p.add_argument("--repeat", type=int, default=1,
                   help="run the chosen routes this many times, in turn")
    p.add_argument("--fastq", action="store_true",
                   help="also write FASTQ (per-base qualities) on every "
                        "route but two_step")
    p.add_argument("--step", choices=ALL_STEPS, default=None,
                   help="(internal) run one route in this process")
    a = p.parse_args()
    if a.step:
        run_step(a.step, a.dir, a.t, a.b, a.region, a.fastq)
        return

    import torch

    from roko_amd.model import RokoModel

    d = a.dir or tempfile.mkdtemp(prefix="polish_bench_")
    os.makedirs(d, exist_ok=True)
    t0 = time.time()
    n = make_case(d, a.ref_len, a.cov)
    torch.manual_seed(0)
    torch.save(RokoModel().state_dict(), os.path.join(d, "model.pth"))
    print(json.dumps({"step": "make_case", "draft_bases": n,
                      "wall_s": round(time.time() - t0, 1)}), flush=True)
    routes = [r for r in a.routes.split(",") if r]
    for r in routes:
        if r not in ALL_STEPS:
            p.error(f"unknown route {r!r} (known: {', '.join(ALL_STEPS)})")
    for step in routes * max(a.repeat, 1):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable,
               os.path.abspath(__file__), "--step", step, "--dir", d,
               "--t", str(a.t), "--b", str(a.b), "--region", str(a.region)]
        if a.fastq:
            cmd.append("--fastq")
        rc = subprocess.call(cmd)
        if rc != 0:
            print(json.dumps({"step": step, "failed": rc}), flush=True)
            sys.exit(rc)  # start nothing more after a failure
    rec = {"step": "compare"}
    for key, group in (("identical", STEPS),
                       ("identical_counter", COUNTER_STEPS)):
        blobs = {open(os.path.join(d, f"{s}.fasta"), "rb").read()
                 for s in group if s in routes}
        if blobs:
            rec[key] = len(blobs) == 1
        if a.fastq:
            blobs = {open(os.path.join(d, f"{s}.fastq"), "rb").read()
                     for s in group if s in routes and s != "two_step"}
            if blobs:
                rec[key + "_fastq"] = len(blobs) == 1
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
