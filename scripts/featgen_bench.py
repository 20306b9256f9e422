"""Feature-generation throughput: synthetic assembly -> windows/s.

  python scripts/featgen_bench.py [genome_kb] [cov] [--Y]
      [--extract host|device|host,device] [--workers 1,4,8] [--repeat N]
      [--sampler counter|mt19937] [--region N] [--limit SECONDS] [--dir DIR]

The reference's practical wall time is dominated by this stage (pileup walk +
window emission over htslib). Builds a synthetic assembly with
tests/simple_align.build_assembly, then times `features.run` over every
(route, worker count) asked for: the host route (the C++ window builder in
the workers, CPU only) and, with --extract device, the device route (workers
pack reads, windows and labels are built on the GPU). --Y times training
extraction (windows joined with truth labels) instead of inference windows.

--repeat N runs the whole list N times in turn (a, b, a, b, ...), so that
drift of the machine hits all of them alike. Every run is a process of its
own under `timeout` (--limit seconds): one that hangs or faults ends there and
nothing is started after it. Each prints one JSON line with wall seconds and
windows/s; its RKW file is deleted afterwards. The host route is timed with
the counter sampler by default, the one the device route always uses, so both
write the same file.
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


def make_case(d, kb, cov):
    import numpy as np

    from tests.simple_align import build_assembly

    build_assembly(np.random.default_rng(0), d, length=kb * 1000, cov=cov,
                   read_len=3000)


def run_one(a):
    """One (route, workers) run, in this (child) process."""
    from roko_amd import features as F
    from roko_amd.config import FeatureConfig

    out = os.path.join(a.dir, f"{a.step}_{a.t}_{os.getpid()}.rkw")
    cfg = FeatureConfig(sampler=a.sampler, region_size=a.region)
    kw = {"extract": "device"} if a.step == "device" else {}
    t0 = time.perf_counter()
    try:
        n = F.run(os.path.join(a.dir, "draft.fasta"),
                  os.path.join(a.dir, "reads.bam"), out,
                  bam_y=os.path.join(a.dir, "truth.bam") if a.Y else None,
                  workers=a.t, cfg=cfg, log=lambda *x: None, **kw)
        dt = time.perf_counter() - t0
        mb = os.path.getsize(out) / 1e6
    finally:
        if os.path.exists(out):
            os.remove(out)
    print(json.dumps({"route": a.step, "train": bool(a.Y), "workers": a.t,
                      "windows": n, "wall_s": round(dt, 3),
                      "windows_per_s": round(n / dt, 1),
                      "rkw_mb": round(mb, 1)}), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("kb", nargs="?", type=int, default=200,
                   help="genome size, kb")
    p.add_argument("cov", nargs="?", type=int, default=30, help="coverage")
    p.add_argument("--Y", action="store_true",
                   help="training extraction (truth labels)")
    p.add_argument("--extract", default="host",
                   help="routes to time: host, device or host,device")
    p.add_argument("--workers", default="1,4,8",
                   help="worker counts, comma-separated (device: the first "
                        "two)")
    p.add_argument("--device-workers", default=None,
                   help="worker counts of the device route")
    p.add_argument("--repeat", type=int, default=1)
    p.add_argument("--sampler", choices=("counter", "mt19937"),
                   default="counter", help="row sampler of the host route")
    p.add_argument("--region", type=int, default=100_000)
    p.add_argument("--limit", type=int, default=600,
                   help="time limit per run, seconds")
    p.add_argument("--dir", default=None, help="work directory")
    p.add_argument("--step", default=None, help="(internal) run one route")
    p.add_argument("--t", type=int, default=1, help="(internal) workers")
    a = p.parse_args()
    if a.step:
        run_one(a)
        return

    routes = [r for r in a.extract.split(",") if r]
    for r in routes:
        if r not in ("host", "device"):
            p.error(f"unknown route {r!r}")
    workers = [int(w) for w in a.workers.split(",")]
    dev_workers = ([int(w) for w in a.device_workers.split(",")]
                   if a.device_workers else workers[:2])
    d = a.dir or tempfile.mkdtemp(prefix="featgen_bench_")
    os.makedirs(d, exist_ok=True)
    if not os.path.exists(os.path.join(d, "truth.bam")):
        t0 = time.perf_counter()
        make_case(d, a.kb, a.cov)
        bam_mb = os.path.getsize(os.path.join(d, "reads.bam")) / 1e6
        print(json.dumps({"step": "make_case", "kb": a.kb, "cov": a.cov,
                          "bam_mb": round(bam_mb, 1),
                          "wall_s": round(time.perf_counter() - t0, 1)}),
              flush=True)
    runs = [(r, w) for r in routes
            for w in (dev_workers if r == "device" else workers)]
    for route, w in runs * max(a.repeat, 1):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable,
               os.path.abspath(__file__), "--step", route, "--t", str(w),
               "--dir", d, "--sampler", a.sampler, "--region", str(a.region)]
        if a.Y:
            cmd.append("--Y")
        rc = subprocess.call(cmd)
        if rc != 0:
            print(json.dumps({"route": route, "workers": w, "failed": rc}),
                  flush=True)
            sys.exit(rc)  # start nothing more after a failure


if __name__ == "__main__":
    main()
