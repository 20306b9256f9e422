"""Calibration of the per-base qualities: emitted Q against observed error.

For every noisy-read cell of scripts/accuracy_bench.py (read error x
coverage, synthetic scenario with the truth known exactly) this trains
briefly (100 steps of 32 windows, as many windows as accuracy_bench.py sees
in its 200 steps of 16; the GPU train path takes batches of 32) on one
assembly, polishes a SECOND assembly of the same scenario (another seed, so
the model has not seen it) with `polish(out_fastq=)`,
aligns polished to truth with `_pileup.align_cigar`, and tabulates the emitted
Q in bins of 10 against the observed error rate of the bases in the bin.

An emitted base is an error when it is aligned to a different truth base (M,
mismatch) or to none (I). A truth base missing from the polished sequence (D)
has no emitted base and therefore no quality; those are counted beside the
table. Prints a markdown table (docs/ACCURACY.md "Quality calibration").

Every cell runs in a fresh child process under `timeout`, so a cell that
fails or hangs ends the run there and nothing is started after it. Runs on
the GPU when there is one, else on the CPU (about a minute per cell).
Usage: python scripts/quality_calibration.py [--out FILE]
"""
import argparse
import json
import math
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from roko_amd import features as F
from roko_amd.config import TrainConfig
from roko_amd.io.fasta import read_fastq
from roko_amd.ops import pileup_ext
from roko_amd.polish import polish
from roko_amd.train import train
from tests.simple_align import build_assembly

BINS = [(0, 9), (10, 19), (20, 29), (30, 39), (40, 49), (50, 59), (60, 60)]
QUIET = lambda *a, **k: None  # noqa: E731


def base_errors(polished: str, truth: str):
    """(per-base error flags of `polished`, number of truth bases missing
    from it) from the unit-cost global alignment."""
    px = pileup_ext()
    band = 32 + len(truth) // 20
    while True:
        try:
            res = px.align_cigar(polished, truth, band=band)
            break
        except RuntimeError:
            if band >= max(len(truth), len(polished)):
                raise
            band *= 2
    err = np.zeros(len(polished), dtype=bool)
    i = j = missing = 0
    for n, op in re.findall(r"(\d+)([MID])", res["cigar"]):
        n = int(n)
        if op == "M":
            for k in range(n):
                err[i + k] = polished[i + k] != truth[j + k]
            i, j = i + n, j + n
        elif op == "I":
            err[i : i + n] = True
            i += n
        else:
            missing += n
            j += n
    assert i == len(polished) and j == len(truth)
    return err, missing


def run_cell(read_err, cov):
    fcfg = F.FeatureConfig(region_size=2000, region_overlap=300)
    with tempfile.TemporaryDirectory() as td:
        seen = build_assembly(np.random.default_rng(0), os.path.join(td, "a"),
                              length=3000, cov=cov, read_err=read_err)
        held = build_assembly(np.random.default_rng(1), os.path.join(td, "b"),
                              length=3000, cov=cov, read_err=read_err)
        train_rkw = os.path.join(td, "train.rkw")
        F.run(seen["draft_fasta"], seen["reads_bam"], train_rkw,
              bam_y=seen["truth_bam"], workers=1, cfg=fcfg, log=QUIET)
        model, _ = train(train_rkw, os.path.join(td, "out"),
                         cfg=TrainConfig(batch_size=32, epochs=50, lr=2e-3,
                                         in_memory=True, seed=0),
                         log=QUIET, max_steps=100)
        fastq = os.path.join(td, "held.fastq")
        polish(held["draft_fasta"], held["reads_bam"], None, None, workers=1,
               batch_size=32, cfg=fcfg, model=model.eval(), log=QUIET,
               out_fastq=fastq)
        (_, seq, quals), = list(read_fastq(fastq))
    err, missing = base_errors(seq, held["truth"])
    q = np.frombuffer(quals.encode("ascii"), dtype=np.uint8).astype(int) - 33
    return q, err, missing


def table(bases, errors):
    """Markdown rows from per-Q counts of emitted bases and of errors."""
    rows = []
    for lo, hi in BINS:
        n, e = int(bases[lo:hi + 1].sum()), int(errors[lo:hi + 1].sum())
        rate = e / n if n else float("nan")
        obs = ("-" if n == 0 else ">= %.0f" % (-10 * math.log10(1 / n))
               if e == 0 else "%.1f" % (-10 * math.log10(rate)))
        label = f"{lo}-{hi}" if lo != hi else f"{lo}"
        rows.append(f"| {label} | {n} | {e} | "
                    + ("-" if n == 0 else f"{rate:.4%}") + f" | {obs} |")
    return rows


def main():
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--out", default=None, help="also write the tables here")
    p.add_argument("--limit", type=int, default=600,
                   help="time limit per cell, seconds")
    p.add_argument("--cell", nargs=2, default=None,
                   metavar=("READ_ERR", "COV"),
                   help="(internal) run one cell in this process")
    a = p.parse_args()
    if a.cell:
        torch.manual_seed(0)
        q, err, missing = run_cell(float(a.cell[0]), int(a.cell[1]))
        print(json.dumps({
            "bases": np.bincount(q, minlength=61).tolist(),
            "errors": np.bincount(q[err], minlength=61).tolist(),
            "missing": missing, "mean_q": float(q.mean())}), flush=True)
        return
    lines = []
    bases, errors, all_missing = np.zeros(61, int), np.zeros(61, int), 0
    for read_err in (0.03, 0.05, 0.10):
        for cov in (10, 20, 40):
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable,
                   os.path.abspath(__file__), "--cell", str(read_err),
                   str(cov)]
            res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            if res.returncode != 0:
                sys.exit(res.returncode)  # start nothing more after a failure
            rec = json.loads(res.stdout.strip().splitlines()[-1])
            b, e = np.array(rec["bases"]), np.array(rec["errors"])
            bases, errors = bases + b, errors + e
            all_missing += rec["missing"]
            lines.append(f"cell read_err={read_err:.0%} cov={cov}x: "
                         f"{b.sum()} bases, {e.sum()} wrong, "
                         f"{rec['missing']} truth bases missing, mean Q "
                         f"{rec['mean_q']:.1f}")
            print(lines[-1], flush=True)
    lines += ["", "| emitted Q | bases | errors | observed error | observed Q |",
              "|---|---|---|---|---|"] + table(bases, errors)
    lines.append("")
    lines.append(f"all cells: {bases.sum()} emitted bases, {errors.sum()} "
                 f"wrong; {all_missing} truth bases missing from the "
                 "polished sequences (no quality)")
    text = "\n".join(lines)
    print(text[text.index("| emitted"):], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
