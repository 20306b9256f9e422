"""Does --min-qual help? Polished-vs-truth errors against the threshold.

For every noisy-read cell of scripts/quality_calibration.py (read error x
coverage, the same brief training on one assembly and the same unseen second
assembly) this polishes the unseen assembly at min_qual in 0, 5, 10, 15, 20,
30 (`polish(min_qual=, out_vcf=)`) and prints, per cell and threshold, the
errors of the polished sequence against the truth (accuracy.seq_stats: edit
distance) and the number of edits the filter rejected: the edits listed by
the unfiltered VCF minus those the filtered one lists (sums of NE).

Prints a markdown table (docs/ACCURACY.md "Quality calibration"). Every cell
runs in a fresh child process under `timeout`, so a cell that fails or hangs
ends the run there and nothing is started after it. Runs on the GPU when
there is one, else on the CPU (about a minute per cell).
Usage: python scripts/minqual_sweep.py [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from roko_amd import features as F
from roko_amd.accuracy import seq_stats
from roko_amd.config import TrainConfig
from roko_amd.polish import polish
from roko_amd.train import train
from tests.simple_align import build_assembly

MIN_QUALS = (0, 5, 10, 15, 20, 30)
QUIET = lambda *a, **k: None  # noqa: E731


def vcf_edits(path):
    with open(path) as fh:
        return sum(int(line.rsplit("NE=", 1)[1].split(";")[0]) for line in fh
                   if not line.startswith("#"))


def run_cell(read_err, cov):
    """The training and the assemblies of quality_calibration.run_cell."""
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
        model = model.eval()
        rec = {"draft": seq_stats(held["draft"], held["truth"])
               ["edit_distance"], "errors": [], "edits": []}
        for q in MIN_QUALS:
            vcf = os.path.join(td, f"q{q}.vcf")
            out = polish(held["draft_fasta"], held["reads_bam"], None, None,
                         workers=1, batch_size=32, cfg=fcfg, model=model,
                         log=QUIET, out_vcf=vcf, min_qual=q)
            (seq,) = out.values()
            rec["errors"].append(
                seq_stats(seq, held["truth"])["edit_distance"])
            rec["edits"].append(vcf_edits(vcf))
    return rec


def main():
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--out", default=None, help="also write the table here")
    p.add_argument("--limit", type=int, default=600,
                   help="time limit per cell, seconds")
    p.add_argument("--cell", nargs=2, default=None,
                   metavar=("READ_ERR", "COV"),
                   help="(internal) run one cell in this process")
    a = p.parse_args()
    if a.cell:
        torch.manual_seed(0)
        print(json.dumps(run_cell(float(a.cell[0]), int(a.cell[1]))),
              flush=True)
        return
    head = "| read error | coverage | draft errors | " + " | ".join(
        f"Q>={q}" for q in MIN_QUALS) + " |"
    lines = ["polished-vs-truth errors (edits rejected) per min_qual", "",
             head, "|---" * (3 + len(MIN_QUALS)) + "|"]
    print("\n".join(lines), flush=True)
    total_err = np.zeros(len(MIN_QUALS), int)
    total_rej = np.zeros(len(MIN_QUALS), int)
    total_draft = 0
    for read_err in (0.03, 0.05, 0.10):
        for cov in (10, 20, 40):
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable,
                   os.path.abspath(__file__), "--cell", str(read_err),
                   str(cov)]
            res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            if res.returncode != 0:
                sys.exit(res.returncode)  # start nothing more after a failure
            rec = json.loads(res.stdout.strip().splitlines()[-1])
            err = np.array(rec["errors"])
            rej = rec["edits"][0] - np.array(rec["edits"])
            total_err, total_rej = total_err + err, total_rej + rej
            total_draft += rec["draft"]
            lines.append(f"| {read_err:.0%} | {cov}x | {rec['draft']} | "
                         + " | ".join(f"{e} ({r})" for e, r in zip(err, rej))
                         + " |")
            print(lines[-1], flush=True)
    lines.append(f"| all | all | {total_draft} | "
                 + " | ".join(f"{e} ({r})"
                              for e, r in zip(total_err, total_rej)) + " |")
    print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
