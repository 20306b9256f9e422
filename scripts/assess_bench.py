"""Assessment at genome scale: the exact wavefront aligner on the device and
on the CPU, and the banded aligner where it runs at all.

Synthetic truth/assembly pairs (default 1 Mb and 4 Mb at 0.05 % and 1.4 %
divergence, substitutions : insertions : deletions = 2 : 1 : 1 as in
tests/simple_align.py). Every figure comes from a process of its own
(`--one`), three timed rounds after one small warm-up call; the driver prints
one JSON line per figure and a markdown table.

  python scripts/assess_bench.py                       # all figures
  python scripts/assess_bench.py --one device 1000000 0.014

Kernel times come from a separate run under the profiler, e.g.
  rocprofv3 --kernel-trace --stats -d OUT -- \\
      python scripts/assess_bench.py --one device 1000000 0.014 --rounds 1
"""

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BASES = np.frombuffer(b"ACGT", dtype=np.uint8)


def make_pair(length: int, div: float, seed: int = 5):
    """(assembly, truth) as ASCII bytes; per truth base div/2 substitution,
    div/4 deletion, and div/4 inserted bases after it."""
    rng = np.random.default_rng(seed)
    truth = BASES[rng.integers(0, 4, length)]
    r = rng.random(length)
    keep = r >= div / 4
    sub = (r >= div / 4) & (r < 3 * div / 4)
    asm = truth.copy()
    asm[sub] = BASES[(np.searchsorted(BASES, truth[sub])
                      + rng.integers(1, 4, int(sub.sum()))) % 4]
    ins_at = np.flatnonzero(rng.random(length) < div / 4)
    out = np.insert(asm[keep], np.searchsorted(np.flatnonzero(keep), ins_at),
                    BASES[rng.integers(0, 4, len(ins_at))])
    return out.tobytes(), truth.tobytes()


def run_one(route: str, length: int, div: float, rounds: int) -> dict:
    from roko_amd import wfa
    from roko_amd.ops import pileup_ext

    asm, truth = make_pair(length, div)
    res = {"route": route, "length": length, "divergence": div}
    if route == "banded":
        q, t = asm.decode(), truth.decode()
        band = min(len(t), 32 + len(t) // 20)  # accuracy.seq_stats, band=0

        def call():
            return pileup_ext().align_stats(q, t, band=band)["edit_distance"]
    else:
        dev = route == "device"
        if dev:
            import torch

            wfa.align(asm[:5000], truth[:5000], device=True)  # warm-up
            torch.cuda.synchronize()

        def call():
            return wfa.align(asm, truth, device=dev)["edit_distance"]
    times = []
    try:
        for _ in range(rounds):
            t0 = time.perf_counter()
            dist = call()
            times.append(time.perf_counter() - t0)
        res.update(edit_distance=int(dist), seconds=times,
                   median=statistics.median(times))
    except (RuntimeError, MemoryError) as e:
        res["refused"] = str(e).splitlines()[0][:120]
    return res


def main() -> None:
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--one", nargs=3, metavar=("ROUTE", "LENGTH", "DIV"))
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--sizes", type=int, nargs="+",
                   default=[1_000_000, 4_000_000])
    p.add_argument("--divs", type=float, nargs="+", default=[0.0005, 0.014])
    p.add_argument("--routes", nargs="+",
                   default=["device", "cpu", "banded"])
    p.add_argument("--timeout", type=float, default=600.0,
                   help="seconds one figure's process may take")
    a = p.parse_args()
    if a.one:
        print(json.dumps(run_one(a.one[0], int(a.one[1]), float(a.one[2]),
                                 a.rounds)), flush=True)
        return
    rows = []
    for length in a.sizes:
        for div in a.divs:
            for route in a.routes:
                out = subprocess.run(
                    [sys.executable, os.path.abspath(__file__), "--one",
                     route, str(length), str(div), "--rounds",
                     str(a.rounds)],
                    capture_output=True, text=True, timeout=a.timeout)
                line = out.stdout.strip().splitlines()[-1:] or [""]
                try:
                    row = json.loads(line[0])
                except ValueError:
                    row = {"route": route, "length": length,
                           "divergence": div,
                           "refused": f"exit {out.returncode}: "
                                      f"{out.stderr.strip()[-120:]}"}
                print(json.dumps(row), flush=True)
                rows.append(row)
                if out.returncode != 0:  # a crashed figure ends the run
                    raise SystemExit(f"{route} {length} {div}: exit "
                                     f"{out.returncode}")
    print("\n| length | divergence | route | edit distance | median s | "
          "rounds s |\n|---|---|---|---|---|---|")
    for r in rows:
        if "refused" in r:
            print(f"| {r['length']} | {r['divergence']:.2%} | {r['route']} | "
                  f"- | refused | {r['refused']} |")
        else:
            print(f"| {r['length']} | {r['divergence']:.2%} | {r['route']} | "
                  f"{r['edit_distance']} | {r['median']:.4f} | "
                  + " ".join(f"{x:.4f}" for x in r["seconds"]) + " |")


if __name__ == "__main__":
    main()
