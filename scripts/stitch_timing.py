"""Host stitch against device stitch on one large contig.

  python scripts/stitch_timing.py [--bases N] [--reps R] [--min-qual Q]
      [--keep-uncovered] [--limit SECONDS]

Builds the vote and quality tables of one contig (default 4 Mb) on the device
from a seed: every position voted but for one 10 kb hole, about 1.4% of the
positions substituted or deleted or followed by an inserted base, 5% of them
with a GAP vote in an insertion slot. After a warm-up it alternates, in one
process,

  host    DeviceVotes.consensus_quality (two bytes per column slot, 8 per
          draft base, over PCIe) + the numpy stitch (quality.stitch_dense_qual,
          or stitch.stitch_filtered with a filter)
  device  DeviceVotes.stitch (ops/hip/stitch.hip): draft up, three words and
          the polished bytes back

each timed with a host clock around work that ends in a device synchronise,
and prints median, smallest and largest time of each, the bytes each copies
back, and one JSON line. The two outputs must be equal. The measurement runs
in a child process under `timeout` (--limit), so a hang ends there.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build(n, seed=0):
    import numpy as np

    from roko_amd import config as C
    from roko_amd.ops.votes import DeviceVotes

    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 4, n)
    draft = np.frombuffer(b"ACGT", dtype=np.uint8)[codes].tobytes() \
        .decode("ascii")
    hole = n // 2
    pos = np.arange(1000, n - 1000)
    pos = pos[(pos < hole) | (pos >= hole + 10_000)]
    cls = codes[pos].copy()
    r = rng.random(len(pos))
    sub, dele = r < 0.006, (r >= 0.006) & (r < 0.010)
    cls[sub] = (cls[sub] + rng.integers(1, 4, int(sub.sum()))) % 4
    cls[dele] = C.LABEL_GAP
    ins = pos[(r >= 0.010) & (r < 0.014)]
    gap = pos[rng.random(len(pos)) < 0.05]
    slots = np.concatenate([pos * 4, ins * 4 + 1, gap * 4 + 2])
    preds = np.concatenate([cls, rng.integers(0, 4, len(ins)),
                            np.full(len(gap), C.LABEL_GAP)]).astype(np.uint8)
    positions = np.stack([slots // 4, slots % 4], axis=1).astype(np.int32)
    units = rng.integers(0, 256, (len(slots), C.NUM_CLASSES)).astype(np.uint8)
    dv = DeviceVotes({"c": n}, quality=True)
    for lo in range(0, len(slots), 1 << 20):  # bounded uploads
        hi = lo + (1 << 20)
        dv.scatter("c", preds[lo:hi], positions[lo:hi], units[lo:hi])
    return dv, draft


def measure(a):
    import torch

    from roko_amd.quality import stitch_dense_qual
    from roko_amd.stitch import is_default, stitch_filtered

    if not torch.cuda.is_available():
        sys.exit("stitch_timing needs a GPU")
    dv, draft = build(a.bases)
    filt = (a.min_qual, a.keep_uncovered)

    def host():
        maj, qual = dv.consensus_quality("c")
        out = stitch_dense_qual(draft, maj, qual) if is_default(*filt) \
            else stitch_filtered(draft, maj, qual, *filt)
        torch.cuda.synchronize()
        return out

    def device():
        out = dv.stitch("c", draft, *filt)
        torch.cuda.synchronize()
        return out

    want, got = host(), device()  # warm-up: code objects, allocator
    if want != got:
        sys.exit("the device stitch disagrees with the host stitch")
    times = {"host": [], "device": []}
    for _ in range(a.reps):
        for name, fn in (("host", host), ("device", device)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
    rec = {"bases": a.bases, "polished": len(got[0]), "reps": a.reps,
           "min_qual": a.min_qual, "keep_uncovered": a.keep_uncovered,
           "equal": True,
           "host_d2h_bytes": 2 * 4 * a.bases,
           "device_d2h_bytes": 24 + 2 * len(got[0]),
           "device_h2d_bytes": a.bases + 24}
    for name, ts in times.items():
        rec[name + "_ms"] = {"median": round(1e3 * statistics.median(ts), 3),
                             "min": round(1e3 * min(ts), 3),
                             "max": round(1e3 * max(ts), 3)}
        print(f"{name:6s} median {rec[name + '_ms']['median']:9.3f} ms  "
              f"min {rec[name + '_ms']['min']:9.3f}  "
              f"max {rec[name + '_ms']['max']:9.3f}", flush=True)
    print(f"bytes back: host {rec['host_d2h_bytes']}, device "
          f"{rec['device_d2h_bytes']} (+ {rec['device_h2d_bytes']} up)",
          flush=True)
    print(json.dumps(rec), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--bases", type=int, default=4_000_000)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--min-qual", type=int, default=0)
    p.add_argument("--keep-uncovered", action="store_true")
    p.add_argument("--limit", type=int, default=300,
                   help="time limit of the measurement, seconds")
    p.add_argument("--child", action="store_true",
                   help="(internal) measure in this process")
    a = p.parse_args()
    if a.child:
        measure(a)
        return
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable,
           os.path.abspath(__file__), "--child", "--bases", str(a.bases),
           "--reps", str(a.reps), "--min-qual", str(a.min_qual)]
    if a.keep_uncovered:
        cmd.append("--keep-uncovered")
    sys.exit(subprocess.call(cmd))


if __name__ == "__main__":
    main()
