"""Training rate of the train CLI's data routes on one RKW file.

  python scripts/train_data_bench.py [--windows N] [--val-windows N]
      [--b BATCH] [--epochs N] [--rounds N] [--limit SECONDS] [--dir DIR]
      [--routes a,b,...]

Writes a synthetic training file (16,384 random windows, ~296 MB) and a
2,048-window validation file, then runs roko_amd.train.train() for 2 epochs
at b=128 on

  file_t0   TrainDataset, DataLoader with no workers
  file_t8   TrainDataset, 8 DataLoader workers          (--t 8)
  memory    InMemoryTrainDataset                        (--memory)
  device    the sets resident in GPU memory             (--data device)

The three host routes run only code the device route leaves untouched, so
they are the baseline on the same input. --rounds N takes the routes in turn
N times (a, b, c, d, a, ...), so that drift of the machine hits all alike.

Each run is a fresh process under `timeout` (--limit seconds): one that hangs
or faults ends there and nothing is started after it. Each prints one JSON
line: the epoch-2 windows/s of the returned history (epoch 1 carries
warm-up), the seconds of the epoch-2 validation pass, and the load seconds —
from the call of train() to its "train path" log line, i.e. datasets or
resident sets built and the model on the device. A last line per route gives
the slowest, median and fastest epoch-2 rate over the rounds.
"""

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUTES = ("file_t0", "file_t8", "memory", "device")


def write_set(path, n, seed, group=1024):
    import numpy as np

    from roko_amd import config as C
    from roko_amd.rkdata import RkwWriter

    rng = np.random.default_rng(seed)
    with RkwWriter(path, inference=False) as w:
        for s in range(0, n, group):
            m = min(group, n - s)
            pos = np.zeros((m, C.WINDOW_COLS, 2), dtype=np.int32)
            pos[..., 0] = np.arange(C.WINDOW_COLS)[None, :]
            w.store("c1", 0, C.WINDOW_COLS, pos,
                    rng.integers(0, C.NUM_BASE_IDS,
                                 (m, C.WINDOW_ROWS, C.WINDOW_COLS),
                                 dtype=np.uint8),
                    rng.integers(0, C.NUM_CLASSES, (m, C.WINDOW_COLS),
                                 dtype=np.uint8))
        w.write_contigs([("c1", "A" * 200)])


def run_route(route, d, batch, epochs, rnd):
    """One route, in this (child) process; prints its JSON line."""
    import torch

    import roko_amd.ops.device_data as DD
    import roko_amd.train as T
    from roko_amd.config import TrainConfig

    val_s = []

    def timed(fn):
        def wrapper(*a, **k):
            torch.cuda.synchronize()
            t = time.time()
            r = fn(*a, **k)
            torch.cuda.synchronize()
            val_s.append(time.time() - t)
            return r
        return wrapper

    # train() looks both up at call time
    T.evaluate = timed(T.evaluate)
    DD.evaluate_device = timed(DD.evaluate_device)

    t0 = time.time()
    marks = {}
    lines = []

    def log(msg):
        lines.append(str(msg))
        if str(msg).startswith("train path"):
            marks["load_s"] = time.time() - t0

    cfg = TrainConfig(batch_size=batch, epochs=epochs, seed=1,
                      workers=8 if route == "file_t8" else 0,
                      in_memory=route == "memory",
                      data="device" if route == "device" else "host")
    out = tempfile.mkdtemp(prefix=f"ckpt_{route}_", dir=d)
    _, hist = T.train(os.path.join(d, "train.rkw"), out,
                      val_path=os.path.join(d, "val.rkw"), cfg=cfg, log=log)
    rec = {"route": route, "round": rnd, "batch": batch,
           "windows_per_sec": round(hist[-1]["windows_per_sec"], 1),
           "epoch1_windows_per_sec": round(hist[0]["windows_per_sec"], 1),
           "val_s": round(val_s[-1], 3),
           "load_s": round(marks.get("load_s", float("nan")), 3),
           "wall_s": round(time.time() - t0, 3),
           "val_acc": hist[-1]["val_acc"],
           "path": next((m for m in lines if m.startswith("train path")), "")}
    print(json.dumps(rec), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--windows", type=int, default=16_384)
    p.add_argument("--val-windows", type=int, default=2_048)
    p.add_argument("--b", type=int, default=128, help="batch size")
    p.add_argument("--epochs", type=int, default=2)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--limit", type=int, default=300,
                   help="time limit per run, seconds")
    p.add_argument("--dir", default=None, help="work directory")
    p.add_argument("--routes", default=",".join(ROUTES),
                   help="comma-separated routes to run, in this order")
    p.add_argument("--route", choices=ROUTES, default=None,
                   help="(internal) run one route in this process")
    p.add_argument("--round", type=int, default=0, help="(internal)")
    a = p.parse_args()
    if a.route:
        run_route(a.route, a.dir, a.b, a.epochs, a.round)
        return

    routes = [r for r in a.routes.split(",") if r]
    for r in routes:
        if r not in ROUTES:
            p.error(f"unknown route {r!r} (known: {', '.join(ROUTES)})")
    d = a.dir or tempfile.mkdtemp(prefix="train_data_bench_")
    os.makedirs(d, exist_ok=True)
    t0 = time.time()
    write_set(os.path.join(d, "train.rkw"), a.windows, seed=0)
    write_set(os.path.join(d, "val.rkw"), a.val_windows, seed=1)
    print(json.dumps({
        "step": "write_sets", "windows": a.windows,
        "val_windows": a.val_windows,
        "train_bytes": os.path.getsize(os.path.join(d, "train.rkw")),
        "wall_s": round(time.time() - t0, 1)}), flush=True)

    rates = {r: [] for r in routes}
    for rnd in range(1, max(a.rounds, 1) + 1):
        for route in routes:
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable,
                   os.path.abspath(__file__), "--route", route, "--dir", d,
                   "--b", str(a.b), "--epochs", str(a.epochs),
                   "--round", str(rnd)]
            res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            sys.stdout.write(res.stdout)
            sys.stdout.flush()
            if res.returncode != 0:
                print(json.dumps({"route": route, "round": rnd,
                                  "failed": res.returncode}), flush=True)
                sys.exit(res.returncode)  # start nothing more after a failure
            rec = json.loads(res.stdout.strip().splitlines()[-1])
            rates[route].append(rec["windows_per_sec"])
    for route in routes:
        v = rates[route]
        print(json.dumps({"route": route, "runs": len(v), "slowest": min(v),
                          "median": statistics.median(v),
                          "fastest": max(v)}), flush=True)


if __name__ == "__main__":
    main()
