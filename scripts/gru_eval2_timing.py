"""A/B the eval GRU kernels: the LDS-staged 16-row kernel (impl=1) against the
transposed register-input kernel (impl=2), alternated in one process at
T = 90, B = 128 and B = 1024, random xg / U / bhh. Events on one stream, 20
warm-up launches, 7 rounds x 50 launches per kernel; prints each round, the
median and the minimum (us per launch). impl=3 (the hseq store variant that is
not shipped) and impl=4 (the new kernel with xg staged through LDS, the
fallback form) run in the same rounds. Then the probe masks of the new kernel
(1 no hseq store, 4 no gate VALU, 8 no xg loads, 16 no MFMA), and those of the
old kernel for comparison.
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from roko_amd import ops

ext = ops.ext()
torch.manual_seed(0)
T = 90
ROUNDS, LAUNCHES, WARMUP = 7, 50, 20
NAMES = {1: "old", 2: "new", 3: "new/alt-store", 4: "new/staged"}
PROBES = ((0, "full"), (1, "no hseq store"), (4, "no gate VALU"),
          (8, "no xg loads/staging"), (16, "no MFMA"))


def run(xg, u, bhh, out, impl, dbg=0):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(
        enable_timing=True)
    a.record()
    for _ in range(LAUNCHES):
        ext.gru_layer_fwd(xg, u, bhh, False, dbg, impl=impl, out=out)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / LAUNCHES


for B in (128, 1024):
    xg = (torch.randn(T, B, 2, 384, device="cuda") * 0.3).to(torch.bfloat16)
    u = (torch.randn(2, 384, 128, device="cuda") * 0.2).to(torch.bfloat16)
    bhh = torch.randn(2, 384, device="cuda")
    outs = {k: torch.zeros(T, B, 2, 128, dtype=torch.bfloat16, device="cuda")
            for k in NAMES}
    for k in NAMES:
        for _ in range(WARMUP):
            ext.gru_layer_fwd(xg, u, bhh, False, 0, impl=k, out=outs[k])
    torch.cuda.synchronize()
    print(f"B={B}: bytes equal to old: " + ", ".join(
        f"{NAMES[k]} {torch.equal(outs[1], outs[k])}" for k in (2, 3, 4)))
    us = {k: [] for k in NAMES}
    for r in range(ROUNDS):
        for k in NAMES:
            us[k].append(run(xg, u, bhh, outs[k], k))
        print(f"  round {r}: " + "   ".join(
            f"{NAMES[k]} {us[k][-1]:7.1f} us" for k in NAMES)
            + f"   old/new {us[1][-1] / us[2][-1]:.3f}")
    for k in NAMES:
        print(f"  {NAMES[k]:14s} median {statistics.median(us[k]):7.1f}  "
              f"min {min(us[k]):7.1f} us")
    print(f"  new faster than old in every round: "
          f"{all(n < o for o, n in zip(us[1], us[2]))}")
    for impl in (2, 1):
        print(f"  probes, {NAMES[impl]} kernel (median / min us, "
              f"ns per step):")
        for dbg, label in PROBES:
            for _ in range(WARMUP):
                ext.gru_layer_fwd(xg, u, bhh, False, dbg, impl=impl,
                                  out=outs[impl])
            v = [run(xg, u, bhh, outs[impl], impl, dbg) for _ in range(3)]
            med = statistics.median(v)
            print(f"    {label:22s} {med:7.1f} / {min(v):7.1f}   "
                  f"{med / T * 1e3:6.0f}")
