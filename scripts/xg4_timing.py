"""Isolated timing of the serving xg projection, xg_gemm3 against every form
of xg_gemm4 (the persistent tile stream; for K=256 also the W-stationary
kernel), at the coalesced width (M = 90*1024) and the b=128 width (M = 90*128),
for both K families (layer 0: K=500 padded to 512; layers 1 and 2: K=256).
Uniform random operands; events on one stream; 20 warm-up launches, then the
kernels alternate in rounds inside one process. Each figure is the median
(and minimum) over rounds, and the per-round comparison against xg_gemm3 is
printed because "faster in every round" is the acceptance bar.

Also the target of the counter runs: `--pmc-only` launches each kernel three
times at M = 92,160 with no timing loop, so a `rocprofv3 --pmc FETCH_SIZE`
run of this script stays short (one derived counter per pass).

Usage (GPU): python scripts/xg4_timing.py [--rounds 7] [--iters 50] [--pmc-only]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import roko_amd  # noqa: F401  (env defaults)
from roko_amd.ops import _hip_ops as ext

# per K, at M = 92,160: (memory floor us at 6.3 TB/s of must-move bytes, MFMA
# floor us at 2.5 PF); scaled by M below
FLOORS = {512: (37.0, 29.0), 256: (30.0, 14.5)}


def operands(M, kreal, kp):
    Ap = torch.zeros(M, kp, dtype=torch.bfloat16, device="cuda")
    Ap[:, :kreal] = (torch.rand(M, kreal, device="cuda") * 2 - 1).bfloat16()
    Wp = torch.zeros(768, kp, dtype=torch.bfloat16, device="cuda")
    Wp[:, :kreal] = ((torch.rand(768, kreal, device="cuda") * 2 - 1)
                     * 0.05).bfloat16()
    bias = ((torch.rand(768, device="cuda") * 2 - 1) * 0.1).bfloat16()
    return Ap, Wp, bias


def timed(fn, iters):
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3  # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--pmc-only", action="store_true")
    args = ap.parse_args()

    torch.manual_seed(0)
    stream = torch.cuda.Stream()
    print(f"{ext.xg_gemm4_cus()} CUs", flush=True)
    with torch.cuda.stream(stream):
        for B in ((1024,) if args.pmc_only else (1024, 128)):
            M = 90 * B
            for kreal, kp, tag in [(500, 512, "l0"), (256, 256, "l1/l2")]:
                Ap, Wp, bias = operands(M, kreal, kp)
                names = ["xg_gemm3", "xg_gemm4 stream",
                         "xg_gemm4 stream 1 tile/wg"]
                if kp == 256:
                    names.append("xg_gemm4 wstat")
                outs = {k: torch.empty(M, 768, device="cuda",
                                       dtype=torch.bfloat16) for k in names}
                tiles = M // 128 * 6
                fns = {
                    "xg_gemm3": lambda: ext.xg_gemm3(
                        Ap, Wp, bias, out=outs["xg_gemm3"]),
                    "xg_gemm4 stream": lambda: ext.xg_gemm4(
                        Ap, Wp, bias, out=outs["xg_gemm4 stream"],
                        form="stream"),
                    # diagnostic: the grid uncapped, so every workgroup has
                    # one tile and no walk — the stream's code at
                    # xg_gemm3's structure
                    "xg_gemm4 stream 1 tile/wg": lambda: ext.xg_gemm4(
                        Ap, Wp, bias, out=outs["xg_gemm4 stream 1 tile/wg"],
                        max_wgs=tiles, form="stream"),
                }
                if kp == 256:
                    fns["xg_gemm4 wstat"] = lambda: ext.xg_gemm4(
                        Ap, Wp, bias, out=outs["xg_gemm4 wstat"], form="wstat")
                for fn in fns.values():
                    fn()
                torch.cuda.synchronize()
                for k in list(fns)[1:]:
                    print(f"M={M} {tag}: {k} == xg_gemm3 bitwise: "
                          f"{torch.equal(outs[k], outs['xg_gemm3'])}",
                          flush=True)
                if args.pmc_only:
                    for fn in fns.values():
                        for _ in range(3):
                            fn()
                    torch.cuda.synchronize()
                    continue
                for fn in fns.values():
                    for _ in range(20):
                        fn()
                torch.cuda.synchronize()
                times = {k: [] for k in fns}
                for _ in range(args.rounds):
                    for k, fn in fns.items():
                        times[k].append(timed(fn, args.iters))
                flops = 2 * M * 768 * kreal
                byt = M * kp * 2 + M * 768 * 2  # A once as stored + C once
                mem_floor, mfma_floor = (f * M / 92160 for f in FLOORS[kp])
                for k, ts in times.items():
                    med, mn = statistics.median(ts), min(ts)
                    print(f"M={M} {tag}: {k} median {med:.1f} us min "
                          f"{mn:.1f} us  ({flops / med / 1e6:.0f} TF/s, "
                          f"{byt / med / 1e6:.2f} TB/s of must-move bytes, "
                          f"{med / mem_floor:.2f}x memory floor, "
                          f"{med / mfma_floor:.2f}x MFMA floor)", flush=True)
                base = times["xg_gemm3"]
                for k in list(fns)[1:]:
                    wins = sum(t < b for t, b in zip(times[k], base))
                    print(f"M={M} {tag}: {k} vs xg_gemm3: "
                          f"{statistics.median(base) / statistics.median(times[k]):.3f}x"
                          f" (medians), faster in {wins} of {len(base)} rounds;"
                          f" rounds us: "
                          + " ".join(f"{b:.1f}/{t:.1f}"
                                     for t, b in zip(times[k], base)),
                          flush=True)


if __name__ == "__main__":
    main()
