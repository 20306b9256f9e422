"""Isolated timing of the serving xg projection kernels, xg_gemm2 against
xg_gemm3, at the b=128 width (M = 90*128) and the coalesced width
(M = 90*1024), for both K families (layer 0: K=500 padded to 512; layers 1
and 2: K=256). Uniform random operands; events on one stream after warm-up;
the two kernels alternate in rounds inside one process, and each figure is
the median (and minimum) over rounds.

Also the target of the counter runs: `--pmc-only` launches each kernel a
handful of times with no timing loop, so a `rocprofv3 --pmc FETCH_SIZE` run
of this script stays short (one derived counter per pass: FETCH_SIZE and
WRITE_SIZE together are rejected as exceeding what one pass can collect).

Usage (GPU): python scripts/xg3_timing.py [--rounds 7] [--iters 50] [--pmc-only]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import roko_amd  # noqa: F401  (env defaults)
from roko_amd.ops import _hip_ops as ext


def operands(M, kreal, kp):
    A = (torch.rand(M, kreal, device="cuda") * 2 - 1).bfloat16().contiguous()
    W = ((torch.rand(768, kreal, device="cuda") * 2 - 1) * 0.05).bfloat16()
    bias = ((torch.rand(768, device="cuda") * 2 - 1) * 0.1).bfloat16()
    Wp = torch.zeros(768, kp, dtype=torch.bfloat16, device="cuda")
    Wp[:, :kreal] = W
    Ap = torch.zeros(M, kp, dtype=torch.bfloat16, device="cuda")
    Ap[:, :kreal] = A
    return A, Ap, Wp.contiguous(), bias


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
    has3 = hasattr(ext, "xg_gemm3")

    torch.manual_seed(0)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        for B in (128, 1024):
            M = 90 * B
            for kreal, kp, tag in [(500, 512, "l0"), (256, 256, "l1/l2")]:
                A, Ap, Wp, bias = operands(M, kreal, kp)
                out2 = ext.xg_gemm2(A, Wp, bias)
                fns = {"xg_gemm2": lambda: ext.xg_gemm2(A, Wp, bias)}
                if has3:
                    out3 = torch.empty(M, 768, device="cuda",
                                       dtype=torch.bfloat16)
                    fns["xg_gemm3"] = lambda: ext.xg_gemm3(Ap, Wp, bias,
                                                           out=out3)
                    fns["xg_gemm3"]()
                    torch.cuda.synchronize()
                    print(f"M={M} {tag}: xg_gemm3 == xg_gemm2 bitwise: "
                          f"{torch.equal(out3, out2)}", flush=True)
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
                # bytes that must move: A once (as stored) + C once
                for k, ts in times.items():
                    a_bytes = M * (kreal if k == "xg_gemm2" else kp) * 2
                    byt = a_bytes + M * 768 * 2
                    med, mn = statistics.median(ts), min(ts)
                    print(f"M={M} {tag}: {k} median {med:.1f} us min "
                          f"{mn:.1f} us  ({flops / med / 1e6:.0f} TF/s, "
                          f"{byt / med / 1e6:.2f} TB/s of must-move bytes)",
                          flush=True)
                if has3:
                    print(f"M={M} {tag}: speedup (medians) "
                          f"{statistics.median(times['xg_gemm2']) / statistics.median(times['xg_gemm3']):.2f}x",
                          flush=True)


if __name__ == "__main__":
    main()
