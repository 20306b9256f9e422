"""Where a workgroup of xg_gemm3 spends its time: the phase stamps of the
timing-only instantiation (`ext.xg_gemm3_phases`; the production kernel holds
no stamp), at M = 92,160 for K = 256 and K = 512.

Lane 0 of wave 0 of every workgroup records the shader clock (s_memtime) at
entry, after the prologue's barrier, after each k-slice's barrier and after
the last store is issued, plus the wall clock (s_memrealtime) at entry and
exit and the CU it ran on. From these:

  prologue  entry -> first barrier (two slices issued, one waited for,
            committed)
  slice k   barrier to barrier
  epilogue  last slice's barrier -> last store issued
  gap       per CU: a workgroup's start minus the latest end on that CU that
            precedes it (the slot it took over), wall clock converted to
            shader-clock ticks with the ratio the stamps themselves give

The stamped build fences every stamp, so it forbids overlaps the real kernel
has: read the SHARES, not the length.

Usage (GPU): python scripts/xg4_phases.py [--save stamps.npz]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import roko_amd  # noqa: F401  (env defaults)
from roko_amd.ops import _hip_ops as ext


def q(x):
    return (f"{np.median(x):8.0f} {np.percentile(x, 10):8.0f} "
            f"{np.percentile(x, 90):8.0f}")


def analyse(st, KB, tag):
    st = st.astype(np.int64)
    pro = st[:, 1] - st[:, 0]
    sl = [st[:, 2 + k] - st[:, 1 + k] for k in range(KB)]
    epi = st[:, 10] - st[:, 1 + KB]
    tot = st[:, 10] - st[:, 0]
    rt0, rt1 = st[:, 11], st[:, 12]
    # shader-clock ticks per wall-clock tick, from the workgroups themselves
    ratio = float(np.sum(tot)) / max(float(np.sum(rt1 - rt0)), 1.0)
    place = st[:, 13]
    cu = ((place >> 32) << 8) | ((place >> 8) & 0xFF)  # XCC, SE/SH/CU bits
    gaps = []
    per_cu = []
    for c in np.unique(cu):
        idx = np.where(cu == c)[0]
        per_cu.append(len(idx))
        ends = np.sort(rt1[idx])
        for s in np.sort(rt0[idx]):
            k = np.searchsorted(ends, s, side="right")
            if k > 0:
                gaps.append((s - ends[k - 1]) * ratio)
    gaps = np.array(gaps) if gaps else np.zeros(1)
    span = (rt1.max() - rt0.min()) * ratio
    print(f"== {tag}: {st.shape[0]} workgroups on {len(per_cu)} CUs "
          f"({np.mean(per_cu):.1f} per CU), {ratio:.2f} shader-clock ticks per "
          f"wall-clock tick, kernel span {span:.0f} ticks")
    print(f"{'phase':<12} {'median':>8} {'p10':>8} {'p90':>8}  share of tile")
    med_tot = np.median(tot)
    rows = [("prologue", pro)] + [(f"slice {k}", s) for k, s in enumerate(sl)]
    rows += [("epilogue", epi), ("tile total", tot), ("gap", gaps)]
    for name, x in rows:
        print(f"{name:<12} {q(x)}  {np.median(x) / med_tot * 100:5.1f}%")
    kloop = np.sum(sl, axis=0)
    print(f"k-loop {np.median(kloop):.0f} ({np.median(kloop) / med_tot * 100:.1f}%), "
          f"of it slice 0 {np.median(sl[0]):.0f}; per-slot occupancy: tile total x "
          f"rounds = {med_tot * st.shape[0] / (2 * len(per_cu)):.0f} of span {span:.0f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--save", default="")
    args = ap.parse_args()
    torch.manual_seed(0)
    M = 92160
    saved = {}
    for kreal, kp in [(256, 256), (500, 512)]:
        A = torch.zeros(M, kp, dtype=torch.bfloat16, device="cuda")
        A[:, :kreal] = (torch.rand(M, kreal, device="cuda") * 2 - 1).bfloat16()
        W = torch.zeros(768, kp, dtype=torch.bfloat16, device="cuda")
        W[:, :kreal] = ((torch.rand(768, kreal, device="cuda") * 2 - 1)
                        * 0.05).bfloat16()
        bias = ((torch.rand(768, device="cuda") * 2 - 1) * 0.1).bfloat16()
        ref = ext.xg_gemm3(A, W, bias)
        for _ in range(10):
            out, stamps = ext.xg_gemm3_phases(A, W, bias)
        torch.cuda.synchronize()
        assert torch.equal(out, ref), "the stamped build changed the output"
        st = stamps.cpu().numpy()
        saved[f"k{kp}"] = st
        analyse(st, kp // 64, f"xg_gemm3 stamped, M={M} K={kp}")
    if args.save:
        np.savez_compressed(args.save, **saved)


if __name__ == "__main__":
    main()
