"""A/B the wave-private eval fronts: v3 (one wave per SIMD) against v4
(persistent, three waves per SIMD), alternated in one process at B = 128 and
B = 1024. Events on one stream, 20 warm-up launches, 7 rounds x 50 launches
per kernel; prints each round, the median and the minimum (us per launch).
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from roko_amd import ops
from roko_amd.model import RokoModel
from roko_amd.ops import forward as fwd

ext = ops.ext()
torch.manual_seed(0)
m = RokoModel().cuda().eval()
w = fwd._bf16_weights(m)
ROUNDS, LAUNCHES, WARMUP = 7, 50, 20


def run(fn, x, out):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(
        enable_timing=True)
    a.record()
    for _ in range(LAUNCHES):
        fn(x, w["w1g"], w["b1"], w["w2"], w["b2"], w["emb"], None, 512, out)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / LAUNCHES


for B in (128, 1024):
    x = torch.randint(0, 12, (B, 200, 90), dtype=torch.uint8, device="cuda")
    o3 = torch.zeros(90, B, 512, dtype=torch.bfloat16, device="cuda")
    o4 = torch.zeros_like(o3)
    fns = {"v3": (ext.embed_mlp_fwd3, o3), "v4": (ext.embed_mlp_fwd4, o4)}
    for fn, o in fns.values():
        for _ in range(WARMUP):
            fn(x, w["w1g"], w["b1"], w["w2"], w["b2"], w["emb"], None, 512, o)
    torch.cuda.synchronize()
    print(f"B={B}: v4 == v3 bytes: {torch.equal(o3, o4)}")
    us = {"v3": [], "v4": []}
    for r in range(ROUNDS):
        for k, (fn, o) in fns.items():
            us[k].append(run(fn, x, o))
        print(f"  round {r}: v3 {us['v3'][-1]:7.1f} us   v4 {us['v4'][-1]:7.1f}"
              f" us   v3/v4 {us['v3'][-1] / us['v4'][-1]:.3f}")
    med = {k: statistics.median(v) for k, v in us.items()}
    print(f"  median v3 {med['v3']:.1f} v4 {med['v4']:.1f} us  ratio "
          f"{med['v3'] / med['v4']:.3f};  min v3 {min(us['v3']):.1f} "
          f"v4 {min(us['v4']):.1f} us;  v4 faster in every round: "
          f"{all(b < a for a, b in zip(us['v3'], us['v4']))}")
