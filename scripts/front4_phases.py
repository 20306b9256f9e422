"""Per-phase timing of the v4 eval front via its timing buffer: cycles that
lane 0 of wave 0 of every workgroup spends per phase, summed over the grid.
At B = 128 each workgroup has one window, and wave 0 walks 8 of its 90
columns. Companion of front3_phases.py (v3: wave 0 walks 23 columns)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from roko_amd import ops
from roko_amd.model import RokoModel
from roko_amd.ops import forward as fwd

ext = ops.ext()
torch.manual_seed(0)
m = RokoModel().cuda().eval()
w = fwd._bf16_weights(m)
B = 128
x = torch.randint(0, 12, (B, 200, 90), dtype=torch.uint8, device="cuda")
tim = torch.zeros(4, dtype=torch.int64, device="cuda")
iters = 30
for _ in range(3):
    ext.embed_mlp_fwd4(x, w["w1g"], w["b1"], w["w2"], w["b2"], w["emb"])
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(iters):
    ext.embed_mlp_fwd4(x, w["w1g"], w["b1"], w["w2"], w["b2"], w["emb"], tim)
torch.cuda.synchronize()
us = (time.perf_counter() - t0) / iters * 1e6
# s_memtime ticks per workgroup and launch (front3_phases.py prints the sum
# over the B workgroups: divide its figures by B to compare)
t = tim.cpu().numpy() / iters / B
names = ["scatter", "G1+handoff", "G2+G3", "store"]
tot = t.sum()
print(f"kernel {us:.1f} us (timed run incl. instrumentation)")
for n, v in zip(names, t):
    print(f"  {n:10s} {v:10.1f} ticks/wg  {100 * v / tot:5.1f}%   "
          f"{v / 8:8.2f} ticks/col")
