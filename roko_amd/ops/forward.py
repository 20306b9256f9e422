"""Full-model GPU forward through the hand-written gfx950 kernels.

Orchestration: the fused embed+MLP kernel produces the GRU
input sequence; per layer, the input projections of BOTH directions and all
90 steps are ONE hipBLASLt GEMM (plain GEMM -> library; the brief's rule) and
the recurrence is one persistent kernel launch; the 5-class head is a fused
GEMV(+argmax) kernel. No per-step launches, no MIOpen RNN, no eager fallback.
"""

from __future__ import annotations

import os

import torch

from .. import config as C

#: eval front kernel: the one-hot embed+MLP (factors the read reduction
#: through the 12 base classes — ~2.3x fewer MFMAs per column) does ~1.45x
#: less chip-work than the shared train-front kernel; v3 (wave-private
#: columns, no per-phase barriers) is the measured-fastest default
#: (106.7 us vs v2's 152.4 at b=128). v4 is v3's arithmetic, byte for byte,
#: on a persistent grid at three waves per SIMD with W1 in LDS and the
#: G1->G2->G3 hand-offs in registers. ROKO_FRONT=v4/v3/v2/v1/shared for A/B.
_FRONT = os.environ.get("ROKO_FRONT", "v4")


def _front_eval(ext, ids, w):
    if _FRONT == "shared":
        return ext.front_fwd(ids, w["w1"], w["b1"], w["w2"], w["b2"],
                             w["emb"], 0, 1.0)
    if _FRONT == "v1":
        return ext.embed_mlp_fwd(ids, w["w1"], w["b1"], w["w2"], w["b2"],
                                 w["emb"])
    if _FRONT == "v4":
        return ext.embed_mlp_fwd4(ids, w["w1g"], w["b1"], w["w2"], w["b2"],
                                  w["emb"])
    if _FRONT == "v3":
        return ext.embed_mlp_fwd3(ids, w["w1g"], w["b1"], w["w2"], w["b2"],
                                  w["emb"])
    return ext.embed_mlp_fwd2(ids, w["w1g"], w["b1"], w["w2"], w["b2"],
                              w["emb"])


def _ext():
    from . import ext

    return ext()


def _bf16_weights(model) -> dict:
    """Per-model cache of bf16/fp32 kernel-ready weight tensors."""
    params = [
        model.embedding.weight, model.fc1.weight, model.fc1.bias,
        model.fc2.weight, model.fc2.bias, model.fc4.weight, model.fc4.bias,
    ]
    for l in range(C.NUM_LAYERS):
        for suffix in ("", "_reverse"):
            for kind in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                params.append(getattr(model.gru, f"{kind}_l{l}{suffix}"))
    ver = tuple(p._version for p in params) + (params[0].device,)
    cache = getattr(model, "_hip_weight_cache", None)
    if cache is not None and cache["ver"] == ver:
        return cache

    g = model.gru
    c = {"ver": ver}
    c["w1"] = model.fc1.weight.detach().to(torch.bfloat16).contiguous()
    # (112, 232) zero-padded W1 for the chunked v2 front (L2-resident A tile)
    w1g = torch.zeros(112, 232, dtype=torch.bfloat16,
                      device=model.fc1.weight.device)
    w1g[:100, :200] = c["w1"]
    c["w1g"] = w1g
    c["b1"] = model.fc1.bias.detach().float().contiguous()
    c["w2"] = model.fc2.weight.detach().to(torch.bfloat16).contiguous()
    c["b2"] = model.fc2.bias.detach().float().contiguous()
    c["emb"] = model.embedding.weight.detach().to(torch.bfloat16).contiguous()
    c["w4"] = model.fc4.weight.detach().to(torch.bfloat16).contiguous()
    c["b4"] = model.fc4.bias.detach().float().contiguous()
    for l in range(C.NUM_LAYERS):
        wf = getattr(g, f"weight_ih_l{l}").detach()
        wr = getattr(g, f"weight_ih_l{l}_reverse").detach()
        bf = getattr(g, f"bias_ih_l{l}").detach()
        br = getattr(g, f"bias_ih_l{l}_reverse").detach()
        # (in, 768) so xg = x @ w_ih_t is one GEMM covering both directions
        w_cat = torch.cat([wf, wr], dim=0).to(torch.bfloat16)
        c[f"w_ih_t{l}"] = w_cat.t().contiguous()
        # (768, KP) row-padded copy for the in-kernel xg GEMM (KP multiple of
        # 32 and 16-byte-aligned rows; zero pad cols are multiplied by the
        # zero-padded x stage)
        kin = w_cat.shape[1]
        kp = 512 if kin > 256 else 256
        wp = torch.zeros(768, kp, dtype=torch.bfloat16, device=w_cat.device)
        wp[:, :kin] = w_cat
        c[f"w_ih_p{l}"] = wp.contiguous()
        c[f"b_ih{l}"] = torch.cat([bf, br]).to(torch.bfloat16).contiguous()
        c[f"u{l}"] = torch.stack(
            [getattr(g, f"weight_hh_l{l}").detach(),
             getattr(g, f"weight_hh_l{l}_reverse").detach()]
        ).to(torch.bfloat16).contiguous()
        c[f"bhh{l}"] = torch.stack(
            [getattr(g, f"bias_hh_l{l}").detach(),
             getattr(g, f"bias_hh_l{l}_reverse").detach()]
        ).float().contiguous()
    model._hip_weight_cache = c
    return c


def _pad32(x: torch.Tensor) -> torch.Tensor:
    """ids as contiguous uint8, zero rows appended up to a multiple of 32."""
    ids = x.to(torch.uint8).contiguous()
    pad = (-ids.shape[0]) % 32
    if pad:
        ids = torch.cat([ids, ids.new_zeros(pad, *ids.shape[1:])])
    return ids


def _forward(model, ids: torch.Tensor, logits: bool) -> torch.Tensor:
    """front -> 3 x (addmm + GRU) -> head on padded ids (B % 32 == 0):
    logits (B, 90, 5) fp32, or the fused argmax (B, 90) uint8."""
    ext = _ext()
    w = _bf16_weights(model)
    B = ids.shape[0]
    T = C.WINDOW_COLS
    seq = _front_eval(ext, ids, w)
    for l in range(C.NUM_LAYERS):
        xg = torch.addmm(
            w[f"b_ih{l}"], seq.reshape(T * B, -1), w[f"w_ih_t{l}"]
        ).view(T, B, 2, 384)
        (hseq,) = ext.gru_layer_fwd(xg.contiguous(), w[f"u{l}"], w[f"bhh{l}"], False)
        seq = hseq.view(T, B, 2 * C.HIDDEN_SIZE)
    (out,) = ext.head_fwd(seq, w["w4"], w["b4"], logits, not logits)
    return out


def roko_forward(model, x: torch.Tensor) -> torch.Tensor:
    """ids (B, 200, 90) int/uint8 on GPU -> logits (B, 90, 5) fp32."""
    return _forward(model, _pad32(x), True)[: x.shape[0]]


def roko_argmax(model, x: torch.Tensor) -> torch.Tensor:
    """ids -> per-position class predictions (B, 90) uint8, argmax fused."""
    return _forward(model, _pad32(x), False)[: x.shape[0]]


#: shipped coalescing request (ROKO_COALESCE overrides): consecutive
#: submits that share one wide slot. Chosen by the sweep recorded in
#: profiles/PERF_HISTORY.md ("Cross-batch coalescing").
_COALESCE_DEFAULT = 8


def coalesce_width(request: int, depth: int) -> int:
    """Effective coalescing factor G: the largest power of two that is
    <= `request` and divides `depth` (at least 1)."""
    g = 1
    while g * 2 <= request and depth % (g * 2) == 0:
        g *= 2
    return g


class InferencePipeline:
    """Serving-style pipelined inference on one GPU.

    The GRU recurrence is latency-bound: at b=128 one forward occupies only
    8 workgroups of the 256 CUs (profiles/ kernel stats — gru_layer_fwd
    dominates chain time at ~3% chip occupancy). Independent batches
    therefore overlap, so the engine keeps `depth` in-flight batches on
    per-slot HIP streams. Each slot's whole forward (front kernel -> 3x
    (xg GEMM + persistent GRU kernel) -> fused head+argmax -> pinned D2H)
    is enqueued by ONE C++ call (`ext.ServeSlot.submit`); for batches
    >= 256 the slot auto-captures its kernel sequence into a RAW hipGraph
    (BASELINE.json config 4's "hipGraph-captured GRU steps") — a measured
    win at large batch and a measured loss at b=128, both A/B'd
    (profiles/PERF_HISTORY.md; ROKO_GSLOT overrides). What a slot chose to
    launch is its `cpp.plan`.

    Every submitted batch runs the full model; nothing is cached or skipped
    — pipelining only overlaps independent batches, as a serving deployment
    would.

    Coalescing: a narrow batch launches narrow grids (the GRU runs
    batch/16 x 2 workgroups on 256 CUs), so G consecutive submits share one
    slot of width G*batch. Each submit still copies its input at once (the
    caller's tensor is free when submit() returns); the submit that fills
    the slot enqueues the model ONCE at full width plus one D2H. G is
    `coalesce_width(coalesce, depth)`: `coalesce=None` reads ROKO_COALESCE,
    else the shipped default; depth 1 or 3 gives G=1, which is exactly the
    uncoalesced path. There are depth/G slots, so slot memory and the
    `depth`-submissions validity of copy_out=False predictions are
    unchanged. Nothing is launched by a timer or a thread: a ticket,
    drain() and slot reuse flush a partly filled slot first (the model runs
    at full width over stale rows whose predictions nobody reads, and runs
    again when the remaining parts arrive), so no caller waits on work that
    was never enqueued. A caller that only synchronizes the device — as
    bench.py does after 32 submits per step — sees every batch complete as
    long as the number of submits is a multiple of G; any power of two
    <= 32 keeps that true for the benchmark. Votes mode needs G=1.
    """

    def __init__(self, model, batch: int, depth: int = 4, coalesce=None,
                 quality: bool = False):
        from . import require

        require()
        self.batch = batch
        self.depth = depth
        self.model = model
        self.w = _bf16_weights(model)
        # quality=True: the slots' head kernel also writes five quality
        # units per column (roko_amd/quality.py) for the votes mode; fixed
        # at construction, and off it leaves the slots exactly as they were
        self.quality = bool(quality)
        dev = next(model.parameters()).device
        if coalesce is None:
            coalesce = int(os.environ.get("ROKO_COALESCE", _COALESCE_DEFAULT))
        self.coalesce = coalesce_width(coalesce, depth)
        self.slots = []
        for _ in range(depth // self.coalesce):
            self.slots.append(_Slot(self, batch, dev, self.coalesce))
        self._next = 0

    def _place(self):
        """(slot, part) of the next submission k: group (k // G) % (depth //
        G), part k % G."""
        k, g = self._next, self.coalesce
        return self.slots[(k // g) % len(self.slots)], k % g

    def unlaunched(self) -> int:
        """Submitted batches whose model launch is still deferred."""
        return sum(s.cpp.unlaunched() for s in self.slots)

    def submit(self, x: torch.Tensor, copy_out: bool = True):
        """Enqueue one batch (device or host tensor, (<=batch, R, W) int).
        Returns a ticket; call ticket() to wait and get predictions
        (n, W) uint8 on pinned host memory (a view — copy before the slot
        is reused `depth` submissions later, or pass copy_out=True)."""
        slot, part = self._place()
        self._next += 1
        return slot.submit(x, copy_out, part)

    # -- votes mode: predictions stay on the GPU and vote into a device table
    # (ops/votes.py DeviceVotes drives these three) -------------------------
    def votes_staging(self):
        """Pinned staging of the slot the next submit_votes() uses, as numpy
        views x (batch, R, W) u8 and pos (batch, W, 2) i32. The slot is
        synced first: its previous submit read this staging asynchronously."""
        self._need_uncoalesced()
        return self.slots[self._next % self.depth].votes_staging()

    def submit_votes(self, n: int, table: torch.Tensor, n_slots: int,
                     err_flag: torch.Tensor, qsum=None) -> None:
        """Enqueue rows 0..n of the current staging: H2D, model, and one vote
        per column into `table` (and its quality units into `qsum`, on a
        quality pipeline). No predictions come back."""
        self._need_uncoalesced()
        slot = self.slots[self._next % self.depth]
        self._next += 1
        slot.submit_votes(n, table, n_slots, err_flag, qsum)

    def submit_votes_device(self, x: torch.Tensor, pos: torch.Tensor, n: int,
                            table: torch.Tensor, n_slots: int,
                            err_flag: torch.Tensor, qsum=None) -> None:
        """submit_votes() for windows that are already in device memory
        (ops/windows.py): x (>=n, R, W) u8 and pos (>=n, W, 2) i32 on the
        GPU, n <= batch. The slot copies them device to device on its own
        stream, ordered behind the current stream, and keeps their memory
        alive until the copy has run; no staging is involved."""
        self._need_uncoalesced()
        if not (x.is_cuda and pos.is_cuda):
            raise ValueError("submit_votes_device takes device tensors; use "
                             "votes_staging() + submit_votes() for host data")
        if not 0 <= n <= min(self.batch, x.shape[0], pos.shape[0]):
            raise ValueError(f"n={n} outside [0, min(batch, rows given)]")
        slot = self.slots[self._next % self.depth]
        self._next += 1
        slot.submit_votes_device(x, pos, n, table, n_slots, err_flag, qsum)

    def _need_uncoalesced(self):
        if self.coalesce != 1:
            raise RuntimeError(
                "votes mode needs an uncoalesced pipeline: construct it with "
                f"coalesce=1 (this one coalesces {self.coalesce} submits)")

    def drain(self) -> None:
        """Launch what is still deferred and wait for every slot; after this
        all submitted batches and votes are in."""
        for slot in self.slots:
            slot.flush()
        for slot in self.slots:
            slot.wait_done()


class _Ticket:
    """Handle for one submitted batch; call it to wait and get the (n, W)
    uint8 predictions. Snapshotted automatically when its slot is reused.
    `need` is the ordinal of the slot launch that covers the submission (0:
    it was launched by its own submit); the slot is flushed first if that
    launch has not happened."""

    def __init__(self, slot: "_Slot", n: int, part: int = 0, need: int = 0):
        self.slot = slot
        self.n = n
        self.row0 = part * slot.bp
        self.need = need
        self.data = None

    def materialize(self):
        if self.data is None:
            if self.slot.launches < self.need:
                self.slot.flush()
            self.slot.wait_done()
            self.data = self.slot.host_out[
                self.row0 : self.row0 + self.n].clone()

    def __call__(self) -> torch.Tensor:
        self.materialize()
        return self.data


class _Slot:
    """One pipeline slot: an `ext.ServeSlot` owns the slot stream and
    enqueues the whole forward (input copy, front kernel, 3x xg GEMM + GRU,
    fused head+argmax, pinned D2H) in ONE pybind call. The server is
    host-bound (a torch hipGraph replay costs ~51 us + ~15 us/node of host
    time on ROCm and threads don't scale: runtime-global enqueue lock), so
    per-batch Python work IS the throughput limit
    (profiles/PERF_HISTORY.md)."""

    def __init__(self, pipe: "InferencePipeline", batch: int, dev,
                 parts: int = 1):
        # `parts` consecutive submissions of `batch` rows share this slot;
        # the slot is `parts * batch` rows wide
        self.pipe = pipe
        self.bp = batch
        self.parts = parts
        self.pending = [None] * parts
        self.launches = 0  # model launches of this slot so far
        batch = batch * parts
        self.host_out = torch.empty(
            (batch, C.WINDOW_COLS), dtype=torch.uint8, pin_memory=True
        )
        self.cpp = _ext().ServeSlot(pipe.w, batch, self.host_out, parts,
                                    pipe.quality)
        # one warm-up pass primes the hipBLASLt workspace/algo cache for
        # the slot stream so submit() never allocates
        warm = torch.zeros((batch, C.WINDOW_ROWS, C.WINDOW_COLS),
                           dtype=torch.uint8, device=dev)
        self.cpp.run(warm, batch)
        self.cpp.sync()

    def wait_done(self):
        self.cpp.sync()

    def unlaunched(self) -> int:
        return self.cpp.unlaunched() if self.parts > 1 else 0

    def flush(self):
        """Launch the model for the parts received so far, if any."""
        if self.parts > 1 and self.cpp.flush():
            self.launches += 1

    def votes_staging(self):
        if self.pending[0] is not None:
            self.pending[0].materialize()
            self.pending[0] = None
        self.wait_done()
        if getattr(self, "x_stage", None) is None:
            b = self.host_out.shape[0]
            self.x_stage = torch.zeros(
                (b, C.WINDOW_ROWS, C.WINDOW_COLS), dtype=torch.uint8,
                pin_memory=True)
            self.pos_stage = torch.zeros(
                (b, C.WINDOW_COLS, 2), dtype=torch.int32, pin_memory=True)
        return self.x_stage.numpy(), self.pos_stage.numpy()

    def submit_votes(self, n: int, table, n_slots: int, err_flag,
                     qsum=None):
        if getattr(self, "x_stage", None) is None:
            raise RuntimeError("call votes_staging() and fill it first")
        self.cpp.submit_votes(self.x_stage, self.pos_stage, n, table,
                              n_slots, err_flag, qsum)

    def submit_votes_device(self, x, pos, n: int, table, n_slots: int,
                            err_flag, qsum=None):
        if x.dtype != torch.uint8 or pos.dtype != torch.int32:
            raise ValueError("x must be uint8 and pos int32")
        if self.pending[0] is not None:
            self.pending[0].materialize()
            self.pending[0] = None
        # the same back-pressure as the staging route: at most `depth`
        # batches (and the window tensors they pin) are in flight
        self.wait_done()
        self.cpp.submit_votes(x.contiguous(), pos.contiguous(), n, table,
                              n_slots, err_flag, qsum)

    def submit(self, x: torch.Tensor, copy_out: bool, part: int = 0):
        n = x.shape[0]
        # preserve the previous tenant's predictions before the slot buffers
        # are overwritten (its ticket may be called arbitrarily late)
        if self.pending[part] is not None:
            self.pending[part].materialize()
            self.pending[part] = None
        if x.dtype != torch.uint8:
            x = x.to(torch.uint8)
        if self.parts > 1:
            # coalesced: the input copy is enqueued now; the model is
            # enqueued by the submit that fills the slot
            t = _Ticket(self, n, part, need=self.launches + 1)
            if self.cpp.submit_part(
                    x if x.is_contiguous() else x.contiguous(), n, part):
                self.launches += 1
            if copy_out:
                self.pending[part] = t
            return t
        # ONE C++ call enqueues the whole forward (GIL released). No event
        # sync in the hot path: stream ordering makes buffer reuse safe,
        # tickets sync in materialize(), and hipEventSynchronize itself
        # measured ~80 us with ~32 live streams (profiles/PERF_HISTORY.md)
        self.cpp.submit(x if x.is_contiguous() else x.contiguous(), n)
        t = _Ticket(self, n)
        if copy_out:
            self.pending[0] = t
        return t
