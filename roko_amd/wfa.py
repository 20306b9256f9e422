"""Exact unit-cost global alignment by diagonal transition (wavefront, WFA).

This module is the contract (numpy / pure Python, no GPU) of the genome-scale
scorer behind `accuracy.seq_stats(aligner="wfa")`: the definition, a slow
reference (`reference_ops`, `replay`), the chunk schedule and table sizes the
device driver follows, and the public entry `align`. The C++ route
(`_pileup.wfa_ops`, ops/cpp/wfa.cpp) and the device route (ops/hip/wfa.hip)
compute the same op string byte for byte; tests compare the three.

Definitions. Query `q` of length n (the assembly), target `t` of length m (the
truth), diagonal k = j - i. F[s][k] is the furthest target offset j reachable
on diagonal k with exactly s edits; absent entries are -inf. ext(i, j) advances
both indices while i < n, j < m and q[i] == t[j] (raw bytes, as `align_stats`
compares them). F[0][0] = ext(0, 0).

Score step, for s >= 1 and k in [max(-s, -n), min(s, m)]: the candidates, in
this order of preference on equal offset, are

  X  mismatch                                  F[s-1][k] + 1    valid if <= m
                                                                and i <= n
  D  truth base missing from the query (j+1)   F[s-1][k-1] + 1  valid if <= m
  I  extra query base (i+1)                    F[s-1][k+1]      valid if
                                                                j - k <= n

The largest valid candidate wins; a later kind replaces an earlier one only if
its offset is strictly greater. The winner is extended and its kind recorded
in dir[s][k]. The first s with F[s][m-n] == m is the edit distance S.

Traceback starts at k = m - n and for s = S..1 emits dir[s][k] and moves k by
0, -1, +1 for X, D, I. The result is the op string: S bytes over {X, D, I} in
forward order. The tie rule is part of the contract because co-optimal
alignments differ in their breakdown ("AC" vs "CA" is "XX" here).

Replay (`replay`, `_pileup.replay_ops`) turns an op string back into an
alignment: start at (0, 0), extend greedily, and for each op check that it is
legal (X: i < n, j < m, q[i] != t[j]; D: j < m; I: i < n), apply it, extend.
After the last op the position must be exactly (n, m). Replay is O(n + S),
yields the counts and the M/I/D CIGAR in the `align_cigar` convention, and is
the self-check of every route: an op string that does not replay raises and is
never turned into statistics. I counts as an insertion and D as a deletion in
the sense `align_stats` uses; mismatches = #X, matches = n - #X - #I.
"""

from __future__ import annotations

from typing import Dict, Iterator, List, Optional, Tuple, Union

import numpy as np

#: bytes a lane of the step kernel compares alone before the wave helps
PROBE = 8
#: bytes one round of the wave-cooperative extension compares
COOP = 256
#: bytes after each sequence on the device (>= the widest cooperative read)
PAD = COOP
#: pad bytes: distinct, and outside printable ASCII, so they occur in no input
QUERY_PAD, TARGET_PAD = 0x00, 0x01
#: the -inf of the device offset buffers
NEG = -(1 << 30)

CHUNK_FIRST = 64
CHUNK_CAP = 4096
#: share of the free device memory the direction tables may take by default
BUDGET_SHARE = 0.5
#: `align(device=None)` on a GPU host: the C++ route runs first, bounded to
#: distances below this; only a pair beyond it goes to the device. The C++
#: route costs ~2.6 ns * S^2 and the device route ~5 us * S (one launch per
#: score), which cross near S = 2,000 (profiles/PERF_HISTORY.md, "Exact
#: aligner"); a bounded first pass that fails costs about 11 ms.
DEVICE_MIN_SCORE = 2048

Seq = Union[str, bytes, bytearray]


class BudgetError(RuntimeError):
    """The direction tables would exceed the byte budget."""


class ScoreLimitError(RuntimeError):
    """The edit distance exceeds `max_score`."""


def as_bytes(seq: Seq, name: str = "sequence") -> bytes:
    """`seq` as bytes; ValueError unless every byte is printable ASCII
    (0x20..0x7E), which keeps the device pad bytes out of the input."""
    if isinstance(seq, str):
        try:
            b = seq.encode("ascii")
        except UnicodeEncodeError:
            raise ValueError(f"{name} holds a non-ASCII character") from None
    else:
        b = bytes(seq)
    if b:
        a = np.frombuffer(b, dtype=np.uint8)
        if int(a.min()) < 0x20 or int(a.max()) > 0x7E:
            raise ValueError(f"{name} holds a byte outside printable ASCII")
    return b


# ---------------------------------------------------------------------------
# schedule and sizes

def chunk_bounds(limit: Optional[int] = None) -> Iterator[int]:
    """Exclusive upper score bounds of the driver's chunks: the first chunk
    holds scores 0..63, each later one twice as many up to CHUNK_CAP. Endless
    without `limit`; with it, stops after the first bound > limit."""
    size, end = CHUNK_FIRST, 0
    while True:
        end += size
        yield end
        if limit is not None and end > limit:
            return
        size = min(2 * size, CHUNK_CAP)


def _sum_min(s: int, a: int) -> int:
    """sum of min(r, a) over r in [0, s)."""
    if s <= 0:
        return 0
    if s - 1 <= a:
        return s * (s - 1) // 2
    return a * (a + 1) // 2 + (s - 1 - a) * a


def dir_cells(n: int, m: int, s0: int, s1: int) -> int:
    """Entries of the direction table of scores [s0, s1): the sum of
    min(s, m) + min(s, n) + 1 over them."""
    if s1 <= s0:
        return 0
    return (_sum_min(s1, m) - _sum_min(s0, m) + _sum_min(s1, n)
            - _sum_min(s0, n) + (s1 - s0))


# ---------------------------------------------------------------------------
# slow reference

def _ext(q: bytes, t: bytes, i: int, j: int) -> int:
    n, m = len(q), len(t)
    while i < n and j < m and q[i] == t[j]:
        i += 1
        j += 1
    return j


def reference_ops(query: Seq, target: Seq,
                  max_score: Optional[int] = None) -> bytes:
    """The op string by the definition above, one diagonal at a time."""
    q, t = as_bytes(query, "query"), as_bytes(target, "target")
    n, m = len(q), len(t)
    prev: Dict[int, int] = {0: _ext(q, t, 0, 0)}
    dirs: List[Dict[int, str]] = [{}]
    s = 0
    while prev.get(m - n) != m:
        s += 1
        if max_score is not None and s > max_score:
            raise ScoreLimitError(f"edit distance exceeds max_score "
                                  f"{max_score}")
        cur: Dict[int, int] = {}
        d: Dict[int, str] = {}
        for k in range(max(-s, -n), min(s, m) + 1):
            best, kind = None, ""
            fx, fd, fi = prev.get(k), prev.get(k - 1), prev.get(k + 1)
            if fx is not None and fx + 1 <= m and fx + 1 - k <= n:
                best, kind = fx + 1, "X"
            if fd is not None and fd + 1 <= m and (best is None
                                                   or fd + 1 > best):
                best, kind = fd + 1, "D"
            if fi is not None and fi - k <= n and (best is None or fi > best):
                best, kind = fi, "I"
            if best is not None:
                cur[k] = _ext(q, t, best - k, best)
                d[k] = kind
        dirs.append(d)
        prev = cur
    ops = []
    k = m - n
    for r in range(s, 0, -1):
        kind = dirs[r][k]
        ops.append(kind)
        k += {"X": 0, "D": -1, "I": 1}[kind]
    return "".join(reversed(ops)).encode("ascii")


def replay(query: Seq, target: Seq, ops: bytes) -> Dict[str, object]:
    """Python twin of `_pileup.replay_ops`: counts and CIGAR of an op string;
    ValueError when it does not replay onto (n, m)."""
    q, t = as_bytes(query, "query"), as_bytes(target, "target")
    n, m = len(q), len(t)
    runs: List[List] = []

    def push(cnt: int, op: str) -> None:
        if cnt <= 0:
            return
        if runs and runs[-1][1] == op:
            runs[-1][0] += cnt
        else:
            runs.append([cnt, op])

    j = _ext(q, t, 0, 0)
    i = j
    push(j, "M")
    nx = ni = nd = 0
    for pos, op in enumerate(bytes(ops)):
        c = chr(op)
        if c == "X":
            if not (i < n and j < m and q[i] != t[j]):
                raise ValueError(f"op {pos} (X) is not legal at ({i}, {j})")
            i, j, nx = i + 1, j + 1, nx + 1
            push(1, "M")
        elif c == "D":
            if not j < m:
                raise ValueError(f"op {pos} (D) is not legal at ({i}, {j})")
            j, nd = j + 1, nd + 1
            push(1, "D")
        elif c == "I":
            if not i < n:
                raise ValueError(f"op {pos} (I) is not legal at ({i}, {j})")
            i, ni = i + 1, ni + 1
            push(1, "I")
        else:
            raise ValueError(f"op {pos} is not one of X, D, I")
        j2 = _ext(q, t, i, j)
        push(j2 - j, "M")
        i, j = i + (j2 - j), j2
    if (i, j) != (n, m):
        raise ValueError(f"op string ends at ({i}, {j}), not ({n}, {m})")
    return {
        "edit_distance": nx + ni + nd,
        "matches": n - nx - ni,
        "mismatches": nx,
        "insertions": ni,
        "deletions": nd,
        "cigar": "".join(f"{c}{op}" for c, op in runs),
    }


def edit_sites(query: Seq, target: Seq,
               cigar: str) -> Iterator[Tuple[int, str, int]]:
    """One (truth position, op, assembly position) per edit of a replayed
    CIGAR, in order; op is X, I or D and positions are 1-based. For I the
    truth position, and for D the assembly position, is that of the base the
    edit follows (0 at the very start)."""
    q = np.frombuffer(as_bytes(query, "query"), dtype=np.uint8)
    t = np.frombuffer(as_bytes(target, "target"), dtype=np.uint8)
    i = j = num = 0
    for ch in cigar:
        if ch.isdigit():
            num = num * 10 + int(ch)
            continue
        if ch == "M":
            for off in np.flatnonzero(q[i:i + num] != t[j:j + num]):
                yield j + int(off) + 1, "X", i + int(off) + 1
            i, j = i + num, j + num
        elif ch == "I":
            for off in range(num):
                yield j, "I", i + off + 1
            i += num
        elif ch == "D":
            for off in range(num):
                yield j + off + 1, "D", i
            j += num
        else:
            raise ValueError(f"unexpected CIGAR op {ch!r}")
        num = 0


# ---------------------------------------------------------------------------
# routes

def _ops_cpu(q: bytes, t: bytes, max_score: Optional[int]) -> bytes:
    from .ops import pileup_ext

    try:
        return pileup_ext().wfa_ops(q, t, -1 if max_score is None
                                    else int(max_score))
    except RuntimeError as e:
        if "max_score" in str(e):
            raise ScoreLimitError(str(e)) from None
        raise


def _ops_device(q: bytes, t: bytes, max_score: Optional[int],
                budget_bytes: Optional[int], device) -> bytes:
    """The device route: upload once, enqueue the score steps a chunk at a
    time (the only synchronisation is the read of `done` after each chunk),
    walk the direction tables backwards on the device, fetch the op string."""
    import torch

    from . import ops

    ext = ops.ext()
    if (ext.wfa_probe(), ext.wfa_coop()) != (PROBE, COOP):
        raise RuntimeError("wfa.PROBE / wfa.COOP differ from the built kernel")
    n, m = len(q), len(t)
    if n + m + 3 + PAD >= 1 << 31:
        raise ValueError("sequences too long for int32 offsets")
    dev = torch.device("cuda", torch.cuda.current_device()) \
        if device is None or device is True else torch.device(device)
    limit = max(n, m) if max_score is None else min(int(max_score), max(n, m))
    with torch.cuda.device(dev):
        if budget_bytes is None:
            budget_bytes = int(BUDGET_SHARE * torch.cuda.mem_get_info()[0])
        first = dir_cells(n, m, 0, min(CHUNK_FIRST, limit + 1))
        if first > budget_bytes:
            raise BudgetError(f"direction table of the first chunk ({first} "
                              f"bytes) exceeds the budget ({budget_bytes})")

        def padded(b: bytes, pad: int) -> "torch.Tensor":
            a = np.full(len(b) + PAD, pad, dtype=np.uint8)
            a[:len(b)] = np.frombuffer(b, dtype=np.uint8)
            return torch.from_numpy(a).to(dev)

        dq, dt = padded(q, QUERY_PAD), padded(t, TARGET_PAD)
        offs = torch.full((2, n + m + 3), NEG, dtype=torch.int32, device=dev)
        done = torch.full((1,), -1, dtype=torch.int32, device=dev)
        chunks = []
        used, s0, dist = 0, 0, -1
        for s1 in chunk_bounds():
            s1 = min(s1, limit + 1)
            cells = dir_cells(n, m, s0, s1)
            if used + cells > budget_bytes:
                raise BudgetError(
                    f"direction tables up to score {s1 - 1} need "
                    f"{used + cells} bytes, the budget is {budget_bytes}")
            table = torch.empty(cells, dtype=torch.uint8, device=dev)
            ext.wfa_steps(dq, dt, n, m, s0, s1, offs, table, done)
            chunks.append((s0, s1, table))
            used += cells
            dist = int(done.item())
            if dist >= 0:
                break
            if s1 > limit:
                if max_score is not None and limit == int(max_score):
                    raise ScoreLimitError(
                        f"edit distance exceeds max_score {max_score}")
                raise RuntimeError("wfa: no alignment within max(n, m) edits")
            s0 = s1
        if dist == 0:
            return b""
        out = torch.empty(dist, dtype=torch.uint8, device=dev)
        # walk state: {current diagonal, error flag}
        walk = torch.tensor([m - n, 0], dtype=torch.int32, device=dev)
        for c0, c1, table in reversed(chunks):
            hi = min(dist, c1 - 1)
            if hi >= max(c0, 1):
                ext.wfa_trace(table, n, m, c0, hi, walk, out)
        if int(walk[1].item()) != 0:
            raise RuntimeError("wfa: device traceback left the wavefront")
        return out.cpu().numpy().tobytes()


def align(query: Seq, target: Seq, device=None,
          max_score: Optional[int] = None,
          budget_bytes: Optional[int] = None) -> Dict[str, object]:
    """Exact global alignment of `query` against `target`.

    Returns the `replay_ops` dict (edit_distance, matches, mismatches,
    insertions, deletions, cigar) plus `ops` (the op string) and `route`
    ("device" or "cpu"). device=None on a host without a GPU takes the C++
    route; with a GPU it needs the kernels (as `ops.require` does), runs the
    C++ route bounded to distances below DEVICE_MIN_SCORE, where it is the
    faster one, and sends a pair beyond that to the device. device=True or a
    torch device insists on the GPU; device=False or "cpu" takes the C++
    route. `max_score` bounds the distance (ScoreLimitError) and
    `budget_bytes` the device direction tables (BudgetError; default: half of
    the free device memory). Both sequences must be printable ASCII.
    """
    from .ops import pileup_ext

    q, t = as_bytes(query, "query"), as_bytes(target, "target")
    if max_score is not None and max_score < 0:
        raise ValueError("max_score must be >= 0")
    if device is False or device == "cpu":
        ops_, route = _ops_cpu(q, t, max_score), "cpu"
    elif device is None:
        import torch

        cap = DEVICE_MIN_SCORE - 1
        if not torch.cuda.is_available() or (max_score is not None
                                             and max_score <= cap):
            ops_, route = _ops_cpu(q, t, max_score), "cpu"
        else:
            from . import ops

            ops.require()
            try:
                ops_, route = _ops_cpu(q, t, cap), "cpu"
            except ScoreLimitError:
                ops_, route = _ops_device(q, t, max_score, budget_bytes,
                                          None), "device"
    else:
        ops_, route = _ops_device(q, t, max_score, budget_bytes, device), \
            "device"
    res = dict(pileup_ext().replay_ops(q, t, ops_))
    res["ops"] = ops_
    res["route"] = route
    return res
