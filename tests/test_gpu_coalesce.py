"""Cross-batch coalescing of the serving pipeline: G consecutive submits
share one wide slot and one model launch. Every prediction must equal
`roko_argmax` of its own batch, whatever the order tickets are called in and
wherever a flush falls."""

import pytest
import torch

from roko_amd.model import RokoModel

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs ROCm GPU"
)

SHORT = 29  # rows of a partial batch


class _Cases:
    """Seeded inputs, distinct per (index, rows), and their references —
    each computed once and shared by every test."""

    def __init__(self):
        from roko_amd.ops.forward import roko_argmax

        torch.manual_seed(21)
        self.model = RokoModel().cuda().eval()
        self._argmax = roko_argmax
        self._x = {}
        self._ref = {}

    def x(self, i, rows):
        key = (i, rows)
        if key not in self._x:
            g = torch.Generator().manual_seed(1000 * rows + i)
            self._x[key] = torch.randint(
                0, 12, (rows, 200, 90), generator=g, dtype=torch.uint8).cuda()
        return self._x[key]

    def ref(self, i, rows):
        key = (i, rows)
        if key not in self._ref:
            with torch.no_grad():
                self._ref[key] = self._argmax(self.model, self.x(i, rows)).cpu()
        return self._ref[key]


@pytest.fixture(scope="module")
def cases():
    return _Cases()


def _pipe(cases, batch, depth, coalesce):
    from roko_amd.ops.forward import InferencePipeline

    return InferencePipeline(cases.model, batch, depth, coalesce=coalesce)


def _check(cases, ticket, i, rows):
    got = ticket()
    ref = cases.ref(i, rows)
    assert got.shape == ref.shape, (i, rows)
    assert torch.equal(got, ref), (i, rows, (got != ref).float().mean())


@requires_gpu
@pytest.mark.parametrize("batch,G", [(32, 2), (32, 4), (64, 4)])
def test_parity(cases, batch, G):
    """Widths 64 (hipBLASLt body: 90*64 % 256 != 0), 128 (specialised xg
    GEMM body) and 256 (auto-captured graph body). 3G+1 submits over two
    slots, two of them partial, tickets called newest first — the last one
    sits alone in its slot and is launched by its own ticket."""
    pipe = _pipe(cases, batch, 2 * G, G)
    assert pipe.coalesce == G and len(pipe.slots) == 2
    nsub = 3 * G + 1
    rows = [batch] * nsub
    rows[nsub // 2] = rows[-1] = SHORT
    tickets = [pipe.submit(cases.x(i, rows[i]), copy_out=True)
               for i in range(nsub)]
    for i in reversed(range(nsub)):
        _check(cases, tickets[i], i, rows[i])


@requires_gpu
def test_shipped_width_matches_narrow_batches(cases):
    """The shipped serving shape: 8 x 128 rows in one slot of width 1024,
    wider than any other test runs the model; the references run at width
    128 and every row must still be equal."""
    G, batch = 8, 128
    pipe = _pipe(cases, batch, G, G)
    tickets = [pipe.submit(cases.x(i, batch), copy_out=True)
               for i in range(G)]
    assert pipe.unlaunched() == 0
    for i in range(G):
        _check(cases, tickets[i], i, batch)


@requires_gpu
def test_flush_by_ticket(cases):
    """A ticket launches its partly filled slot itself; the parts that
    arrive later complete the round and launch the same slot again."""
    G, batch = 4, 32
    pipe = _pipe(cases, batch, G, G)
    first = pipe.submit(cases.x(0, batch), copy_out=True)
    assert pipe.unlaunched() == 1
    _check(cases, first, 0, batch)
    assert pipe.unlaunched() == 0
    more = [pipe.submit(cases.x(i, batch), copy_out=True)
            for i in range(1, G + 1)]
    _check(cases, first, 0, batch)
    for i, t in enumerate(more, start=1):
        _check(cases, t, i, batch)


@requires_gpu
@pytest.mark.parametrize("G", [2, 4, 8])
def test_benchmark_pattern(cases, G):
    """32 submits with copy_out=False and only a device synchronize, as
    bench.py does per step: nothing may be left unlaunched or running, and
    the last `depth` tickets hold their own batches."""
    depth, batch, nsub = 8, 32, 32
    pipe = _pipe(cases, batch, depth, G)
    assert pipe.coalesce == G
    tickets = [pipe.submit(cases.x(i, batch), copy_out=False)
               for i in range(nsub)]
    torch.cuda.synchronize()
    assert pipe.unlaunched() == 0
    assert all(s.cpp.done() for s in pipe.slots)
    for i in range(nsub - depth, nsub):
        _check(cases, tickets[i], i, batch)


@requires_gpu
def test_reuse_saves_previous_tenant(cases):
    """depth + G submits with copy_out=True, no ticket called until the
    end: the first G tenants are saved before their parts are overwritten."""
    G, depth, batch = 4, 8, 32
    pipe = _pipe(cases, batch, depth, G)
    nsub = depth + G
    tickets = [pipe.submit(cases.x(i, batch), copy_out=True)
               for i in range(nsub)]
    for i in range(nsub):
        _check(cases, tickets[i], i, batch)


@requires_gpu
def test_odd_depth_is_uncoalesced(cases):
    """A coalesce request that no power of two > 1 dividing `depth` can
    serve runs today's one-batch-per-slot path."""
    pipe = _pipe(cases, 32, 3, 4)
    assert pipe.coalesce == 1
    assert len(pipe.slots) == 3
    assert pipe.slots[0].cpp.amax.shape == (32, 90)
    t = pipe.submit(cases.x(0, SHORT), copy_out=True)
    assert pipe.unlaunched() == 0
    _check(cases, t, 0, SHORT)


@requires_gpu
def test_votes_need_uncoalesced(cases):
    pipe = _pipe(cases, 32, 2, 2)
    assert pipe.coalesce == 2
    with pytest.raises(RuntimeError):
        pipe.votes_staging()
    table = torch.zeros(64, dtype=torch.int32, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError):
        pipe.submit_votes(1, table, 64, err)
