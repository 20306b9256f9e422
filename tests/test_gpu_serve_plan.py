"""ext.ServeSlot.plan: what a serving slot decided to launch, for every
documented switch. Construction only: no kernel is launched and nothing is
captured."""

import pytest
import torch

from roko_amd.model import RokoModel
from tests.serve_plan_cases import expected_plan, wstat_pays

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs ROCm GPU"
)

SWITCHES = ("ROKO_FRONT", "ROKO_XGFOLD", "ROKO_XG2", "ROKO_XG3", "ROKO_XG4",
            "ROKO_GSLOT")


@pytest.fixture(scope="module")
def weights():
    from roko_amd.ops.forward import _bf16_weights

    torch.manual_seed(21)
    return _bf16_weights(RokoModel().cuda().eval())


def _plan(weights, B, monkeypatch, env=None):
    from roko_amd.ops import _hip_ops as ext

    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    host_out = torch.empty((B, 90), dtype=torch.uint8, pin_memory=True)
    return ext.ServeSlot(weights, B, host_out, 1).plan


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _p(front, xg, seq_ld, raw, graph):
    return {"front": front, "xg": xg if isinstance(xg, list) else [xg] * 3,
            "seq_ld": seq_ld, "raw": raw, "graph": graph}


@requires_gpu
@pytest.mark.parametrize("B", [32, 64])
def test_narrow_slot_is_lt(weights, monkeypatch, B):
    assert _plan(weights, B, monkeypatch) == _p("v4", "lt", 500, False, False)


@requires_gpu
def test_default_widths(weights, monkeypatch):
    assert _plan(weights, 128, monkeypatch) == _p("v4", "xg3", 512, True,
                                                 False)
    assert _plan(weights, 256, monkeypatch) == _p("v4", "xg3", 512, True,
                                                 True)
    # the shipped coalesced width: W-stationary for the K = 256 layers
    # wherever it pays, which on 256 CUs is from B = 1024 up
    assert wstat_pays(1024, 256) and not wstat_pays(896, 256)
    tail = "wstat" if wstat_pays(1024, _cus()) else "xg3"
    assert _plan(weights, 1024, monkeypatch) == _p(
        "v4", ["xg3", tail, tail], 512, True, True)


@requires_gpu
@pytest.mark.parametrize("env,want", [
    ({"ROKO_XG4": "0"}, _p("v4", "xg3", 512, True, False)),
    ({"ROKO_XG4": "stream"}, _p("v4", "stream", 512, True, False)),
    ({"ROKO_XG4": "wstat"},
     _p("v4", ["xg3", "wstat", "wstat"], 512, True, False)),
    ({"ROKO_XG3": "0"}, _p("v4", "xg2", 500, True, False)),
    ({"ROKO_XG2": "0"}, _p("v4", "lt", 500, False, False)),
    ({"ROKO_XGFOLD": "1"}, _p("v4", "fold", 500, True, False)),
    # v2 takes no leading dimension, so no xg3
    ({"ROKO_FRONT": "v2"}, _p("v2", "xg2", 500, True, False)),
    ({"ROKO_FRONT": "v3"}, _p("v3", "xg3", 512, True, False)),
    ({"ROKO_GSLOT": "1"}, _p("v4", "xg3", 512, True, True)),
    ({"ROKO_GSLOT": "0"}, _p("v4", "xg3", 512, True, False)),
], ids=["XG4=0", "XG4=stream", "XG4=wstat", "XG3=0", "XG2=0", "XGFOLD=1",
        "FRONT=v2", "FRONT=v3", "GSLOT=1", "GSLOT=0"])
def test_switches_at_128(weights, monkeypatch, env, want):
    got = _plan(weights, 128, monkeypatch, env)
    assert got == want
    assert got == expected_plan(128, _cus(), env)


@requires_gpu
def test_fold_is_raw_without_xg2(weights, monkeypatch):
    env = {"ROKO_XGFOLD": "1"}
    assert _plan(weights, 32, monkeypatch, env) == _p("v4", "fold", 500, True,
                                                     False)


@requires_gpu
def test_lt_path_never_graphs(weights, monkeypatch):
    env = {"ROKO_GSLOT": "1"}
    assert _plan(weights, 64, monkeypatch, env) == _p("v4", "lt", 500, False,
                                                     False)


@requires_gpu
def test_padded_weights_are_required(weights, monkeypatch):
    from roko_amd.ops import _hip_ops as ext

    w = {k: v for k, v in weights.items() if k != "w1g"}
    host_out = torch.empty((32, 90), dtype=torch.uint8, pin_memory=True)
    with pytest.raises(RuntimeError, match="w1g"):
        ext.ServeSlot(w, 32, host_out, 1)
