"""The driver depends on bench.py's exact output contract: JSON lines on
stdout with the documented schema, the LAST being the inference record. Run
it end-to-end on CPU (tiny step counts; eager torch path; a plain run times
the inference section only, the train section sits behind --full and skips
without a GPU) and validate every field the driver reads."""

import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cpu_env():
    """Environment for the CPU rehearsals below: they use batches and rank
    counts that only the eager path takes, so hide any GPU of the host."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    env.pop("RANK", None), env.pop("WORLD_SIZE", None)
    return env


def test_bench_json_contract_cpu():
    out = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"),
         "--steps", "2", "--warmup", "1", "--batch", "8", "--depth", "2"],
        cwd=ROOT, capture_output=True, text=True, timeout=600, env=_cpu_env(),
    )
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.strip().splitlines() if l.startswith("{")]
    # a plain run prints the inference record; under --full on GPU a train
    # record precedes it (the driver parses the last line)
    assert len(lines) >= 1, out.stdout
    r = json.loads(lines[-1])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup",
                "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config"):
        assert key in r, key
    assert r["metric"] == "inference_bases_per_sec"
    assert r["n_gpus"] == 1 and r["steps"] == 2 and r["warmup"] == 1
    assert r["higher_is_better"] is True
    assert r["scaling"] == "weak"
    assert r["data"] == "synthetic"
    assert r["value"] > 0 and r["ms_per_step"] > 0
    cfg = r["config"]
    for key in ("model", "global_batch", "seq_len", "parallelism"):
        assert key in cfg, key
    assert cfg["global_batch"] == 8 and cfg["seq_len"] == 90


def _run_bench(*extra):
    out = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
         "--steps", "2", "--warmup", "1", "--batch", "32", "--depth", "2",
         *extra],
        cwd=ROOT, capture_output=True, text=True, timeout=600,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    return [json.loads(l) for l in out.stdout.strip().splitlines()
            if l.startswith("{")]


def test_bench_plain_run_is_headline_only_and_dumps_outputs(tmp_path):
    """A plain run prints the inference record alone; --full keeps the
    inference record last. --dump-outputs writes the last timed step's
    predictions as float32 .npy, identical from run to run (seeded inputs
    and weights), whatever else the run measures."""
    import numpy as np

    a, b = tmp_path / "a", tmp_path / "b"
    plain = _run_bench("--dump-outputs", str(a))
    full = _run_bench("--full", "--dump-outputs", str(b))
    assert [r["metric"] for r in plain] == ["inference_bases_per_sec"]
    assert plain[0]["config"]["mode"] == "inference"
    assert full[-1]["metric"] == "inference_bases_per_sec"
    assert full[-1]["config"]["mode"] == "inference"
    for key in ("metric", "unit", "higher_is_better", "dtype", "steps",
                "warmup", "n_gpus"):
        assert plain[0][key] == full[-1][key], key
    assert plain[0]["steps"] == 2 and plain[0]["ms_per_step"] > 0

    pa = np.load(a / "predictions.npy")
    pb = np.load(b / "predictions.npy")
    assert pa.dtype == np.float32
    # (batches kept from the last step, batch, window columns)
    assert pa.ndim == 3 and pa.shape[1:] == (32, 90) and pa.shape[0] >= 1
    assert pa.nbytes <= 64 << 20
    assert ((pa >= 0) & (pa < 5) & (pa == np.round(pa))).all()
    np.testing.assert_array_equal(pa, pb)
    # the logits behind the step's final batch agree with its predictions
    la = np.load(a / "logits.npy")
    assert la.dtype == np.float32 and la.shape == (32, 90, 5)
    assert np.isfinite(la).all()
    np.testing.assert_array_equal(la.argmax(axis=2), pa[-1])


def test_hw_queue_default_set_on_import():
    """The 4-HW-queue default serializes the serving streams; the package
    must raise it before HIP init (PERF_HISTORY.md)."""
    out = subprocess.run(
        [sys.executable, "-c",
         "import roko_amd, os; print(os.environ['GPU_MAX_HW_QUEUES'])"],
        cwd=ROOT, capture_output=True, text=True, timeout=120,
        env={k: v for k, v in os.environ.items()
             if k != "GPU_MAX_HW_QUEUES"},
    )
    assert out.returncode == 0, out.stderr[-500:]
    assert out.stdout.strip() == "20"


def test_bench_gpus_flag_validated():
    """--gpus N without a matching torchrun WORLD_SIZE must exit loudly
    (round-1 flagged the flag as cosmetic)."""
    out = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4",
         "--steps", "1", "--warmup", "0"],
        cwd=ROOT, capture_output=True, text=True, timeout=300,
    )
    assert out.returncode != 0
    assert "WORLD_SIZE" in out.stderr


def test_bench_world2_gloo():
    """The driver launches bench.py under torchrun with --nproc-per-node N;
    rehearse that exact shape at N=2 on CPU (gloo): rendezvous, per-rank
    work, MAX-reduce of elapsed, and rank-0-only JSON output."""
    env = _cpu_env()
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29871", os.path.join(ROOT, "bench.py"),
         "--gpus", "2", "--steps", "2", "--warmup", "1",
         "--batch", "4", "--depth", "2"],
        cwd=ROOT, capture_output=True, text=True, timeout=900, env=env,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.strip().splitlines() if l.startswith("{")]
    # rank 0 prints once per record; no duplicate records from rank 1
    recs = [json.loads(l) for l in lines]
    assert len([r for r in recs if r["metric"] == "inference_bases_per_sec"]) == 1
    r = recs[-1]
    assert r["n_gpus"] == 2
    assert r["config"]["parallelism"] == "dp2"
    assert r["config"]["global_batch"] == 8
