"""Driver-contract test for bench.py: the round-end harness runs
`python bench.py --gpus N --steps K --warmup W` (N>1 via
torch.distributed.run), parses ONE JSON line from rank 0 and computes
scaling efficiency from per-N values. These tests pin that contract on
CPU (gloo world 2) so the 8-GPU scaling run can't be broken by a repo
change that only CPU CI sees."""

import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REQUIRED = {"metric", "value", "unit", "n_gpus", "steps", "warmup",
            "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config"}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _last_json_line(stdout: str) -> dict:
    lines = [ln for ln in stdout.strip().splitlines() if ln.startswith("{")]
    assert lines, f"no JSON line in output: {stdout[-2000:]}"
    return json.loads(lines[-1])


@pytest.mark.timeout(300)
def test_bench_single_process_contract():
    r = subprocess.run([sys.executable, "bench.py", "--steps", "10",
                        "--warmup", "2"],
                       capture_output=True, text=True, cwd=ROOT, timeout=280)
    assert r.returncode == 0, r.stderr[-2000:]
    out = _last_json_line(r.stdout)
    assert REQUIRED.issubset(out.keys())
    assert out["metric"] == "concurrent_agent_chat_req_per_s"
    assert out["scaling"] == "weak"
    assert out["higher_is_better"] is True
    assert out["ms_per_step"] > 0
    assert out["config"]["parallelism"] == "dp1"
    # the headline must be NON-VACUOUS at any driver-chosen step count
    # (steps=20 x gen_len=64 produced value=0.0): requests
    # complete inside the timed region and carry a real p50
    assert out["value"] > 0
    assert out["config"]["p50_e2e_s"] is not None
    assert out["config"]["gen_len"] <= max(out["steps"] // 2, 1)


@pytest.mark.timeout(300)
def test_bench_dump_outputs_reproducible(tmp_path):
    """--dump-outputs writes the last timed step's arrays as float .npy
    files (<= 64 MB in all), identical from run to run for the same
    arguments; --steps is the number of timed steps; --full is accepted."""
    import numpy as np

    dumps = []
    for name, extra in (("a", []), ("b", ["--full"])):
        d = tmp_path / name
        r = subprocess.run([sys.executable, "bench.py", "--gpus", "1",
                            "--steps", "50", "--warmup", "9",
                            "--dump-outputs", str(d)] + extra,
                           capture_output=True, text=True, cwd=ROOT,
                           timeout=280)
        assert r.returncode == 0, r.stderr[-2000:]
        out = _last_json_line(r.stdout)
        # above the old CPU caps (40 / 8): the request is honoured as given
        assert out["steps"] == 50 and out["warmup"] == 9
        assert out["ms_per_step"] > 0
        dumps.append({p.name: np.load(p) for p in sorted(d.glob("*.npy"))})
    a, b = dumps
    assert {"last_step_logits.npy", "last_step_tokens.npy",
            "reply_tokens.npy"} <= set(a)
    assert set(a) == set(b)
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for k in a:
        assert a[k].dtype in (np.float32, np.float64), k
        assert np.array_equal(a[k], b[k]), k
    n_agents, vocab = a["last_step_logits.npy"].shape
    assert a["last_step_tokens.npy"].shape == (n_agents,)
    assert np.isfinite(a["last_step_logits.npy"]).all()
    # greedy decode: the dumped tokens are the argmax of the dumped logits
    # (the sampler reads them as bf16; ties are compared by value)
    import torch

    lg = torch.from_numpy(a["last_step_logits.npy"]).to(
        torch.bfloat16).float().numpy()
    tk = a["last_step_tokens.npy"].astype(np.int64)
    assert np.array_equal(lg[np.arange(n_agents), tk], lg.max(axis=1))
    assert (a["reply_tokens.npy"] >= 0).any()


@pytest.mark.timeout(300)
def test_bench_driver_r1_shape_nonzero():
    """The EXACT launch shape whose round-1 record carried value=0.0
    (driver ran --steps 20 --warmup 5 against gen_len=64)."""
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1",
                        "--steps", "20", "--warmup", "5"],
                       capture_output=True, text=True, cwd=ROOT, timeout=280)
    assert r.returncode == 0, r.stderr[-2000:]
    out = _last_json_line(r.stdout)
    assert out["value"] > 0, out
    assert out["config"]["p50_e2e_s"] is not None
    assert out["config"]["p99_e2e_s"] is not None


@pytest.mark.timeout(300)
def test_bench_world2_gloo_contract():
    """Exactly the driver's multi-GPU launch shape, on CPU/gloo."""
    env = dict(os.environ)
    env["MASTER_ADDR"] = "127.0.0.1"
    r = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", str(_free_port()), "bench.py", "--gpus", "2",
         "--steps", "8", "--warmup", "2"],
        capture_output=True, text=True, cwd=ROOT, timeout=280, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    out = _last_json_line(r.stdout)
    assert out["config"]["parallelism"] == "dp2"
    # whole-job aggregate: both ranks' completions are summed
    assert out["config"]["global_batch"] == 2 * out["config"]["agents_per_gpu"]
    assert out["value"] > 0
    # p50/p99 merge every rank's e2e population (not rank-0-only)
    assert out["config"]["p50_e2e_s"] is not None


@pytest.mark.timeout(300)
def test_bench_tp2_gloo_contract():
    """Config-4 launch shape (one engine tensor-sharded across ranks):
    bench.py --gpus N --tp N under torchrun, on CPU/gloo. Pins the TP
    measurement path so the 70B TP=8 headline is driver-runnable."""
    env = dict(os.environ)
    env["MASTER_ADDR"] = "127.0.0.1"
    r = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", str(_free_port()), "bench.py", "--gpus", "2",
         "--tp", "2", "--steps", "8", "--warmup", "2"],
        capture_output=True, text=True, cwd=ROOT, timeout=280, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    out = _last_json_line(r.stdout)
    assert out["config"]["parallelism"] == "tp2"
    assert out["config"]["model"] == "tiny-llama-tp"
    assert out["scaling"] == "strong"
    assert out["value"] > 0
    assert out["config"]["p50_e2e_s"] is not None


@pytest.mark.timeout(300)
def test_server_load_harness_contract():
    """tools/server_load.py (the HTTP serving measurement behind the
    round-2 serving-path fixes) must stay runnable: echo engine, tiny
    window, one JSON line with the req/s + latency + engine fields."""
    r = subprocess.run(
        [sys.executable, "tools/server_load.py", "--device", "echo",
         "--agents", "4", "--window", "3", "--warmup", "1"],
        capture_output=True, text=True, cwd=ROOT, timeout=280)
    assert r.returncode == 0, r.stderr[-2000:]
    out = _last_json_line(r.stdout)
    assert out["tool"] == "server_load"
    assert out["http_req_per_s"] > 0
    assert out["p50_e2e_s"] is not None
    assert "engine_mode" in out and "decode_occupancy" in out
