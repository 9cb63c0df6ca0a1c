"""LoRA cost on the MI355X: the BGMV kernel pair alone, and the engine's
decode step with the adapter pool off / on-but-unused / in use.

  python tools/lora_bench.py --kernels          # per-kernel times
  python tools/lora_bench.py --engine           # ms per decode step, 3 configs
  python tools/lora_bench.py --out FILE.json    # also write the JSON there

Kernel part: Llama-3-8B projection shapes (qkv, o, gate_up, down with pool
ranks 48, 16, 32, 16 at lora_max_rank 16), T in {1, 16, 64}, four resident
adapters, rows spread over them; device-event time over --iters launches
after --warmup, min and median of --rounds rounds.

Engine part: 64 agents decoding on llama3-8b, host clock around --steps
steps between two device synchronisations, for
  off      engine.lora_slots = 0
  idle     lora_slots = 4, no adapter bound: the cost of the pool being on
           (non-deferred o/down reduction + eight launches per layer that
           skip every row)
  active   the 64 agents spread over four rank-16 adapters
Needs a GPU; there is no CPU fallback for a timing.
"""

from __future__ import annotations

import argparse
import gc
import json
import os
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from agentainer_amd import ops  # noqa: E402
from agentainer_amd.config import load_config  # noqa: E402
from agentainer_amd.engine.llm import GenRequest, LLMEngine  # noqa: E402
from agentainer_amd.models.llama import LLAMA_CONFIGS  # noqa: E402
from agentainer_amd.models.lora import FUSED, _PARENT, proj_dims  # noqa: E402
from agentainer_amd.registry import Manager  # noqa: E402
from agentainer_amd.store import Store  # noqa: E402

# (name, K, N, R) of the four fused projections of llama3-8b
SHAPES_8B = [("qkv", 4096, 6144, 48), ("o", 4096, 4096, 16),
             ("gate_up", 4096, 28672, 32), ("down", 14336, 4096, 16)]
S = 4


def _time_us(fn, warmup, iters, rounds):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(rounds):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1000.0 / iters)
    return {"min_us": round(min(out), 2),
            "median_us": round(statistics.median(out), 2)}


def bench_kernels(args):
    dev = "cuda"
    rows = []
    for name, K, N, R in SHAPES_8B:
        A = (torch.randn(S, R, K, device=dev) / K ** 0.5).bfloat16()
        B = (torch.randn(S, N, R, device=dev) / R ** 0.5).bfloat16()
        for T in (1, 16, 64):
            x = torch.randn(T, K, device=dev).bfloat16()
            y = torch.randn(T, N, device=dev).bfloat16()
            v = torch.empty(T, R, device=dev)
            ids = (torch.arange(T, device=dev) % S).int()
            none = torch.full((T,), -1, dtype=torch.int32, device=dev)
            row = {"proj": name, "K": K, "N": N, "R": R, "T": T}
            row["shrink"] = _time_us(lambda: ops.lora_shrink(v, x, A, ids),
                                     args.warmup, args.iters, args.rounds)
            row["expand_add"] = _time_us(
                lambda: ops.lora_expand_add(y, v, B, ids),
                args.warmup, args.iters, args.rounds)
            row["pair_all_rows_skipped"] = _time_us(
                lambda: ops.lora_apply(y, x, A, B, none),
                args.warmup, args.iters, args.rounds)
            print(json.dumps(row), flush=True)
            rows.append(row)
    return rows


def _write_adapter(path, cfg, r, seed):
    from safetensors.torch import save_file
    os.makedirs(path, exist_ok=True)
    gen = torch.Generator().manual_seed(seed)
    sd = {}
    dims = proj_dims(cfg)
    for i in range(cfg.n_layers):
        for proj, mods in FUSED.items():
            K, outs = dims[proj]
            for m, n in zip(mods, outs):
                base = f"base_model.model.model.layers.{i}.{_PARENT[m]}.{m}."
                sd[base + "lora_A.weight"] = (
                    torch.randn(r, K, generator=gen) / K ** 0.5).bfloat16()
                sd[base + "lora_B.weight"] = (
                    torch.randn(n, r, generator=gen) * 0.01).bfloat16()
    with open(os.path.join(path, "adapter_config.json"), "w") as f:
        json.dump({"r": r, "lora_alpha": 2 * r,
                   "target_modules": sorted(_PARENT)}, f)
    save_file(sd, os.path.join(path, "adapter_model.safetensors"))
    return path


def _engine_case(args, tmp, tag, lora_slots, adapters):
    cfg = load_config(path="/nonexistent.yaml", env={})
    root = os.path.join(tmp, tag)
    cfg.data["store"]["path"] = root
    cfg.data["engine"].update(sync_mode=True, max_batch_tokens=16384,
                              max_decode_batch=args.agents,
                              kv_pool_gb=args.kv_pool_gb,
                              lora_slots=lora_slots, lora_max_rank=16)
    store = Store(os.path.join(root, "state"), sync="never")
    engine = LLMEngine(store, cfg, device=args.device, state_root=root)
    manager = Manager(store, engine, cfg)
    agents = []
    for i in range(args.agents):
        a = manager.deploy(name=f"a{i}", model=args.model,
                           lora=adapters[i % len(adapters)] if adapters else "")
        manager.start(a.id)
        agents.append(a)
    inst = engine._instances[args.model]
    gen = torch.Generator().manual_seed(0)
    total = args.warmup_steps + args.steps + 16
    reqs = []
    for a in agents:
        toks = torch.randint(3, inst.cfg.vocab_size, (args.prompt_len,),
                             generator=gen).tolist()
        req = GenRequest(agent_id=a.id, prompt_tokens=toks, max_new=total + 8,
                         temperature=0.0, top_p=1.0, seed=0)
        b = inst.binding(a.id)
        with inst._lock:
            b.queue.put(req)
            inst._pump_agent(b)
        reqs.append(req)
    for _ in range(64):  # prefill until every agent decodes
        inst.step()
        if len(inst.running) == args.agents:
            break
    assert len(inst.running) == args.agents, "prefill did not finish"
    for _ in range(args.warmup_steps):
        inst.step()
    rounds = []
    per = max(args.steps // args.rounds, 1)
    for _ in range(args.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(per):
            inst.step()
        torch.cuda.synchronize()
        rounds.append((time.perf_counter() - t0) * 1000.0 / per)
    st = engine.stats()["models"][args.model]
    assert not any(r.error for r in reqs)
    res = {"config": tag, "lora_slots": lora_slots,
           "adapters_bound": len(adapters), "agents": args.agents,
           "steps_per_round": per,
           "ms_per_step_min": round(min(rounds), 3),
           "ms_per_step_median": round(statistics.median(rounds), 3),
           "ms_per_step_rounds": [round(r, 3) for r in rounds],
           "use_graph": st["use_graph"], "async_decode": st["async_decode"]}
    print(json.dumps(res), flush=True)
    engine.shutdown()
    del inst, engine, manager, reqs
    ops._ws_cache.clear()
    ops._lora_ws_cache.clear()
    gc.collect()
    torch.cuda.empty_cache()
    return res


def bench_engine(args):
    cfg = LLAMA_CONFIGS[args.model]
    out = []
    with tempfile.TemporaryDirectory(prefix="lora-bench-") as tmp:
        adapters = [_write_adapter(os.path.join(tmp, f"adapter{i}"), cfg, 16, i)
                    for i in range(4)]
        out.append(_engine_case(args, tmp, "off", 0, []))
        out.append(_engine_case(args, tmp, "idle", 4, []))
        out.append(_engine_case(args, tmp, "active", 4, adapters))
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--kernels", action="store_true")
    p.add_argument("--engine", action="store_true")
    p.add_argument("--model", default="llama3-8b")
    p.add_argument("--agents", type=int, default=64)
    p.add_argument("--prompt-len", type=int, default=256)
    p.add_argument("--steps", type=int, default=200)
    p.add_argument("--warmup-steps", type=int, default=20)
    p.add_argument("--kv-pool-gb", type=float, default=16.0)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--iters", type=int, default=200)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lora_bench needs a GPU: a CPU run gives no timing")
    args.device = "cuda"
    if not (args.kernels or args.engine):
        args.kernels = args.engine = True
    res = {}
    if args.kernels:
        res["kernels"] = bench_kernels(args)
    if args.engine:
        res["engine"] = bench_engine(args)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
