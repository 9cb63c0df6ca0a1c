"""Sampler kernel timing at decode shape (B=64, V=128256 by default).

One mode per process so that `rocprofv3 --kernel-trace --stats` gives each
setting its own kernel average:

    rocprofv3 --kernel-trace --stats -d rocprof_out/ex_topk -- \
        python tools/sample_bench.py --mode ex_topk

Modes: topp (the plain topp_sample kernel), ex_greedy (sample_ex, all rows
greedy with penalties over a 200-token history), ex_topk (top_k=40),
ex_nucleus (top_p=0.9 only through sample_ex: 1024 candidates sorted).
Before every call the logits are rewritten by a device copy, as the
lm_head GEMM rewrites them in the decode graph, so the sampler never
reads a row that it left in cache itself. Also prints the host-side call
time (device events around the whole ops call, H2D parameter copies
included).
"""

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from agentainer_amd import ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", required=True,
                    choices=["topp", "ex_greedy", "ex_topk", "ex_nucleus"])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    B, V = args.batch, args.vocab
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    # peaked like LLM logits: a few tokens carry the mass
    src = (torch.randn(B, V, generator=g) * 2.5).to(torch.bfloat16).to(dev)
    logits = torch.empty_like(src)
    out = torch.empty(B, dtype=torch.long, device=dev)
    seeds = list(range(B))
    hist = [[(int(t), 3, 0.0) for t in
             sorted(set(torch.randint(0, V, (200,), generator=g).tolist()))]
            for _ in range(B)]
    none = [[] for _ in range(B)]
    temps_t = torch.full((B,), 0.8, device=dev)
    tops_t = torch.full((B,), 0.9, device=dev)
    seeds_t = torch.tensor(seeds, dtype=torch.int64, device=dev)

    def call():
        if args.mode == "topp":
            ops.topp_sample(out, logits, temps_t, tops_t, seeds_t)
        elif args.mode == "ex_greedy":
            ops.sample_ex(out, logits, [0.0] * B, [1.0] * B, seeds, [0] * B,
                          [0.0] * B, [1.2] * B, [0.5] * B, [0.25] * B, hist)
        elif args.mode == "ex_topk":
            ops.sample_ex(out, logits, [0.8] * B, [1.0] * B, seeds, [40] * B,
                          [0.0] * B, [1.0] * B, [0.0] * B, [0.0] * B, none)
        else:
            ops.sample_ex(out, logits, [0.8] * B, [0.9] * B, seeds, [0] * B,
                          [0.0] * B, [1.0] * B, [0.0] * B, [0.0] * B, none)

    times = []
    for i in range(args.warmup + args.iters):
        logits.copy_(src)
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        if i >= args.warmup:
            times.append(e0.elapsed_time(e1) * 1000.0)
    times.sort()
    print(json.dumps({"mode": args.mode, "B": B, "V": V, "iters": args.iters,
                      "call_us_median": round(times[len(times) // 2], 1),
                      "call_us_min": round(times[0], 1),
                      "picks_head": out[:4].tolist()}))


if __name__ == "__main__":
    main()
