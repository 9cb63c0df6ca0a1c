"""Logprobs kernel timing at decode shape (B=64, V=128256 by default)
against the torch composition it replaces:

    lp = torch.log_softmax(logits.float(), -1)
    lp.gather(1, chosen[:, None]); lp.topk(K)

For each K the two are timed alternately in one loop, each between device
events of its own. Before every call the logits are rewritten by a device
copy, as the lm_head GEMM rewrites them in the decode graph, so neither
side reads rows that it left in cache itself. Prints one JSON line per K
with both mean times and the kernel's ratio to the one-read traffic floor
(B * V * 2 bytes at --hbm-tbs).
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
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--ks", default="0,5,20")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--hbm-tbs", type=float, default=8.0,
                    help="peak HBM bandwidth for the traffic floor, TB/s")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    B, V = args.batch, args.vocab
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    # peaked like LLM logits: a few tokens carry the mass
    src = (torch.randn(B, V, generator=g) * 2.5).to(torch.bfloat16).to(dev)
    logits = torch.empty_like(src)
    rows = torch.arange(B, dtype=torch.int32, device=dev)
    chosen = torch.randint(0, V, (B,), generator=g).to(dev)
    floor_us = B * V * 2 / (args.hbm_tbs * 1e12) * 1e6

    def kernel(K):
        return ops.token_logprobs(logits, rows, chosen, K)

    def composed(K):
        lp = torch.log_softmax(logits.float(), -1)
        out = lp.gather(1, chosen[:, None])
        return (out, *lp.topk(K)) if K else (out,)

    for K in (int(k) for k in args.ks.split(",")):
        total = {"kernel": 0.0, "torch": 0.0}
        for it in range(args.warmup + args.iters):
            for name, fn in (("kernel", kernel), ("torch", composed)):
                logits.copy_(src)
                t0 = torch.cuda.Event(enable_timing=True)
                t1 = torch.cuda.Event(enable_timing=True)
                t0.record()
                fn(K)
                t1.record()
                t1.synchronize()
                if it >= args.warmup:
                    total[name] += t0.elapsed_time(t1)
        k_us = total["kernel"] / args.iters * 1e3
        t_us = total["torch"] / args.iters * 1e3
        print(json.dumps({
            "batch": B, "vocab": V, "K": K, "kernel_us": round(k_us, 1),
            "torch_us": round(t_us, 1), "speedup": round(t_us / k_us, 2),
            "floor_us": round(floor_us, 2),
            "kernel_over_floor": round(k_us / floor_us, 1)}), flush=True)


if __name__ == "__main__":
    main()
