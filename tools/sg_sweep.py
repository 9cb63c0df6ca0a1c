"""Skinny packed GEMM sweep: shapes x KC x split x NW, TB/s + correctness.

python tools/sg_sweep.py [M] [--cold] [--shapes qkv,o,gate_up,down]

--cold rotates every timed call over enough distinct weight copies to
exceed twice the 256 MiB Infinity Cache, so no call finds its weights
cached (the decode graph streams 15 GB of weights between two uses of one
matrix). The default warm loop re-reads one copy and flatters anything
that fits the cache, or nearly does: gate_up (235 MB) measured 13 us
faster warm than in-graph.
"""
import argparse
import sys
import time

import torch

sys.path.insert(0, ".")
import agentainer_amd.ops as O
from agentainer_amd.ops import pack_weight

ap = argparse.ArgumentParser()
ap.add_argument("M", nargs="?", type=int, default=64)
ap.add_argument("--cold", action="store_true")
ap.add_argument("--shapes", default="qkv,o,gate_up,down")
ap.add_argument("--iters", type=int, default=200)
args = ap.parse_args()

mod = O._load_hip()
M = args.M
ALL = {"qkv": (6144, 4096), "o": (4096, 4096), "gate_up": (28672, 4096),
       "down": (4096, 14336)}
LLC = 256 << 20


def timed(fns):
    """us per call, cycling over fns (one per weight copy)."""
    n = len(fns)
    for i in range(max(20, n)):
        fns[i % n]()
    torch.cuda.synchronize()
    t0 = time.time()
    for i in range(args.iters):
        fns[i % n]()
    torch.cuda.synchronize()
    return (time.time() - t0) / args.iters * 1e6


for name in args.shapes.split(","):
    N, K = ALL[name]
    nbytes = N * K * 2
    copies = max(3, -(-2 * LLC // nbytes) + 1) if args.cold else 1
    ws_ = [torch.randn(N, K, dtype=torch.bfloat16, device="cuda") * 0.05
           for _ in range(copies)]
    wps = [pack_weight(w) for w in ws_]
    x = torch.randn(M, K, dtype=torch.bfloat16, device="cuda")
    ref = torch.nn.functional.linear(x.float(), ws_[0].float())
    gb = nbytes / 1e9
    mode = f"cold x{copies}" if args.cold else "warm"
    dlib = timed([lambda w=w: torch.nn.functional.linear(x, w) for w in ws_])
    print(f"{name} N={N:6d} K={K:6d} [{mode}] lib: {dlib:7.1f} us "
          f"{gb/dlib*1e3:5.2f} TB/s", flush=True)
    if name == "gate_up":
        inter = N // 2
        act = torch.empty(M, inter, dtype=torch.bfloat16, device="cuda")

        def lib_silu(w):
            gu = torch.nn.functional.linear(x, w)
            mod.silu_mul(act, gu[:, :inter], gu[:, inter:])

        d = timed([lambda w=w: lib_silu(w) for w in ws_])
        print(f"  lib + silu_mul: {d:7.1f} us", flush=True)
    for kc in (128, 256):
        for split in (1, 2, 4, 8, 16):
            if (K % (kc * split) or K % (256 * split)
                    or (N // 64) * split > 4096):
                continue
            for nw in (1, 2, 4):
                if N % (64 * nw) or (N // (64 * nw)) * split < 64:
                    continue
                ws = O._skinny_ws(x.device, N, split)
                out = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
                mod.skinny_gemm_packed(out, x, wps[0], N, K, ws, split, False,
                                       kc, True, nw)
                torch.cuda.synchronize()
                rel = ((out.float() - ref).abs().max().item()
                       / ref.abs().max().item())
                d = timed([lambda wp=wp: mod.skinny_gemm_packed(
                    out, x, wp, N, K, ws, split, False, kc, True, nw)
                    for wp in wps])
                flag = "BAD" if rel > 2e-2 else "ok"
                print(f"  kc={kc} split={split:2d} nw={nw}: {d:7.1f} us "
                      f"{gb/d*1e3:5.2f} TB/s  rel={rel:.1e} {flag}",
                      flush=True)
    del ws_, wps
