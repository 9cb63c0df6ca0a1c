"""Record the bit-exact fixture of tests/test_prefill_attn_tiles.py.

python tools/record_prefill_golden.py [out_dir]

Runs `ops.paged_prefill_attention` of the CURRENT build on seeded inputs
and writes inputs and outputs as raw-bit .npy files (bf16 as int16, fp8 as
uint8) plus `cases.json` (page tables, lengths, row offsets). Run it on the
commit whose arithmetic is the yardstick: the committed fixture under
tests/golden/prefill_attn/ was recorded with the 32-row, one-wave-per-SIMD
kernel that preceded the latency rewrite, and the rewrite has to reproduce
it bit for bit. Re-record only when the arithmetic is changed on purpose.

Shapes are n_q = 4 / n_kv = 1 / head 128 / page 16 so the files stay
small. One KV pool (bf16 and its fp8 twin) is shared by every case; pages
are random everywhere, also past a sequence's end, so a kernel that reads a
token it should have masked shows up in the bits.
"""
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from agentainer_amd import ops  # noqa: E402

N_Q, N_KV, D, PS = 4, 1, 128, 16
POOL_PAGES = 40          # page 0 is the engine's scratch page
GAP = 3                  # unused q/out rows between sequences and at the end
SENTINEL = 0x7B7B        # bf16 bits pre-filled into `out`

SINGLES = [(0, 1), (0, 31), (0, 33), (0, 97), (5, 64), (37, 130), (300, 20)]
# name -> list of (ctx, new) or ("pad", n); max_qlen as the engine passes it
BATCHES = {
    "varlen": ([(0, 1), (16, 16), (64, 200), (0, 40)], 200),
    "padrow": ([(10, 50), ("pad", 48)], 50),
}


def build_cases():
    rng = np.random.RandomState(1234)
    cases = {}
    for ctx, new in SINGLES:
        cases[f"c{ctx}_n{new}"] = {"specs": [[ctx, new]], "max_qlen": new,
                                   "fp8": True}
    for name, (specs, mq) in BATCHES.items():
        cases[name] = {"specs": [list(s) for s in specs], "max_qlen": mq,
                       "fp8": False}
    for name, c in cases.items():
        specs = c["specs"]
        totals = [s[1] if s[0] == "pad" else s[0] + s[1] for s in specs]
        max_pages = max(-(-t // PS) for t in totals)
        perm = (rng.permutation(POOL_PAGES - 1) + 1).tolist()  # shuffled
        pt = np.zeros((len(specs), max_pages), dtype=np.int32)
        for b, (s, t) in enumerate(zip(specs, totals)):
            if s[0] == "pad":
                continue                       # repeats scratch page 0
            n = -(-t // PS)
            pt[b, :n] = [perm.pop() for _ in range(n)]
        starts, acc = [], 0
        for s in specs:
            starts.append(acc)
            acc += s[1] + GAP
        c.update(page_table=pt.tolist(), seq_lens=totals, q_starts=starts,
                 q_lens=[s[1] for s in specs], rows=acc)
    return cases


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
        "tests", "golden", "prefill_attn")
    os.makedirs(out_dir, exist_ok=True)
    assert torch.cuda.is_available() and ops.hip_available()
    gen = torch.Generator().manual_seed(20240521)
    kc = torch.randn(POOL_PAGES, N_KV, D // 8, PS, 8, generator=gen)
    vc = torch.randn(POOL_PAGES, N_KV, PS, D, generator=gen)
    pools = {"bf16": (kc.to(torch.bfloat16), vc.to(torch.bfloat16)),
             "fp8": (kc.to(torch.float8_e4m3fn), vc.to(torch.float8_e4m3fn))}
    for kind, (k, v) in pools.items():
        np_t = torch.int16 if kind == "bf16" else torch.uint8
        np.save(os.path.join(out_dir, f"k_cache_{kind}.npy"), k.view(np_t).numpy())
        np.save(os.path.join(out_dir, f"v_cache_{kind}.npy"), v.view(np_t).numpy())
    cases = build_cases()
    scale = 1.0 / math.sqrt(D)
    for name, c in cases.items():
        q = torch.randn(c["rows"], N_Q, D, generator=gen).to(torch.bfloat16)
        np.save(os.path.join(out_dir, f"{name}.q.npy"), q.view(torch.int16).numpy())
        dev = [torch.tensor(c[k], dtype=torch.int32, device="cuda")
               for k in ("page_table", "seq_lens", "q_starts", "q_lens")]
        for kind in (("bf16", "fp8") if c["fp8"] else ("bf16",)):
            k, v = pools[kind]
            out = torch.full((c["rows"], N_Q, D), SENTINEL, dtype=torch.int16,
                             device="cuda").view(torch.bfloat16)
            ops.paged_prefill_attention(out, q.cuda(), k.cuda(), v.cuda(), *dev,
                                        scale, c["max_qlen"])
            torch.cuda.synchronize()
            np.save(os.path.join(out_dir, f"{name}.out_{kind}.npy"),
                    out.view(torch.int16).cpu().numpy())
    meta = {"n_q": N_Q, "n_kv": N_KV, "head_dim": D, "page_size": PS,
            "sentinel": SENTINEL, "cases": cases}
    with open(os.path.join(out_dir, "cases.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print(f"recorded {len(cases)} cases into {out_dir}")


if __name__ == "__main__":
    main()
