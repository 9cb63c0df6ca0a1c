"""Record the bit-exact fixture of tests/test_decode_attn_golden.py.

python tools/record_decode_golden.py [out_dir]

Runs `ops.paged_decode_attention` of the CURRENT build on seeded inputs and
writes inputs and outputs as raw-bit .npy files (bf16 as int16, fp8 as
uint8) plus `cases.json` (page tables, lengths). Run it on the commit whose
arithmetic is the yardstick: the committed fixture under
tests/golden/decode_attn/ was recorded with the two-launch split-KV kernels
(partials to an HBM workspace + a combine kernel) that preceded the
single-launch kernel, and that kernel has to reproduce it bit for bit.
Re-record only when the arithmetic is changed on purpose.

Shapes are n_kv = 2 / head 128 / page 16. One 33-page KV pool (bf16 and its
fp8 twin) serves every case: a sequence's page-table row draws its pages
from the pool with repetition, so the longest case (1030 tokens, 65 pages)
needs no larger pool. Entries past a sequence's end point at random pages
too, so a kernel that reads a token it should have masked shows in the bits.
"""
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from agentainer_amd import ops  # noqa: E402

N_KV, D, PS = 2, 128, 16
POOL_PAGES = 33          # page 0 is the engine's scratch page
SENTINEL = 0x7B7B        # bf16 bits pre-filled into `out`

# lengths at the kernel's boundaries (64-token chunks, 8 splits)
LENGTHS = [1, 63, 64, 65, 320, 512, 513, 1030]
MIXED = [65, 0, 320, 1, 513, 1030]     # the 0 row: page table 0, never written
OTHER_RATIOS = {1: [65, 1030], 8: [320, 513]}


def build_cases():
    rng = np.random.RandomState(4321)
    cases = {}
    for n in LENGTHS:
        cases[f"r4_len{n}"] = {"ratio": 4, "seq_lens": [n]}
    cases["r4_mixed"] = {"ratio": 4, "seq_lens": list(MIXED)}
    for r, lens in OTHER_RATIOS.items():
        for n in lens:
            cases[f"r{r}_len{n}"] = {"ratio": r, "seq_lens": [n]}
    for c in cases.values():
        lens = c["seq_lens"]
        max_pages = max(1, max(-(-n // PS) for n in lens)) + 1
        pt = rng.randint(1, POOL_PAGES, size=(len(lens), max_pages))
        for b, n in enumerate(lens):
            if n == 0:
                pt[b, :] = 0
        c["page_table"] = pt.astype(np.int32).tolist()
    return cases


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
        "tests", "golden", "decode_attn")
    os.makedirs(out_dir, exist_ok=True)
    assert torch.cuda.is_available() and ops.hip_available()
    gen = torch.Generator().manual_seed(20241021)
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
        B, n_q = len(c["seq_lens"]), c["ratio"] * N_KV
        q = torch.randn(B, n_q, D, generator=gen).to(torch.bfloat16)
        np.save(os.path.join(out_dir, f"{name}.q.npy"), q.view(torch.int16).numpy())
        pt = torch.tensor(c["page_table"], dtype=torch.int32, device="cuda")
        sl = torch.tensor(c["seq_lens"], dtype=torch.int32, device="cuda")
        for kind, (k, v) in pools.items():
            out = torch.full((B, n_q, D), SENTINEL, dtype=torch.int16,
                             device="cuda").view(torch.bfloat16)
            ops.paged_decode_attention(out, q.cuda(), k.cuda(), v.cuda(), pt, sl,
                                       scale)
            torch.cuda.synchronize()
            np.save(os.path.join(out_dir, f"{name}.out_{kind}.npy"),
                    out.view(torch.int16).cpu().numpy())
    meta = {"n_kv": N_KV, "head_dim": D, "page_size": PS, "sentinel": SENTINEL,
            "cases": cases}
    with open(os.path.join(out_dir, "cases.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print(f"recorded {len(cases)} cases into {out_dir}")


if __name__ == "__main__":
    main()
