"""Record the bit-exact fixture of tests/test_rope_append_golden.py.

python tools/record_rope_append_golden.py [out_dir]

Runs `ops.rope_append` of the CURRENT build on seeded inputs and writes the
qkv rows, the cos/sin table, and the resulting q rows and K/V pools as
raw-bit .npy files (bf16 as int16, fp8 as uint8) plus `cases.json`. Run it
on the commit whose arithmetic is the yardstick: the committed fixture under
tests/golden/rope_append/ was recorded with the one-thread-per-pair kernel
(2-byte accesses). Re-record only when the arithmetic is changed on
purpose.

T = 5 tokens, n_q 4 / n_kv 2 / head 128 / page 16, q, k and v strided views
of one qkv buffer. Positions 0, 1, a mid value and max_position - 1; slots:
the last slot of a page, the first of the next, one -1 (rotates q, appends
nothing). The pools start filled with a sentinel so that a stray store shows.
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from agentainer_amd import ops  # noqa: E402

T, N_Q, N_KV, D, PS = 5, 4, 2, 128, 16
POOL_PAGES = 3
MAX_POS = 64
POSITIONS = [0, 1, 37, MAX_POS - 1, 5]
SLOTS = [PS - 1, PS, -1, 2 * PS + 8, 2]
SENTINEL16 = 0x7B7B
SENTINEL8 = 0x7B


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
        "tests", "golden", "rope_append")
    os.makedirs(out_dir, exist_ok=True)
    assert torch.cuda.is_available() and ops.hip_available()
    gen = torch.Generator().manual_seed(20241022)
    qkv = torch.randn(T, (N_Q + 2 * N_KV) * D, generator=gen).to(torch.bfloat16)
    table = ops.make_cos_sin_table(MAX_POS, D, device="cpu").contiguous()
    np.save(os.path.join(out_dir, "qkv.npy"), qkv.view(torch.int16).numpy())
    np.save(os.path.join(out_dir, "cos_sin.npy"), table.numpy())
    pos = torch.tensor(POSITIONS, dtype=torch.int32, device="cuda")
    slots = torch.tensor(SLOTS, dtype=torch.long, device="cuda")
    for kind, dt, bits, fill in (("bf16", torch.bfloat16, torch.int16, SENTINEL16),
                                 ("fp8", torch.float8_e4m3fn, torch.uint8,
                                  SENTINEL8)):
        buf = qkv.cuda().clone()
        q = buf[:, :N_Q * D].view(T, N_Q, D)
        k = buf[:, N_Q * D:(N_Q + N_KV) * D].view(T, N_KV, D)
        v = buf[:, (N_Q + N_KV) * D:].view(T, N_KV, D)
        kc = torch.full((POOL_PAGES, N_KV, D // 8, PS, 8), fill, dtype=bits,
                        device="cuda").view(dt)
        vc = torch.full((POOL_PAGES, N_KV, PS, D), fill, dtype=bits,
                        device="cuda").view(dt)
        ops.rope_append(q, k, v, kc, vc, table.cuda(), pos, slots)
        torch.cuda.synchronize()
        np.save(os.path.join(out_dir, f"q_out_{kind}.npy"),
                q.contiguous().view(torch.int16).cpu().numpy())
        np.save(os.path.join(out_dir, f"k_cache_out_{kind}.npy"),
                kc.view(bits).cpu().numpy())
        np.save(os.path.join(out_dir, f"v_cache_out_{kind}.npy"),
                vc.view(bits).cpu().numpy())
    meta = {"T": T, "n_q": N_Q, "n_kv": N_KV, "head_dim": D, "page_size": PS,
            "pool_pages": POOL_PAGES, "max_position": MAX_POS,
            "positions": POSITIONS, "slots": SLOTS,
            "sentinel16": SENTINEL16, "sentinel8": SENTINEL8}
    with open(os.path.join(out_dir, "cases.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print(f"recorded rope_append fixture into {out_dir}")


if __name__ == "__main__":
    main()
