"""rope_append, bit for bit against the one-thread-per-pair kernel.

tests/golden/rope_append/ was recorded by tools/record_rope_append_golden.py
with the kernel that rotates one pair per thread on 2-byte accesses. Any
rewrite of it (a 16-byte form was tried: profiles/README.md) has to leave
the same bits in q, in every touched element of the K and V pools, and the
sentinel in every untouched one. Five tokens cannot show a one-ulp f32
difference that bf16 rounding hides in all but one value in 2^16: a rewrite
must also leave bench.py's output dumps equal. T = 5 tokens,
n_q 4 / n_kv 2 / head 128 / page 16, q, k and v strided views of one qkv
buffer; positions 0, 1, a mid value and max_position - 1; slots: the last
slot of a page, the first of the next, and one -1 (q is rotated, nothing is
appended). bf16 and fp8 pools. All @pytest.mark.gpu."""

import json
import os

import numpy as np
import pytest
import torch

from agentainer_amd import ops

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs MI355X", allow_module_level=True)


@pytest.fixture(autouse=True, scope="module")
def _require_hip():
    assert ops.hip_available(), "HIP extension must be present on the GPU box"


DEV = "cuda"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                    "rope_append")
with open(os.path.join(GOLD, "cases.json")) as _f:
    META = json.load(_f)
T, N_Q, N_KV = META["T"], META["n_q"], META["n_kv"]
D, PS, POOL = META["head_dim"], META["page_size"], META["pool_pages"]


def _npy(name):
    return torch.from_numpy(np.load(os.path.join(GOLD, name)))


def test_fixture_covers_the_cases():
    assert (T, N_Q, N_KV, D, PS) == (5, 4, 2, 128, 16)
    pos, slots = META["positions"], META["slots"]
    assert {0, 1, META["max_position"] - 1} <= set(pos)
    assert any(1 < p < META["max_position"] - 1 for p in pos)
    assert -1 in slots
    assert any(s >= 0 and s % PS == PS - 1 and s + 1 in slots for s in slots)


@pytest.mark.parametrize("kind", ["bf16", "fp8"])
def test_bit_equal_to_recorded_kernel(kind):
    dt, bits, fill = ((torch.bfloat16, torch.int16, META["sentinel16"])
                      if kind == "bf16" else
                      (torch.float8_e4m3fn, torch.uint8, META["sentinel8"]))
    buf = _npy("qkv.npy").view(torch.bfloat16).to(DEV)
    q = buf[:, :N_Q * D].view(T, N_Q, D)
    k = buf[:, N_Q * D:(N_Q + N_KV) * D].view(T, N_KV, D)
    v = buf[:, (N_Q + N_KV) * D:].view(T, N_KV, D)
    assert not q.is_contiguous() and not k.is_contiguous()
    kc = torch.full((POOL, N_KV, D // 8, PS, 8), fill, dtype=bits,
                    device=DEV).view(dt)
    vc = torch.full((POOL, N_KV, PS, D), fill, dtype=bits, device=DEV).view(dt)
    table = _npy("cos_sin.npy").to(DEV)
    pos = torch.tensor(META["positions"], dtype=torch.int32, device=DEV)
    slots = torch.tensor(META["slots"], dtype=torch.long, device=DEV)
    kv_before = buf[:, N_Q * D:].clone()
    ops.rope_append(q, k, v, kc, vc, table, pos, slots)
    torch.cuda.synchronize()
    assert torch.equal(buf[:, N_Q * D:], kv_before), "k / v rows were modified"
    got_q = q.contiguous().view(torch.int16).cpu()
    got_k, got_v = kc.view(bits).cpu(), vc.view(bits).cpu()
    want_q = _npy(f"q_out_{kind}.npy")
    want_k = _npy(f"k_cache_out_{kind}.npy")
    want_v = _npy(f"v_cache_out_{kind}.npy")
    # the fixture itself: appended slots differ from the sentinel somewhere,
    # every other slot is all sentinel
    live = sorted(s for s in META["slots"] if s >= 0)
    touched = torch.zeros(POOL * PS, dtype=torch.bool)
    touched[live] = True
    rows_v = (want_v != fill).any(dim=-1).any(dim=1).reshape(-1)  # [page*PS]
    assert torch.equal(rows_v, touched)
    assert torch.equal(got_q, want_q), \
        f"{int((got_q != want_q).sum())} q bits differ from the fixture"
    assert torch.equal(got_k, want_k), \
        f"{int((got_k != want_k).sum())} K pool elements differ from the fixture"
    assert torch.equal(got_v, want_v), \
        f"{int((got_v != want_v).sum())} V pool elements differ from the fixture"
