"""Paged prefill attention at its tile boundaries (gfx950 HIP kernel).

Small shapes around every boundary of the kernel's geometry (32-row q
tile of two 16-row sub-tiles, 32-token KV tile, 16-token pages): q lengths
just below and above a tile, a diagonal that falls mid-tile, a cached
prefix that crosses page and tile boundaries, varlen batches with
early-exit blocks, the engine's pad row, fp8 pages and the model's strided
q view. Every case is checked against the CPU reference (and that rows
the kernel must not write keep their sentinel); the n_q = 4 cases are also
compared bit for bit with tests/golden/prefill_attn/, recorded by
tools/record_prefill_golden.py with the kernel that preceded the latency
rewrite: data movement may change, the arithmetic of an output element
may not. All @pytest.mark.gpu."""

import json
import math
import os

import numpy as np
import pytest
import torch

from agentainer_amd import ops
from agentainer_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs MI355X", allow_module_level=True)


@pytest.fixture(autouse=True, scope="module")
def _require_hip():
    assert ops.hip_available(), "HIP extension must be present on the GPU box"


DEV = "cuda"
D, PS = 128, 16
SENTINEL = 0x7B7B
GAP = 3  # unused rows after every sequence
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                    "prefill_attn")
with open(os.path.join(GOLD, "cases.json")) as _f:
    META = json.load(_f)
assert (META["head_dim"], META["page_size"], META["sentinel"]) == (D, PS, SENTINEL)

SINGLES = [(0, 1), (0, 31), (0, 33), (0, 97), (5, 64), (37, 130), (300, 20)]
VARLEN = [(0, 1), (16, 16), (64, 200), (0, 40)]      # max_qlen 200
PADROW = [(10, 50), ("pad", 48)]                     # last row: page table 0


def _run(q, kc, vc, page_table, seq_lens, q_starts, q_lens, max_qlen,
         strided=False):
    """Launch on the GPU; returns the raw bits of `out` (int16, CPU)."""
    rows, n_q = q.shape[0], q.shape[1]
    qd = q.to(DEV)
    if strided:  # q as the model passes it: a view of the fused qkv rows
        n_kv = kc.shape[1]
        qkv = torch.randn(rows, (n_q + 2 * n_kv) * D, dtype=torch.bfloat16,
                          device=DEV)
        qkv[:, :n_q * D] = qd.view(rows, n_q * D)
        qd = qkv[:, :n_q * D].view(rows, n_q, D)
        assert not qd.is_contiguous()
    out = torch.full((rows, n_q, D), SENTINEL, dtype=torch.int16,
                     device=DEV).view(torch.bfloat16)
    ints = [torch.tensor(x, dtype=torch.int32, device=DEV)
            for x in (page_table, seq_lens, q_starts, q_lens)]
    ops.paged_prefill_attention(out, qd, kc.to(DEV), vc.to(DEV), *ints,
                                1.0 / math.sqrt(D), max_qlen)
    torch.cuda.synchronize()
    return out.view(torch.int16).cpu()


_ref_cache = {}


def _reference(key, q, kc, vc, page_table, seq_lens, q_starts, q_lens):
    """CPU fp32 reference, computed once per case and left unchanged."""
    if key not in _ref_cache:
        want = torch.zeros(q.shape, dtype=torch.bfloat16)
        ref.paged_prefill_attention(
            want, q, kc, vc, torch.tensor(page_table, dtype=torch.int32),
            torch.tensor(seq_lens, dtype=torch.int32),
            torch.tensor(q_starts, dtype=torch.int32),
            torch.tensor(q_lens, dtype=torch.int32), 1.0 / math.sqrt(D))
        _ref_cache[key] = want
    return _ref_cache[key]


def _check_reference(key, bits, q, kc, vc, page_table, seq_lens, q_starts,
                     q_lens):
    want = _reference(key, q, kc, vc, page_table, seq_lens, q_starts, q_lens)
    got = bits.view(torch.bfloat16)
    written = torch.zeros(q.shape[0], dtype=torch.bool)
    for s, n in zip(q_starts, q_lens):
        written[s:s + n] = True
    diff = (got[written].float() - want[written].float()).abs().max().item()
    print(f"{key}: max abs diff vs reference {diff:.5f}")
    assert diff < 0.05, f"prefill attn max abs diff {diff} ({key})"
    assert bool((bits[~written] == SENTINEL).all()), \
        f"{key}: rows outside every sequence were written"


# ---------------------------------------------------------------- fixture


def _npy(name, dtype):
    return torch.from_numpy(np.load(os.path.join(GOLD, name))).view(dtype)


_pools = {}


def _pool(kind):
    if kind not in _pools:
        dt = torch.bfloat16 if kind == "bf16" else torch.float8_e4m3fn
        _pools[kind] = (_npy(f"k_cache_{kind}.npy", dt),
                        _npy(f"v_cache_{kind}.npy", dt))
    return _pools[kind]


GOLDEN = [(name, kind) for name, c in sorted(META["cases"].items())
          for kind in (("bf16", "fp8") if c["fp8"] else ("bf16",))]


def _golden_case(name, kind, strided=False):
    c = META["cases"][name]
    kc, vc = _pool(kind)
    assert (META["n_q"], META["n_kv"]) == (4, kc.shape[1])
    q = _npy(f"{name}.q.npy", torch.bfloat16)
    geom = (c["page_table"], c["seq_lens"], c["q_starts"], c["q_lens"])
    bits = _run(q, kc, vc, *geom, c["max_qlen"], strided=strided)
    _check_reference(f"golden/{name}/{kind}", bits, q, kc, vc, *geom)
    want = _npy(f"{name}.out_{kind}.npy", torch.int16)
    nbad = int((bits != want).sum())
    assert torch.equal(bits, want), \
        f"{name}/{kind}: {nbad} of {bits.numel()} output bits differ from the fixture"


def test_fixture_covers_the_cases():
    cases = META["cases"]
    for ctx, new in SINGLES:
        c = cases[f"c{ctx}_n{new}"]
        assert c["specs"] == [[ctx, new]] and c["fp8"]
    assert cases["varlen"]["specs"] == [list(s) for s in VARLEN]
    assert cases["varlen"]["max_qlen"] == 200
    assert cases["padrow"]["specs"] == [list(s) for s in PADROW]
    assert cases["padrow"]["page_table"][-1] == [0] * len(cases["padrow"]["page_table"][-1])
    for c in cases.values():  # shuffled, non-monotone page tables
        row = [p for p in c["page_table"][0] if p]
        assert len(row) < 3 or sorted(row) != row


@pytest.mark.parametrize("name,kind", GOLDEN)
def test_bit_equal_to_recorded_kernel(name, kind):
    _golden_case(name, kind)


def test_strided_q_view_bit_equal():
    _golden_case("c37_n130", "bf16", strided=True)
    _golden_case("varlen", "bf16", strided=True)


# ------------------------------------------------------- generated shapes


def _make(specs, n_q, n_kv, kind, seed):
    """Random pool (random past every sequence's end too), shuffled page
    table, GAP unused rows after each sequence."""
    gen = torch.Generator().manual_seed(seed)
    totals = [s[1] if s[0] == "pad" else s[0] + s[1] for s in specs]
    need = sum(-(-t // PS) for s, t in zip(specs, totals) if s[0] != "pad")
    pool_pages = need + 4
    dt = torch.bfloat16 if kind == "bf16" else torch.float8_e4m3fn
    kc = torch.randn(pool_pages, n_kv, D // 8, PS, 8, generator=gen).to(dt)
    vc = torch.randn(pool_pages, n_kv, PS, D, generator=gen).to(dt)
    perm = (torch.randperm(pool_pages - 1, generator=gen) + 1).tolist()
    max_pages = max(-(-t // PS) for t in totals)
    page_table = [[0] * max_pages for _ in specs]
    for b, (s, t) in enumerate(zip(specs, totals)):
        if s[0] != "pad":
            for i in range(-(-t // PS)):
                page_table[b][i] = perm.pop()
    q_starts, acc = [], 0
    for s in specs:
        q_starts.append(acc)
        acc += s[1] + GAP
    q = torch.randn(acc, n_q, D, generator=gen).to(torch.bfloat16)
    return q, kc, vc, page_table, totals, q_starts, [s[1] for s in specs]


def _generated_case(key, specs, n_q, n_kv, kind, max_qlen, seed, strided=False):
    q, kc, vc, *geom = _make(specs, n_q, n_kv, kind, seed)
    bits = _run(q, kc, vc, *geom, max_qlen, strided=strided)
    _check_reference(key, bits, q, kc, vc, *geom)


@pytest.mark.parametrize("ctx,new", SINGLES)
@pytest.mark.parametrize("n_q,n_kv", [(4, 1), (8, 1), (8, 2)])
@pytest.mark.parametrize("kind", ["bf16", "fp8"])
def test_single_sequence_matches_reference(kind, n_q, n_kv, ctx, new):
    _generated_case(f"single/{kind}/{n_q}-{n_kv}/c{ctx}_n{new}", [(ctx, new)],
                    n_q, n_kv, kind, new, seed=1000 + 7 * ctx + new)


@pytest.mark.parametrize("n_q,n_kv", [(4, 1), (8, 1), (8, 2)])
def test_varlen_batch_matches_reference(n_q, n_kv):
    _generated_case(f"varlen/{n_q}-{n_kv}", VARLEN, n_q, n_kv, "bf16", 200,
                    seed=21)


@pytest.mark.parametrize("n_q,n_kv", [(4, 1), (8, 1), (8, 2)])
def test_pad_row_batch_matches_reference(n_q, n_kv):
    _generated_case(f"padrow/{n_q}-{n_kv}", PADROW, n_q, n_kv, "bf16", 50,
                    seed=22)


def test_llama_heads_strided_matches_reference():
    # n_q = 32 / n_kv = 8 (ratio 4), q a view of the qkv buffer
    _generated_case("llama/c37_n130", [(37, 130)], 32, 8, "bf16", 130, seed=23,
                    strided=True)


def test_max_qlen_fallback_matches_reference():
    # max_qlen <= 0: the binding derives it from query_lens
    _generated_case("fallback/varlen", VARLEN, 8, 2, "bf16", 0, seed=24)
