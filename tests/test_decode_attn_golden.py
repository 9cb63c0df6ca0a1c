"""Paged decode attention, bit for bit against the two-launch kernels.

tests/golden/decode_attn/ was recorded by tools/record_decode_golden.py with
the split-KV pair that preceded the single-launch kernel (partials through an
HBM workspace, then a combine kernel). The single-launch kernel moves the
merge into LDS and reorders loads; the arithmetic of an output element may
not change, so every case must reproduce the fixture's bits. Lengths sit on
the kernel's boundaries (64-token chunks, 8 splits): 1, 63 / 64 / 65, 320
(five chunks, three empty waves), 512 (one chunk per wave), 513 (two chunks
per wave, three empty waves), 1030 (three per wave, ragged tail); RATIO 4
everywhere, RATIO 1 and 8 at two lengths each; one mixed batch with a
seq_len 0 row whose output must keep its sentinel. n_kv 2, head 128, page
16, page tables drawn at random from a 33-page pool, q a strided view of a
qkv buffer, bf16 and fp8 pages. Each case is also held to the tolerance
tests/test_gpu_ops.py uses for this op against the CPU reference (max abs
diff < 0.05). One case runs under graph capture with the lengths changed
between replays. All @pytest.mark.gpu."""

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
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                    "decode_attn")
with open(os.path.join(GOLD, "cases.json")) as _f:
    META = json.load(_f)
N_KV, D, PS = META["n_kv"], META["head_dim"], META["page_size"]
SENTINEL = META["sentinel"]
assert (N_KV, D, PS) == (2, 128, 16)
SCALE = 1.0 / math.sqrt(D)

LENGTHS = [1, 63, 64, 65, 320, 512, 513, 1030]
KINDS = ["bf16", "fp8"]


def _npy(name, dtype):
    return torch.from_numpy(np.load(os.path.join(GOLD, name))).view(dtype)


_pools = {}


def _pool(kind):
    """(cpu, device) copies of the shared pool, loaded once."""
    if kind not in _pools:
        dt = torch.bfloat16 if kind == "bf16" else torch.float8_e4m3fn
        kc, vc = _npy(f"k_cache_{kind}.npy", dt), _npy(f"v_cache_{kind}.npy", dt)
        _pools[kind] = (kc, vc, kc.to(DEV), vc.to(DEV))
    return _pools[kind]


def _strided_q(q):
    """q as the model passes it: a view of the fused qkv rows."""
    B, n_q = q.shape[0], q.shape[1]
    qkv = torch.randn(B, (n_q + 2 * N_KV) * D, dtype=torch.bfloat16, device=DEV)
    qkv[:, :n_q * D] = q.to(DEV).view(B, n_q * D)
    qd = qkv[:, :n_q * D].view(B, n_q, D)
    assert not qd.is_contiguous() or B == 1
    return qd


def _run(name, kind):
    """Launch one fixture case; returns the raw bits of `out` (int16, CPU)."""
    c = META["cases"][name]
    _, _, kc, vc = _pool(kind)
    q = _npy(f"{name}.q.npy", torch.bfloat16)
    assert q.shape[1] == c["ratio"] * N_KV
    out = torch.full(tuple(q.shape), SENTINEL, dtype=torch.int16,
                     device=DEV).view(torch.bfloat16)
    pt = torch.tensor(c["page_table"], dtype=torch.int32, device=DEV)
    sl = torch.tensor(c["seq_lens"], dtype=torch.int32, device=DEV)
    ops.paged_decode_attention(out, _strided_q(q), kc, vc, pt, sl, SCALE)
    torch.cuda.synchronize()
    return out.view(torch.int16).cpu()


_ref_cache = {}


def _reference(name, kind):
    """CPU fp32 reference, computed once per case and left unchanged."""
    if (name, kind) not in _ref_cache:
        c = META["cases"][name]
        kc, vc, _, _ = _pool(kind)
        q = _npy(f"{name}.q.npy", torch.bfloat16)
        want = torch.zeros(tuple(q.shape), dtype=torch.bfloat16)
        ref.paged_decode_attention(
            want, q, kc, vc, torch.tensor(c["page_table"], dtype=torch.int32),
            torch.tensor(c["seq_lens"], dtype=torch.int32), SCALE)
        _ref_cache[(name, kind)] = want
    return _ref_cache[(name, kind)]


def _check(name, kind, bits):
    c = META["cases"][name]
    live = torch.tensor(c["seq_lens"]) > 0
    want = _reference(name, kind)
    got = bits.view(torch.bfloat16)
    diff = (got[live].float() - want[live].float()).abs().max().item()
    print(f"{name}/{kind}: max abs diff vs reference {diff:.5f}")
    assert diff < 0.05, f"decode attn max abs diff {diff} ({name}/{kind})"
    assert bool((bits[~live] == SENTINEL).all()), \
        f"{name}/{kind}: a seq_len 0 row was written"
    gold = _npy(f"{name}.out_{kind}.npy", torch.int16)
    nbad = int((bits != gold).sum())
    assert torch.equal(bits, gold), \
        f"{name}/{kind}: {nbad} of {bits.numel()} output bits differ from the fixture"


GOLDEN = [(name, kind) for name in sorted(META["cases"]) for kind in KINDS]


def test_fixture_covers_the_cases():
    cases = META["cases"]
    for n in LENGTHS:
        c = cases[f"r4_len{n}"]
        assert c["ratio"] == 4 and c["seq_lens"] == [n]
    for r in (1, 8):
        lens = sorted(c["seq_lens"][0] for name, c in cases.items()
                      if c["ratio"] == r)
        assert len(lens) == 2, (r, lens)
    mixed = cases["r4_mixed"]
    assert mixed["ratio"] == 4 and len(mixed["seq_lens"]) >= 4
    z = mixed["seq_lens"].index(0)
    assert mixed["page_table"][z] == [0] * len(mixed["page_table"][z])
    for c in cases.values():  # shuffled, non-monotone page tables
        row = [p for p in c["page_table"][0] if p]
        assert len(row) < 3 or sorted(row) != row
    for f in os.listdir(GOLD):  # nothing larger than the prefill fixture's files
        assert os.path.getsize(os.path.join(GOLD, f)) <= 275584, f


@pytest.mark.parametrize("name,kind", GOLDEN)
def test_bit_equal_to_recorded_kernels(name, kind):
    _check(name, kind, _run(name, kind))


@pytest.mark.parametrize("kind", KINDS)
def test_graph_capture_with_changing_lengths(kind):
    """The launch sits in the captured decode step and allocates nothing:
    capture once, then replay with other lengths, page tables and q."""
    names = ["r4_len1030", "r4_len320", "r4_len1", "r4_len513", "r4_len1030"]
    cases = META["cases"]
    width = max(len(cases[n]["page_table"][0]) for n in names)
    n_q = 4 * N_KV
    _, _, kc, vc = _pool(kind)
    qkv = torch.zeros(1, (n_q + 2 * N_KV) * D, dtype=torch.bfloat16, device=DEV)
    q = qkv[:, :n_q * D].view(1, n_q, D)
    out = torch.zeros(1, n_q, D, dtype=torch.bfloat16, device=DEV)
    pt = torch.zeros(1, width, dtype=torch.int32, device=DEV)
    sl = torch.zeros(1, dtype=torch.int32, device=DEV)

    def load(name):
        c = cases[name]
        row = c["page_table"][0]
        pt.zero_()
        pt[0, :len(row)] = torch.tensor(row, dtype=torch.int32, device=DEV)
        sl[0] = c["seq_lens"][0]
        q.copy_(_npy(f"{name}.q.npy", torch.bfloat16).to(DEV))
        out.view(torch.int16).fill_(SENTINEL)

    load(names[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.paged_decode_attention(out, q, kc, vc, pt, sl, SCALE)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.paged_decode_attention(out, q, kc, vc, pt, sl, SCALE)
    for name in names:
        load(name)
        graph.replay()
        torch.cuda.synchronize()
        bits = out.view(torch.int16).cpu()
        gold = _npy(f"{name}.out_{kind}.npy", torch.int16)
        assert torch.equal(bits, gold), f"replay {name}/{kind} differs"
