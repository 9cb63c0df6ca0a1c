"""Split-K reduction folded into the add+RMSNorm that consumes it.

The contract is bit-identity: partial-only skinny GEMM -> splitk_add_rmsnorm
must give exactly the out and residual of skinny GEMM (with combine) ->
fused_add_rmsnorm, at op level, through the model, and inside a captured
graph. Also covers the deferred workspace's lifetime guards."""

import pytest
import torch

from agentainer_amd import ops
from agentainer_amd.models.llama import (LLAMA_CONFIGS, AttnMetadata,
                                         LlamaForCausalLM)
from agentainer_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs MI355X", allow_module_level=True)


@pytest.fixture(autouse=True, scope="module")
def _require_hip():
    assert ops.hip_available(), "HIP extension must be present on the GPU box"


DEV = "cuda"
EPS = 1e-5

# (N = H, K, split, kc): H below one vector per thread; VPT 1 with the two
# split counts and k-chunks of the workload; VPT 2 (the 70B hidden size)
SHAPES = [(128, 512, 2, 128), (4096, 1024, 4, 128), (4096, 2048, 8, 256),
          (8192, 1024, 4, 128)]


def _inputs(M, N, K, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = (torch.randn(M, K, generator=g) * 0.1).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) * 0.1).to(torch.bfloat16)
    res = torch.randn(M, N, generator=g).to(torch.bfloat16)
    nw = torch.randn(N, generator=g).to(torch.bfloat16)
    return x, w, res, nw


def _both_paths(M, N, K, split, kc, x, w, res, nw):
    """(out, residual) of combine -> fused_add_rmsnorm and of partial-only ->
    splitk_add_rmsnorm, on the native entry points (no Python dispatch)."""
    mod = ops._load_hip()
    xd, nwd = x.to(DEV), nw.to(DEV)
    wp = ops.pack_weight(w.to(DEV))
    ws = torch.empty(split * M * N, dtype=torch.float32, device=DEV)

    gemm = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    mod.skinny_gemm_packed(gemm, xd, wp, N, K, ws, split, False, kc)
    res_a = res.to(DEV)
    out_a = torch.empty_like(res_a)
    mod.fused_add_rmsnorm(out_a, gemm, res_a, nwd, EPS)

    ws.fill_(float("nan"))  # the partial-only GEMM must rewrite every slab
    unwritten = torch.empty(0, dtype=torch.bfloat16, device=DEV)
    mod.skinny_gemm_packed(unwritten, xd, wp, N, K, ws, split, False, kc,
                           False)
    res_b = res.to(DEV)
    out_b = torch.empty_like(res_b)
    mod.splitk_add_rmsnorm(out_b, ws, split, M, N, res_b, nwd, EPS)
    return (out_a, res_a), (out_b, res_b)


@pytest.mark.parametrize("N,K,split,kc", SHAPES)
@pytest.mark.parametrize("M", [1, 17, 64])
def test_splitk_add_rmsnorm_bit_exact(M, N, K, split, kc):
    x, w, res, nw = _inputs(M, N, K, seed=1000 + M)
    (out_a, res_a), (out_b, res_b) = _both_paths(M, N, K, split, kc,
                                                 x, w, res, nw)
    assert torch.equal(res_b, res_a), "residual differs from combine path"
    assert torch.equal(out_b, out_a), "out differs from combine path"


def test_splitk_add_rmsnorm_unpacked_gemm_bit_exact():
    """The unpacked skinny GEMM's partial-only path feeds the same norm."""
    mod = ops._load_hip()
    M, N, K, split = 17, 4096, 1024, 4
    x, w, res, nw = _inputs(M, N, K, seed=7)
    xd, wd, nwd = x.to(DEV), w.to(DEV), nw.to(DEV)
    ws = torch.empty(split * M * N, dtype=torch.float32, device=DEV)
    gemm = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    mod.skinny_gemm(gemm, xd, wd, ws, split)
    res_a = res.to(DEV)
    out_a = torch.empty_like(res_a)
    mod.fused_add_rmsnorm(out_a, gemm, res_a, nwd, EPS)
    unwritten = torch.empty(0, dtype=torch.bfloat16, device=DEV)
    mod.skinny_gemm(unwritten, xd, wd, ws, split, False)
    res_b = res.to(DEV)
    out_b = torch.empty_like(res_b)
    mod.splitk_add_rmsnorm(out_b, ws, split, M, N, res_b, nwd, EPS)
    assert torch.equal(res_b, res_a) and torch.equal(out_b, out_a)


def test_splitk_add_rmsnorm_matches_fp32_reference():
    M, N, K, split, kc = 64, 4096, 1024, 4, 128
    x, w, res, nw = _inputs(M, N, K, seed=2)
    _, (out_b, res_b) = _both_paths(M, N, K, split, kc, x, w, res, nw)
    res_c = res.clone()
    want = torch.empty_like(res_c)
    ref.fused_add_rmsnorm(want, x.float() @ w.float().T, res_c, nw, EPS)
    assert torch.allclose(res_b.float().cpu(), res_c.float(), atol=0.02, rtol=0.02)
    assert torch.allclose(out_b.float().cpu(), want.float(), atol=0.02, rtol=0.02)


def test_splitk_add_rmsnorm_rejects_bad_arguments():
    mod = ops._load_hip()
    M, N, split = 4, 4096, 4
    res = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
    out = torch.empty_like(res)
    nw = torch.ones(N, dtype=torch.bfloat16, device=DEV)
    ws = torch.zeros(split * M * N, dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError):  # workspace one slab short
        mod.splitk_add_rmsnorm(out, ws[:-1], split, M, N, res, nw, EPS)
    with pytest.raises(RuntimeError):  # GEMM N is not the hidden size
        mod.splitk_add_rmsnorm(out, ws, split, M, N // 2, res, nw, EPS)
    with pytest.raises(RuntimeError):  # partials must be f32
        mod.splitk_add_rmsnorm(out, ws.to(torch.bfloat16), split, M, N, res,
                               nw, EPS)


# ---------------- model level: tiny-llama, skinny forced ----------------

PS = 16


@pytest.fixture(scope="module")
def tiny_model():
    model = LlamaForCausalLM(LLAMA_CONFIGS["tiny-llama"], device=DEV, seed=0)
    model.pack_decode_weights()
    return model


def _caches(cfg, n_pages):
    return [(torch.zeros(n_pages, cfg.n_kv_heads, cfg.head_dim // 8, PS, 8,
                         dtype=torch.bfloat16, device=DEV),
             torch.zeros(n_pages, cfg.n_kv_heads, PS, cfg.head_dim,
                         dtype=torch.bfloat16, device=DEV))
            for _ in range(cfg.n_layers)]


PREFILL_LENS = [23, 17]  # T = 40 <= 64: the prefill GEMMs take the skinny path
MAX_PAGES = 4
PAGE_TABLE = torch.tensor([[1, 2, 3, 4], [5, 6, 7, 8]], dtype=torch.int32)


def _slots(seq, positions):
    return [int(PAGE_TABLE[seq, p // PS]) * PS + p % PS for p in positions]


def _prefill_md():
    slots, pos, starts, acc = [], [], [], 0
    for b, n in enumerate(PREFILL_LENS):
        slots += _slots(b, range(n))
        pos += list(range(n))
        starts.append(acc)
        acc += n
    lens = torch.tensor(PREFILL_LENS, dtype=torch.int32, device=DEV)
    return AttnMetadata(
        page_table=PAGE_TABLE.to(DEV), seq_lens=lens,
        slot_mapping=torch.tensor(slots, dtype=torch.long, device=DEV),
        positions=torch.tensor(pos, dtype=torch.int32, device=DEV),
        is_prefill=True,
        query_starts=torch.tensor(starts, dtype=torch.int32, device=DEV),
        query_lens=lens.clone(), max_qlen=max(PREFILL_LENS))


def _decode_md(step):
    pos = [n + step for n in PREFILL_LENS]
    return AttnMetadata(
        page_table=PAGE_TABLE.to(DEV),
        seq_lens=torch.tensor([p + 1 for p in pos], dtype=torch.int32, device=DEV),
        slot_mapping=torch.tensor([_slots(b, [p])[0] for b, p in enumerate(pos)],
                                  dtype=torch.long, device=DEV),
        positions=torch.tensor(pos, dtype=torch.int32, device=DEV),
        is_prefill=False)


def _run_model(model, n_decode=3):
    """One prefill-shaped forward, then greedy decode forwards; all logits."""
    caches = _caches(model.cfg, 2 * MAX_PAGES + 1)
    g = torch.Generator(device="cpu").manual_seed(5)
    ids = torch.randint(3, model.cfg.vocab_size, (sum(PREFILL_LENS),),
                        generator=g).to(DEV)
    last = torch.tensor([PREFILL_LENS[0] - 1, sum(PREFILL_LENS) - 1], device=DEV)
    logits = [model(ids, _prefill_md(), caches, last)]
    for step in range(n_decode):
        nxt = logits[-1].float().argmax(-1)
        logits.append(model(nxt, _decode_md(step), caches, None))
    torch.cuda.synchronize()
    return logits, caches


@pytest.fixture()
def consumed(monkeypatch):
    """Counts the SplitKPartial handles the norm consumed."""
    calls = []
    orig = ops.SplitKPartial.consume

    def spy(self):
        calls.append(self.split)
        return orig(self)

    monkeypatch.setattr(ops.SplitKPartial, "consume", spy)
    return calls


def test_model_logits_equal_with_and_without_deferral(tiny_model, monkeypatch,
                                                     consumed):
    monkeypatch.setattr(ops, "SKINNY_FORCED", True)
    monkeypatch.setattr(ops, "SPLITK_DEFER_DISABLED", True)
    want, _ = _run_model(tiny_model)
    assert not consumed, "deferral switch must turn the handles off"
    monkeypatch.setattr(ops, "SPLITK_DEFER_DISABLED", False)
    got, _ = _run_model(tiny_model)
    # o-proj (split 2) and down-proj (split 4) of both layers, 4 forwards
    assert sorted(set(consumed)) == [2, 4] and len(consumed) == 16
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), f"logits differ at forward {i}"


def test_deferred_decode_captures_into_graph(tiny_model, monkeypatch, consumed):
    monkeypatch.setattr(ops, "SKINNY_FORCED", True)
    monkeypatch.setattr(ops, "SPLITK_DEFER_DISABLED", False)
    _, caches = _run_model(tiny_model, n_decode=0)  # prefill fills the caches
    ids = torch.tensor([11, 12], device=DEV)
    md = _decode_md(0)  # rewrites the same KV slots each time: idempotent
    eager = tiny_model(ids, md, caches, None).clone()
    torch.cuda.synchronize()
    del consumed[:]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = tiny_model(ids, md, caches, None)
    assert len(consumed) == 4, "the captured forward must use the deferred path"
    for _ in range(2):
        captured.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured, eager)


# ---------------- workspace lifetime ----------------

def test_stale_handle_raises(monkeypatch):
    monkeypatch.setattr(ops, "SKINNY_FORCED", True)
    monkeypatch.setattr(ops, "SPLITK_DEFER_DISABLED", False)
    M, N, K = 8, 512, 1024  # forced-skinny split 4
    x, w, res, nw = _inputs(M, N, K, seed=3)
    xd, wd, nwd = x.to(DEV), w.to(DEV), nw.to(DEV)
    handle = ops.linear_partial(xd, wd, ops.pack_weight(wd))
    assert isinstance(handle, ops.SplitKPartial) and handle.split == 4
    # consumed in time: equals the combining path
    res_a, res_b = res.to(DEV), res.to(DEV)
    out_a, out_b = torch.empty_like(res_a), torch.empty_like(res_b)
    ops.fused_add_rmsnorm(out_b, handle, res_b, nwd, EPS)
    ops.fused_add_rmsnorm(out_a, ops.linear(xd, wd, ops.pack_weight(wd)),
                          res_a, nwd, EPS)
    assert torch.equal(out_a, out_b) and torch.equal(res_a, res_b)
    # ops.linear above took the same (N, split) workspace: handle is stale now
    with pytest.raises(RuntimeError, match="stale"):
        ops.fused_add_rmsnorm(out_b, handle, res_b, nwd, EPS)


def test_workspace_keyed_by_stream():
    dev = torch.device("cuda", torch.cuda.current_device())
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        a = ops._skinny_ws(dev, 4096, 4)
        a_again = ops._skinny_ws(dev, 4096, 4)
    with torch.cuda.stream(s2):
        b = ops._skinny_ws(dev, 4096, 4)
    assert a_again is a, "one stream keeps reusing its workspace"
    assert b is not a and b.data_ptr() != a.data_ptr()
