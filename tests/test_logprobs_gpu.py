"""Logprobs kernel (csrc/logprobs.hip) on the MI355X against the CPU
definition (ops.reference.token_logprobs) on the same bf16 rows.

Ids must match exactly. Logprobs must match within ATOL = 1e-4: with
|logit| <= 64 an f32 logprob has an ulp of at most 7.6e-6, each __expf
term is off by a few 1e-6 relative for arguments down to -80, so the log
of the sum is off by about 1e-5 at worst; 1e-4 leaves under a tenfold
margin. Every test prints the largest error it saw (recorded in
profiles/README.md, "Per-token logprobs").
"""

import math
import tempfile

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs MI355X", allow_module_level=True)

from agentainer_amd import ops
from agentainer_amd.config import load_config
from agentainer_amd.engine.llm import GenRequest, LLMEngine
from agentainer_amd.ops import reference
from agentainer_amd.registry import Manager
from agentainer_amd.store import Store

DEV = "cuda"
ATOL = 1e-4
V_FULL = 128256
NEG_INF = float("-inf")


def _launch(logits_dev, rows, chosen, K):
    rows_t = torch.tensor(rows, dtype=torch.int32, device=DEV)
    chosen_t = torch.tensor(chosen, dtype=torch.int64, device=DEV)
    out = ops.token_logprobs(logits_dev, rows_t, chosen_t, K)
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in out)


def _compare(name, got, want):
    """Ids exact, logprobs within ATOL; returns the largest error."""
    (g_clp, g_id, g_lp), (w_clp, w_id, w_lp) = got, want
    assert g_id.dtype == torch.int32 and g_id.shape == w_id.shape
    pad = w_id < 0
    assert torch.equal(g_lp[pad], w_lp[pad])  # -inf in the same slots
    err = float((g_clp - w_clp).abs().max())
    if (~pad).any():
        err = max(err, float((g_lp[~pad] - w_lp[~pad]).abs().max()))
    print(f"[logprobs] {name}: max |err| = {err:.3e}")
    assert torch.equal(g_id, w_id), name
    assert err <= ATOL, (name, err)
    return err


def _check(name, logits, rows, chosen, K, logits_dev=None):
    """Kernel vs reference on the same rows; returns the kernel's output."""
    if logits_dev is None:
        logits_dev = logits.to(DEV)
    got = _launch(logits_dev, rows, chosen, K)
    want = reference.token_logprobs(
        logits, torch.tensor(rows, dtype=torch.int32),
        torch.tensor(chosen, dtype=torch.int64), K)
    _compare(name, got, want)
    return got


@pytest.fixture(scope="module")
def full_rows():
    """Case 1's inputs and reference, computed once: randn at scales 1
    and 4, B = 4, V = 128256, all rows, K = 20."""
    out = {}
    for scale in (1, 4):
        g = torch.Generator().manual_seed(scale)
        logits = (torch.randn(4, V_FULL, generator=g) * scale).to(torch.bfloat16)
        chosen = torch.randint(0, V_FULL, (4,), generator=g).tolist()
        want = reference.token_logprobs(
            logits, torch.arange(4, dtype=torch.int32),
            torch.tensor(chosen, dtype=torch.int64), 20)
        out[scale] = (logits, chosen, want)
    return out


@pytest.mark.parametrize("scale", [1, 4])
def test_full_size_rows_with_ties(full_rows, scale):
    logits, chosen, want = full_rows[scale]
    got = _launch(logits.to(DEV), [0, 1, 2, 3], chosen, 20)
    # bf16 randn repeats values among its top 20: the tie rule is at work
    top_vals = logits.float().gather(1, want[1].long())
    assert (top_vals[:, 1:] == top_vals[:, :-1]).any()
    err = _compare(f"full size, randn * {scale}", got, want)
    assert err <= 2e-5  # above this on randn, look for a bug


def test_two_launches_are_bit_identical(full_rows):
    logits, chosen, _ = full_rows[4]
    dev = logits.to(DEV)
    a = _launch(dev, [0, 1, 2, 3], chosen, 20)
    b = _launch(dev, [0, 1, 2, 3], chosen, 20)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_unaligned_rows_subset_and_order():
    V = 4099  # odd: rows 1 and 2 start off every vector boundary
    g = torch.Generator().manual_seed(7)
    logits = (torch.randn(3, V, generator=g) * 3).to(torch.bfloat16)
    logits[1] = 1000.0  # wins every comparison; must not be read
    got = _check("unaligned rows", logits, [2, 0], [5, 4000, 17], 5)
    assert torch.isfinite(got[0]).all() and (got[2] > -30).all()


# 40 tied ids: 0, V - 1, both sides of every 1024-id boundary and of the
# first fifteen 64-id boundaries (the kernel hands each wave 256 ids at
# this size, so 256, 512 and 768 are wave boundaries too)
TIE_V = 4099
TIE_IDS = sorted({0, TIE_V - 1}
                 | {b + d for b in range(64, 1024, 64) for d in (-1, 0)}
                 | {b + d for b in range(1024, TIE_V, 1024) for d in (-1, 0)})
BIG_IDS = (2000, 77, 3333)


def _tie_row(values):
    row = torch.full((TIE_V,), -3.0)
    for i, v in zip(BIG_IDS, (9.0, 8.0, 7.0)):
        row[i] = v
    row[TIE_IDS] = torch.tensor(values)
    return row.to(torch.bfloat16)[None]


@pytest.mark.parametrize("signed_zero", [False, True])
def test_threshold_ties_across_waves(signed_zero):
    assert len(TIE_IDS) == 40
    values = ([0.0 if j % 2 else -0.0 for j in range(40)] if signed_zero
              else [2.5] * 40)
    logits = _tie_row(values)
    name = "threshold ties" + (" (+0.0 / -0.0)" if signed_zero else "")
    _, ids, _ = _check(name, logits, [0], [0], 8)
    assert ids[0].tolist() == list(BIG_IDS) + TIE_IDS[:5]
    # 17 ties: the harvest crosses the waves' id ranges
    _, ids, _ = _check(name + ", K = 20", logits, [0], [TIE_V - 1], 20)
    assert ids[0].tolist() == list(BIG_IDS) + TIE_IDS[:17]


@pytest.mark.parametrize("V", [7, 1])
def test_small_vocab_pads(V):
    g = torch.Generator().manual_seed(V)
    logits = torch.randn(2, V, generator=g).to(torch.bfloat16)
    _, ids, lps = _check(f"V = {V}", logits, [1, 0], [0, V - 1], 20)
    assert (ids[:, V:] == -1).all() and (lps[:, V:] == NEG_INF).all()
    assert (ids[:, :V] >= 0).all() and torch.isfinite(lps[:, :V]).all()
    assert sorted(ids[0, :V].tolist()) == list(range(V))


def test_k_zero_and_k_one():
    V = 4104  # whole 16-byte vectors: greedy_sample's fast path
    g = torch.Generator().manual_seed(11)
    logits = (torch.randn(3, V, generator=g) * 2).to(torch.bfloat16)
    logits[2, 100] = logits[2, 3000] = 30.0  # tied argmax: lowest id
    dev = logits.to(DEV)
    chosen = [1, 2, 3]
    clp0, ids0, lps0 = _check("K = 0", logits, [0, 1, 2], chosen, 0, dev)
    assert ids0.shape == (3, 0) and lps0.shape == (3, 0)
    clp1, ids1, _ = _check("K = 1", logits, [0, 1, 2], chosen, 1, dev)
    assert torch.equal(clp0.view(torch.int32), clp1.view(torch.int32))
    greedy = torch.empty(3, dtype=torch.long, device=DEV)
    ops.greedy_sample(greedy, dev)
    assert ids1[:, 0].tolist() == greedy.cpu().tolist()
    assert ids1[2, 0] == 100


def test_peaked_row_is_finite():
    logits = torch.full((2, V_FULL), -40.0)
    logits[:, 70000] = 40.0
    logits = logits.to(torch.bfloat16)
    clp, ids, lps = _check("peaked row", logits, [0, 1], [70000, 5], 4)
    assert abs(float(clp[0])) < 1e-6
    assert abs(float(clp[1]) + 80.0) < ATOL
    assert ids.tolist() == [[70000, 0, 1, 2]] * 2
    assert torch.isfinite(lps).all() and (lps[:, 1:] + 80.0).abs().max() < ATOL


def test_chosen_outside_the_top_k():
    V = 4099
    g = torch.Generator().manual_seed(13)
    logits = (torch.randn(2, V, generator=g) * 4).to(torch.bfloat16)
    low = logits.float().argmin(dim=1).tolist()
    clp, ids, lps = _check("chosen outside the top K", logits, [0, 1], low, 3)
    for r in range(2):
        assert low[r] not in ids[r].tolist()
        assert float(clp[r]) < float(lps[r, 2])


def test_sliced_graph_buffer():
    """The logits as the first B rows of a larger buffer, which is what the
    decode graph's entry["logits"][:B] is."""
    V, B = 4099, 3
    g = torch.Generator().manual_seed(17)
    big = (torch.randn(8, V, generator=g) * 3).to(torch.bfloat16)
    big_dev = big.to(DEV)
    _check("sliced buffer", big[:B], [1, 2, 0], [9, 8, 7], 6,
           logits_dev=big_dev[:B])


# ---------------- engine on the device ----------------

def _engine(td):
    cfg = load_config(path="/nonexistent.yaml", env={})
    cfg.data["engine"]["sync_mode"] = True
    cfg.data["engine"]["kv_pool_gb"] = 1.0
    cfg.data["engine"]["async_decode"] = True
    st = Store(td + "/state", sync="never")
    eng = LLMEngine(st, cfg, device=DEV, state_root=td)
    return eng, Manager(st, eng, cfg), st


def test_engine_graph_async_decode_with_logprobs():
    """GPU tiny-llama, graph + async decode, three agents of staggered
    lengths; two ask for logprobs. The tokens are those of the run without
    the keys."""
    def specs(on):
        def lp(n):
            return {"logprobs": True, "top_logprobs": n} if on else {}
        return [(list(range(3, 43)), 8, 0.0, 0, lp(5)),
                (list(range(100, 120)), 5, 0.7, 123, {"top_k": 8, **lp(3)}),
                (list(range(7, 31)), 7, 0.0, 0, {})]
    results, state = [], None
    for on in (False, True):
        with tempfile.TemporaryDirectory() as td:
            eng, man, st = _engine(td)
            agents = []
            for i in range(3):
                a = man.deploy(name=f"l{i}", model="tiny-llama")
                man.start(a.id)
                agents.append(a)
            inst = eng._instances["tiny-llama"]
            assert inst.async_decode and inst.dev_decode
            if state is None:
                state = {k: v.clone() for k, v in inst.model.state_dict().items()}
            else:
                inst.model.load_state_dict(state)
            reqs = []
            for a, (prompt, n, temp, seed, ctl) in zip(agents, specs(on)):
                r = GenRequest(agent_id=a.id, prompt_tokens=list(prompt),
                               max_new=n, temperature=temp, top_p=0.9,
                               seed=seed, **ctl)
                b = inst.binding(a.id)
                with inst._lock:
                    b.queue.put(r)
                    inst._pump_agent(b)
                reqs.append(r)
            for _ in range(24):
                inst.step()
                if all(r.done.is_set() for r in reqs):
                    break
            inst.drain_async()
            torch.cuda.synchronize()
            for r in reqs:
                assert r.done.is_set() and not r.error, r.error
                assert r.generated
            results.append(([list(r.generated) for r in reqs],
                            [list(r.token_logprobs) for r in reqs]))
            eng.shutdown()
            st.close()
    (plain, none), (toks, lps) = results
    assert toks == plain, (toks, plain)
    assert none == [[], [], []] and lps[2] == []
    for row, n in ((0, 5), (1, 3)):
        assert len(lps[row]) == len(toks[row])
        for tok, e in zip(toks[row], lps[row]):
            assert e["token"] == tok and e["logprob"] <= 0.0
            tops = [t["logprob"] for t in e["top"]]
            assert len(tops) == n and tops == sorted(tops, reverse=True)
            assert all(p <= 0.0 for p in tops)
            assert sum(math.exp(p) for p in tops) <= 1.0 + 1e-3
    for e in lps[0]:  # greedy and unedited: the argmax was drawn
        assert e["top"][0]["token"] == e["token"]
        assert e["top"][0]["logprob"] == e["logprob"]
