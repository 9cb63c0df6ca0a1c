"""Extended sampler kernel (csrc/sample_ex.hip) on the MI355X against the
CPU definition (ops.reference.sample_ex)."""

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


def _run(logits, temps, top_ps, seeds, top_ks, min_ps, reps, press, freqs,
         edits, pending=None):
    """ops.sample_ex on the GPU; returns (picks, edited f32 rows) on CPU."""
    B, V = logits.shape
    out = torch.full((B,), -7, dtype=torch.long, device=DEV)
    ws = torch.zeros(B * V, dtype=torch.float32, device=DEV)
    pend = None if pending is None else torch.tensor(pending, device=DEV)
    ops.sample_ex(out, logits.to(DEV), temps, top_ps, seeds, top_ks, min_ps,
                  reps, press, freqs, edits, pending=pend, ws=ws)
    torch.cuda.synchronize()
    return out.cpu(), ws.view(B, V).cpu()


def _off(B):
    """All-off extended parameters for B rows (temps, ..., edits)."""
    return dict(top_ps=[1.0] * B, seeds=[0] * B, top_ks=[0] * B,
                min_ps=[0.0] * B, reps=[1.0] * B, press=[0.0] * B,
                freqs=[0.0] * B, edits=[[] for _ in range(B)])


def test_argmax_matches_with_bf16_ties_lowest_id():
    B, V = 4, 128256
    g = torch.Generator().manual_seed(1)
    logits = torch.randn(B, V, generator=g).to(torch.bfloat16)
    out, ws = _run(logits, temps=[0.0] * B, **_off(B))
    lf = logits.float()
    want = [int((lf[b] == lf[b].max()).nonzero()[0]) for b in range(B)]
    # bf16 ties at the maximum are what makes the tie rule matter
    assert out.tolist() == want
    assert out.tolist() == lf.argmax(-1).tolist()
    assert torch.equal(ws, lf)  # no edits: the workspace is the widened row


# 1280 pairwise-distinct bf16 values, |x| in [0.5, 16)
_BITS = list(range(0x3F00, 0x4180))
_VALS = torch.tensor(_BITS + [b | 0x8000 for b in _BITS],
                     dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
KEPT_CASES = [  # (top_k, top_p, min_p, T) -> kept prefix length
    ((1024, 1.0, 0.0, 8.0), 1024),
    ((64, 0.9, 0.05, 1.0), 37),
    ((5, 1.0, 0.0, 2.0), 5),
    ((0, 0.95, 0.0, 1.5), 75),
]


@pytest.fixture(scope="module")
def distinct_row():
    V = 4099  # odd: rows after the first are unaligned, scalar head + tail
    g = torch.Generator().manual_seed(0)
    ids = torch.randperm(V, generator=g)[:_VALS.numel()]
    row = torch.full((V,), -30.0, dtype=torch.bfloat16)
    row[ids] = _VALS
    return row


@pytest.mark.parametrize("case,n_kept", KEPT_CASES)
def test_kept_set_and_draw(distinct_row, case, n_kept):
    """256 seeds per case: every pick lies in the float64 kept prefix and
    its CDF interval contains u. The 1e-3 margin is an error bound (<= 1024
    f32 additions of terms <= 1 plus __expf error, about 2e-4)."""
    top_k, top_p, min_p, T = case
    B = 256
    V = distinct_row.numel()
    ids, cum = reference.sample_ex_kept(distinct_row.float(), T, top_p, min_p,
                                        top_k)
    assert ids.numel() == n_kept
    cdf = (cum / cum[-1]).tolist()
    pos = {int(t): j for j, t in enumerate(ids.tolist())}
    logits = distinct_row.unsqueeze(0).expand(B, V).contiguous()
    seeds = [1000 + 7 * b for b in range(B)]
    kw = _off(B)
    kw.update(top_ps=[top_p] * B, seeds=seeds, top_ks=[top_k] * B,
              min_ps=[min_p] * B)
    out, _ = _run(logits, temps=[T] * B, **kw)
    outside = 0
    for b, pick in enumerate(out.tolist()):
        assert pick in pos, (b, pick)
        j = pos[pick]
        u = reference.uniform01(seeds[b], b)
        lo = cdf[j - 1] if j else 0.0
        outside += not (lo - 1e-3 <= u <= cdf[j] + 1e-3)
    print(f"case {case}: kept {n_kept}, {outside} of {B} draws outside")
    assert outside == 0
    if n_kept > 1:
        assert len(set(out.tolist())) > 1  # the seeds do move the draw


def test_all_equal_row_takes_lowest_ids():
    B, V = 8, 4096
    logits = torch.full((B, V), 0.75, dtype=torch.bfloat16)
    seeds = [31 * b + 5 for b in range(B)]
    kw = _off(B)
    kw.update(seeds=seeds, top_ks=[4] * B)
    out, _ = _run(logits, temps=[1.0] * B, **kw)
    want = torch.empty(B, dtype=torch.long)
    args = _csr_args([1.0] * B, kw)
    reference.sample_ex(want, logits, None, *args,
                        torch.full((B,), -1, dtype=torch.long))
    assert all(0 <= t < 4 for t in out.tolist()), out
    assert out.tolist() == want.tolist()
    assert len(set(out.tolist())) > 1


def _csr_args(temps, kw):
    """The tensor arguments of reference.sample_ex for the list-style kw."""
    ptr, tok, cnt, bias = [0], [], [], []
    for row in kw["edits"]:
        for t, c, b in row:
            tok.append(t); cnt.append(c); bias.append(b)
        ptr.append(len(tok))
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    return (f(temps), f(kw["top_ps"]), f(kw["min_ps"]), f(kw["reps"]),
            f(kw["press"]), f(kw["freqs"]),
            torch.tensor(kw["top_ks"], dtype=torch.int32),
            torch.tensor(kw["seeds"], dtype=torch.int64),
            torch.tensor(ptr, dtype=torch.int32),
            torch.tensor(tok, dtype=torch.int32),
            torch.tensor(cnt, dtype=torch.int32), f(bias))


def _edits_from_history(prompt, history, biases):
    """Unique (tok, 2*c + in_prompt, bias) rows from lists with duplicates."""
    toks = sorted(set(prompt) | set(history) | set(biases))
    return [(t, 2 * history.count(t) + (t in prompt), biases.get(t, 0.0))
            for t in toks]


@pytest.mark.parametrize("V", [1000, 128256])
def test_edits_match_reference(V):
    B = 4
    g = torch.Generator().manual_seed(V)
    logits = (torch.randn(B, V, generator=g) * 3).to(torch.bfloat16)
    top = logits.float().argmax(-1).tolist()
    edits = [
        # duplicates in the history, edits on id 0 and id V-1, the argmax
        # penalised away
        _edits_from_history([0, 5, 5, V - 1, top[0]],
                            [top[0], 7, 7, 7, V - 1, top[0], 0],
                            {3: 2.5, V - 1: -1.0}),
        [],  # an empty CSR segment between two rows with edits
        _edits_from_history([1, 2, top[2]], [top[2], 9, 9], {0: 100.0}),
        _edits_from_history([4], [top[3], top[3], 11], {top[3]: -100.0}),
    ]
    # pending: inside row 0's CSR, none, outside row 2's CSR, inside row 3's
    pending = [7, -1, 12, top[3]]
    kw = _off(B)
    kw.update(reps=[1.3, 1.0, 1.7, 1.1], press=[0.5, 0.0, -0.25, 1.0],
              freqs=[0.25, 0.0, 0.5, -0.5], edits=edits)
    temps = [0.0] * B
    out, ws = _run(logits, temps=temps, pending=pending, **kw)
    want = torch.empty(B, dtype=torch.long)
    want_ws = torch.zeros(B * V, dtype=torch.float32)
    reference.sample_ex(want, logits, want_ws, *_csr_args(temps, kw),
                        torch.tensor(pending))
    want_ws = want_ws.view(B, V)
    # exact, except within 1 ulp where the repetition rule divides
    up = torch.nextafter(want_ws, torch.full_like(want_ws, float("inf")))
    dn = torch.nextafter(want_ws, torch.full_like(want_ws, float("-inf")))
    assert bool(((ws >= dn) & (ws <= up)).all())
    differ = (ws != want_ws).nonzero()
    edited = {(b, t) for b in range(B) for t, c, _ in edits[b] if c > 0}
    edited |= {(b, p) for b, p in enumerate(pending) if p >= 0}
    assert all((int(b), int(t)) in edited for b, t in differ), differ
    print(f"V={V}: {len(differ)} edited logits 1 ulp off the reference")
    assert torch.equal(ws[1], logits[1].float())
    assert out.tolist() == want.tolist()
    assert out[0] != top[0] and out[2] == 0 and out[3] != top[3]


def test_same_inputs_same_outputs_with_tied_candidates():
    """bf16 randn at V=128256 puts equal-probability tokens inside and at
    the edge of the candidate set; two runs must agree, and match a run
    with the rows in another block order."""
    B, V = 8, 128256
    g = torch.Generator().manual_seed(3)
    row = torch.randn(V, generator=g).to(torch.bfloat16)
    logits = row.unsqueeze(0).expand(B, V).contiguous()
    kw = _off(B)
    kw.update(top_ps=[0.95] * B, seeds=list(range(40, 40 + B)),
              top_ks=[0, 0, 50, 50, 1024, 1024, 300, 300])
    temps = [1.5, 1.5, 1.0, 1.0, 4.0, 4.0, 0.7, 0.7]
    a, _ = _run(logits, temps=temps, **kw)
    b, _ = _run(logits, temps=temps, **kw)
    assert a.tolist() == b.tolist()
    # every pick is a candidate of the float64 definition: one of the
    # top-n0 by (p desc, id asc)
    lf = row.float()
    for r in range(B):
        n0 = kw["top_ks"][r] or 1024
        order = torch.sort(-lf.double(), stable=True).indices[:n0]
        assert int(a[r]) in set(order.tolist()), (r, int(a[r]))


def _engine(td, async_on):
    cfg = load_config(path="/nonexistent.yaml", env={})
    cfg.data["engine"]["sync_mode"] = True
    cfg.data["engine"]["kv_pool_gb"] = 1.0
    cfg.data["engine"]["async_decode"] = async_on
    st = Store(td + "/state", sync="never")
    eng = LLMEngine(st, cfg, device=DEV, state_root=td)
    return eng, Manager(st, eng, cfg), st


def test_engine_async_matches_sync_with_sampling_controls():
    """GPU tiny-llama, 4 agents with staggered lengths: graph replay, the
    gathered pending token and rollbacks give the synchronous tokens."""
    specs = [
        (list(range(3, 43)), 8, 0.0, 0, {"frequency_penalty": 2.0}),
        (list(range(100, 120)), 5, 0.7, 123, {"top_k": 8, "min_p": 0.05}),
        (list(range(50, 80)), 7, 0.0, 0,
         {"repetition_penalty": 1.3, "logit_bias": {17: -100.0, 5: 0.02}}),
        (list(range(7, 31)), 8, 0.0, 0, {}),
    ]
    results, state = [], None
    for async_on in (True, False):
        with tempfile.TemporaryDirectory() as td:
            eng, man, st = _engine(td, async_on)
            agents = []
            for i in range(len(specs)):
                a = man.deploy(name=f"c{i}", model="tiny-llama")
                man.start(a.id)
                agents.append(a)
            inst = eng._instances["tiny-llama"]
            assert inst.async_decode == async_on
            if state is None:
                state = {k: v.clone() for k, v in inst.model.state_dict().items()}
            else:
                inst.model.load_state_dict(state)
            reqs = []
            for a, (prompt, n, temp, seed, ctl) in zip(agents, specs):
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
            if inst.async_decode:
                inst.drain_async()
            torch.cuda.synchronize()
            for r in reqs:
                assert r.done.is_set() and not r.error, r.error
                assert r.generated
            results.append([list(r.generated) for r in reqs])
            eng.shutdown()
            st.close()
    assert results[0] == results[1], results
    assert 17 not in results[0][2]
