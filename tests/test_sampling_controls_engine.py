"""Per-request sampling controls through the engine (CPU).

The synchronous engine against the speculative one-step-lag engine
(`async_decode_emulate` runs the device-decode machinery on CPU tensors):
under async decode a carried-over row's newest token is still on the
device when the next sample launches, so the penalties must count it from
the gathered previous sample (ops.sample_ex's pending_tok), and under TP
the workers must rebuild the same edits from the OP_DECODE_ASYNC tail.
"""

import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

from agentainer_amd.config import load_config
from agentainer_amd.engine.llm import GenRequest, LLMEngine
from agentainer_amd.registry import Manager
from agentainer_amd.store import Store

# what the repetition-penalised row emits when nothing bans it, per model
BANNED = {"tiny-llama": 502, "tiny-llama-tp": 386}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _engine(tmp, tag, emulate, model="tiny-llama", extra=None):
    cfg = load_config(path="/nonexistent.yaml", env={})
    cfg.data["engine"]["sync_mode"] = True
    cfg.data["engine"]["kv_pool_gb"] = 0.02
    if emulate:
        cfg.data["engine"]["async_decode_emulate"] = True
    for k, v in (extra or {}).items():
        cfg.data["engine"][k] = v
    store = Store(os.path.join(tmp, f"{tag}-state"), sync="never")
    eng = LLMEngine(store, cfg, device="cpu", state_root=f"{tmp}/{tag}")
    return eng, Manager(store, eng, cfg), store


def _gen(eng, man, model, reqspecs, max_steps=80):
    """reqspecs: list of (prompt, max_new, temperature, seed, controls)."""
    agents, reqs = [], []
    for i, spec in enumerate(reqspecs):
        a = man.deploy(name=f"a{i}", model=model,
                       sampling={"max_tokens": spec[1]})
        man.start(a.id)
        agents.append(a)
    inst = eng._instances[model]
    for a, (prompt, max_new, temp, seed, controls) in zip(agents, reqspecs):
        r = GenRequest(agent_id=a.id, prompt_tokens=list(prompt),
                       max_new=max_new, temperature=temp, top_p=0.9,
                       seed=seed, **controls)
        b = inst.binding(a.id)
        with inst._lock:
            b.queue.put(r)
            inst._pump_agent(b)
        reqs.append(r)
    for _ in range(max_steps):
        inst.step()
        if all(r.done.is_set() for r in reqs):
            break
    if inst.async_decode:
        inst.drain_async()
    for r in reqs:
        assert r.done.is_set() and not r.error, r.error
    return [list(r.generated) for r in reqs]


GREEDY_PROMPT = list(range(3, 43))
# staggered lengths force mid-stream finishes => rollbacks
def _specs(model):
  return [
    # greedy + frequency penalty: every step's argmax depends on the
    # counts, the in-flight token included
    (GREEDY_PROMPT, 10, 0.0, 0, {"frequency_penalty": 2.0}),
    (list(range(100, 120)), 6, 0.7, 123, {"top_k": 8, "min_p": 0.05}),
    (list(range(50, 80)), 9, 0.0, 0,
     {"repetition_penalty": 1.3,
      "logit_bias": {BANNED[model]: -100.0, 5: 0.02}}),
    (list(range(7, 31)), 12, 0.0, 0, {}),  # plain: greedy_sample path
  ]


# the same rows with the penalty / the ban taken out
BASELINE_SPECS = [
    (GREEDY_PROMPT, 10, 0.0, 0, {}),
    (list(range(50, 80)), 9, 0.0, 0, {"repetition_penalty": 1.3}),
]


def _check_specs(got, baseline, model):
    assert all(len(t) > 0 for t in got)
    # the ban removes a token that is emitted without it
    assert BANNED[model] in baseline[1] and BANNED[model] not in got[2]
    # the penalty must bite, or the in-flight-token path is not exercised
    assert got[0] != baseline[0], (got[0], baseline[0])


def test_async_emulation_matches_sync_with_sampling_controls(tmp_path):
    tmp = str(tmp_path)
    e0, m0, s0 = _engine(tmp, "plain", emulate=False)
    baseline = _gen(e0, m0, "tiny-llama", BASELINE_SPECS)
    e0.shutdown(); s0.close()
    e1, m1, s1 = _engine(tmp, "sync", emulate=False)
    want = _gen(e1, m1, "tiny-llama", _specs("tiny-llama"))
    e1.shutdown(); s1.close()
    e2, m2, s2 = _engine(tmp, "async", emulate=True)
    got = _gen(e2, m2, "tiny-llama", _specs("tiny-llama"))
    inst = e2._instances["tiny-llama"]
    assert inst.async_decode and inst.dev_decode
    e2.shutdown(); s2.close()
    _check_specs(want, baseline, "tiny-llama")
    assert got == want, (got, want)


def test_forced_and_banned_tokens_through_the_engine(tmp_path):
    """logit_bias end to end: +100 forces every token, -100 on the token
    the plain run starts with removes it."""
    tmp = str(tmp_path)
    e, m, s = _engine(tmp, "bias", emulate=True)
    plain = _gen(e, m, "tiny-llama", [(GREEDY_PROMPT, 5, 0.0, 0, {})])[0]
    e.shutdown(); s.close()
    e, m, s = _engine(tmp, "bias2", emulate=True)
    got = _gen(e, m, "tiny-llama", [
        (GREEDY_PROMPT, 5, 0.0, 0, {"logit_bias": {plain[0]: -100.0}}),
        (GREEDY_PROMPT, 5, 0.8, 9, {"logit_bias": {300: 100.0}}),
    ])
    e.shutdown(); s.close()
    assert plain[0] not in got[0]
    assert got[1] == [300] * 5


# ---------------- TP world-2: the OP_DECODE_ASYNC tail ----------------

def _tp_worker(rank, world, port, tmp, result_file):
    os.environ.update({
        "RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank),
        "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
    import torch.distributed as dist

    from agentainer_amd import parallel as par

    par.init_distributed(backend="gloo")
    results = {}
    # identical shards in all runs; eager decode samples on rank 0 only,
    # async decode samples on every rank from the plan (and its tail)
    runs = (("plain", False, BASELINE_SPECS),
            ("eager", False, _specs("tiny-llama-tp")),
            ("async", True, _specs("tiny-llama-tp")))
    for mode, async_on, specs in runs:
        eng, man, store = _engine(tmp, f"tp-{mode}-r{rank}", emulate=True,
                                  model="tiny-llama-tp",
                                  extra={"tp_degree": world,
                                         "async_decode": async_on})
        if rank != 0:
            eng.run_worker()
            continue
        results[mode] = _gen(eng, man, "tiny-llama-tp", specs)
        assert eng._instances["tiny-llama-tp"].async_decode == async_on
        eng.shutdown()
    if rank == 0:
        torch.save(results, result_file)
    dist.barrier()


@pytest.mark.timeout(300)
def test_tp2_async_decode_token_exact_with_sampling_controls(tmp_path):
    """World-2 speculative decode vs eager decode with extended rows: the
    workers sample from the plan tail with their own pending token; a
    mismatch would desynchronise the ranks' KV and change rank 0's text."""
    tmp = str(tmp_path)
    result_file = os.path.join(tmp, "tp-ctl.pt")
    for attempt in range(2):
        port = _free_port()
        ctx = mp.get_context("spawn")
        procs = [ctx.Process(target=_tp_worker,
                             args=(r, 2, port, tmp, result_file))
                 for r in range(2)]
        for p in procs:
            p.start()
        codes = []
        for p in procs:
            p.join(timeout=240)
            codes.append(p.exitcode)
        for p in procs:
            if p.is_alive():
                p.terminate()
        if all(c == 0 for c in codes):
            break
        assert attempt == 0, f"worker exits {codes} (after retry)"
    res = torch.load(result_file, weights_only=True)
    _check_specs(res["eager"], res["plain"], "tiny-llama-tp")
    assert res["async"] == res["eager"], res


def test_plan_tail_round_trip_and_overflow():
    """The tail decodes to the specs it encoded; one too long for the plan
    vector is announced with n_ext = -1 and read from the stashed list."""
    from agentainer_amd.engine import llm, plan

    def rows(tops, ext):
        z = [0] * len(tops)
        return plan.AsyncDecodePlan(slots=z, feed=z, prev_idx=z, seeds=z,
                                    temps=[0.0] * len(tops), tops=tops,
                                    ext=ext)

    inst = llm.ModelInstance.__new__(llm.ModelInstance)
    inst._ext_tail = None
    ext = [None,
           (40, 0.05, 1.3, -0.5, 0.25, [(0, 1, 0.0), (7, 5, -100.0)]),
           None,
           (0, 0.0, 1.0, 0.0, 0.0, [(511, 0, 2.5)])]
    vec = plan.encode_async(0, "m", rows([1.0, 0.9, 1.0, 1.0], ext))
    assert vec[:4] == [llm.OP_DECODE_ASYNC, 0, 4, 0]
    n0 = 4 + 6 * 4
    assert vec[n0] == 2
    got = plan.decode_async(vec, inst._take_ext_tail).ext
    f32 = lambda x: torch.tensor(x, dtype=torch.float32).item()
    want = [None if sp is None else
            (sp[0], f32(sp[1]), f32(sp[2]), f32(sp[3]), f32(sp[4]), sp[5])
            for sp in ext]
    assert got == want
    # today's vector
    assert plan.decode_async(vec[:n0], inst._take_ext_tail).ext is None
    # overflow: the tail rides a pickled command instead
    sent = []
    big = [(1, 0.0, 1.1, 0.0, 0.0, [(t, 1, 0.0) for t in range(9000)])]
    real = llm.par.broadcast_obj
    llm.par.broadcast_obj = sent.append
    try:
        vec = plan.encode_async(0, "m", rows([1.0], big))
    finally:
        llm.par.broadcast_obj = real
    assert vec[-1] == -1 and len(vec) == 11 and sent[0][0] == "ext_tail"
    inst._ext_tail = sent[0][2]
    got = plan.decode_async(vec, inst._take_ext_tail).ext
    assert got[0][0] == 1 and got[0][5] == big[0][5]
    assert inst._ext_tail is None


# ---------------- Runtime / API: a bad value is a client error ----------------

def test_bad_top_k_is_a_client_error_and_fails_in_the_wal(tmp_path):
    from starlette.testclient import TestClient

    from agentainer_amd.api.server import create_app
    from agentainer_amd.service import Runtime

    cfg = load_config(path="/nonexistent.yaml", env={})
    root = str(tmp_path / "root")
    cfg.data["store"]["path"] = root
    cfg.data["engine"]["kv_pool_gb"] = 0.01
    s = Store(root + "/state", sync="interval")
    rt = Runtime(cfg, engine=LLMEngine(s, cfg, device="cpu", state_root=root),
                 store=s, state_root=root)
    try:
        a = rt.agents.deploy(name="ctl", model="tiny-llama",
                             sampling={"max_tokens": 4, "top_k": 20})
        rt.agents.start(a.id)
        for bad in ({"top_k": 5000}, {"logit_bias": {"512": 1.0}},
                    {"repetition_penalty": 0}):
            st, p = rt.agent_request(a.id, "POST", "/chat",
                                     body={"message": "hi", "sampling": bad})
            assert st == 400 and not p["success"], (st, p)
            assert p["data"]["status"] == "failed"
        allr = rt.requests.all_requests(a.id)
        assert len(allr["failed"]) == 3 and not allr["pending"]
        # the streaming path fails the entry too
        st, events = rt.agent_request_stream(
            a.id, body={"message": "hi", "sampling": {"top_k": -1}})
        evs = list(events)
        assert st == 200 and "error" in evs[-1] and "top_k" in evs[-1]["error"]
        allr = rt.requests.all_requests(a.id)
        assert len(allr["failed"]) == 4 and not allr["pending"]
        # through the HTTP surface, and a valid override still generates
        with TestClient(create_app(rt)) as client:
            r = client.post(f"/agent/{a.id}/chat",
                            json={"message": "hi", "sampling": {"top_k": 5000}})
            assert r.status_code == 400, r.text
            r = client.post(f"/agent/{a.id}/chat", json={
                "message": "hi", "sampling": {
                    "top_k": 5, "temperature": 0.8, "seed": 3,
                    "frequency_penalty": 0.5, "logit_bias": {"65": -100}}})
            assert r.status_code == 200, r.text
            assert r.json()["tokens"] > 0
        allr = rt.requests.all_requests(a.id)
        assert len(allr["failed"]) == 5 and not allr["pending"]
        assert len(allr["completed"]) == 1
    finally:
        rt.shutdown()
