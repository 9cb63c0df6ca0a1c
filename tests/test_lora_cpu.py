"""Per-agent LoRA adapters, CPU side: the fp32 reference ops, the fused-
projection stacking, the adapter loader, the engine (pool slots, ids per
row, stop/resume, slot exhaustion, disabled config), prefix sharing keyed
by adapter, and the `lora` field through YAML / API / backup."""

import json
import os

import pytest
import torch

from agentainer_amd import ops
from agentainer_amd.config import load_config, load_deployment
from agentainer_amd.engine.llm import LLMEngine
from agentainer_amd.models.llama import LLAMA_CONFIGS
from agentainer_amd.models.lora import (LoraError, LoraPool, check_max_rank,
                                        load_adapter, stack_pairs)
from agentainer_amd.ops import reference
from agentainer_amd.registry import Manager
from agentainer_amd.registry.agent import FAILED, RUNNING
from agentainer_amd.store import Store

from lora_fixtures import (adapter_tensors, gen_tokens, module_dims,
                           write_adapter)

CFG = LLAMA_CONFIGS["tiny-llama"]
PROMPT = list(range(3, 35))
# adapter seeds for the engine tests: chosen so that adapter X changes the
# greedy continuation of PROMPT on the seed-0 random-init tiny-llama
SEED_X, SEED_Y, SEED_Z = 11, 12, 13


# ------------------------------------------------------------ reference ops

IDS_CASES = {
    "pad_rows": [-1, 0, -1, 2, 2, -1],
    "repeats": [1, 1, 1, 3, 3, 0],
    "all_distinct": [3, 1, 0, 2],
    "all_base": [-1, -1, -1],
}


@pytest.mark.parametrize("case", sorted(IDS_CASES))
def test_reference_ops_match_plain_fp32_math(case):
    ids_l = IDS_CASES[case]
    T, K, N, R, S = len(ids_l), 64, 40, 8, 4
    g = torch.Generator().manual_seed(1)
    x = torch.randn(T, K, generator=g).bfloat16()
    y0 = torch.randn(T, N, generator=g).bfloat16()
    A = (torch.randn(S, R, K, generator=g) / K ** 0.5).bfloat16()
    B = (torch.randn(S, N, R, generator=g) / R ** 0.5).bfloat16()
    ids = torch.tensor(ids_l, dtype=torch.int32)

    v = torch.full((T, R), 7.0)
    reference.lora_shrink(v, x, A, ids)
    y = y0.clone()
    reference.lora_expand_add(y, v, B, ids)
    for t, i in enumerate(ids_l):
        if i < 0:
            assert torch.equal(v[t], torch.zeros(R))
            assert torch.equal(y[t], y0[t])
            continue
        v_t = torch.stack([(A[i, r].float() * x[t].float()).sum()
                           for r in range(R)])
        assert torch.allclose(v[t], v_t, rtol=1e-5, atol=1e-6)
        y_t = torch.stack([y0[t, n].float() + (B[i, n].float() * v_t).sum()
                           for n in range(N)])
        # one bf16 rounding of the result
        assert torch.allclose(y[t].float(), y_t, rtol=2 ** -7, atol=1e-3)

    # ops.* on CPU tensors dispatch to the same references; lora_apply is
    # shrink + expand-add
    y2 = y0.clone()
    ops.lora_apply(y2, x, A, B, ids)
    assert torch.equal(y2, y)
    v2 = torch.empty(T, R)
    assert torch.equal(ops.lora_shrink(v2, x, A, ids), v)


def test_lora_apply_empty_batch():
    y = torch.empty(0, 16, dtype=torch.bfloat16)
    x = torch.empty(0, 256, dtype=torch.bfloat16)
    A = torch.zeros(2, 8, 256, dtype=torch.bfloat16)
    B = torch.zeros(2, 16, 8, dtype=torch.bfloat16)
    assert ops.lora_apply(y, x, A, B, torch.empty(0, dtype=torch.int32)) is y


# ----------------------------------------------------------------- stacking

@pytest.mark.parametrize("proj,mods", [("qkv", ("q_proj", "k_proj", "v_proj")),
                                       ("gate_up", ("gate_proj", "up_proj"))])
def test_stacked_delta_equals_concatenated_deltas(proj, mods):
    r, max_rank, alpha = 4, 8, 6.0
    dims = module_dims(CFG)
    K = dims[mods[0]][0]
    outs = [dims[m][1] for m in mods]
    g = torch.Generator().manual_seed(2)
    pairs = [(torch.randn(r, K, generator=g) / K ** 0.5,
              torch.randn(n, r, generator=g) / r ** 0.5) for n in outs]
    A_st, B_st = stack_pairs(pairs, outs, K, max_rank, alpha / r)
    assert A_st.shape == (len(mods) * max_rank, K)
    assert B_st.shape == (sum(outs), len(mods) * max_rank)
    x = torch.randn(5, K, generator=g)
    stacked = (x @ A_st.t()) @ B_st.t()
    # per projection, scale applied afterwards
    separate = torch.cat([(x @ A.t()) @ B.t() * (alpha / r)
                          for A, B in pairs], dim=1)
    assert (stacked - separate).abs().max().item() <= 1e-5
    # a missing module contributes zero to its own output rows only
    A_p, B_p = stack_pairs([pairs[0]] + [None] * (len(mods) - 1), outs, K,
                           max_rank, alpha / r)
    part = (x @ A_p.t()) @ B_p.t()
    assert (part[:, :outs[0]] - separate[:, :outs[0]]).abs().max() <= 1e-5
    assert torch.equal(part[:, outs[0]:], torch.zeros(5, sum(outs[1:])))


# ------------------------------------------------------------------- loader

def test_loader_roundtrip_and_partial_targets(tmp_path):
    r, alpha = 4, 8.0
    mods = ("q_proj", "v_proj", "down_proj")
    sd = adapter_tensors(CFG, r, seed=3, modules=mods)
    p = write_adapter(tmp_path / "ad", CFG, r=r, alpha=alpha, modules=mods,
                      tensors=sd)
    layers = load_adapter(p, CFG, max_rank=16)
    assert len(layers) == CFG.n_layers
    for i, per_layer in enumerate(layers):
        assert sorted(per_layer) == ["down", "qkv"]  # o / gate_up untouched
        A_st, B_st = per_layer["qkv"]
        assert A_st.shape == (48, CFG.hidden_size)
        assert B_st.shape == (CFG.q_size + 2 * CFG.kv_size, 48)
        pre = f"base_model.model.model.layers.{i}.self_attn."
        assert torch.equal(A_st[:r], sd[pre + "q_proj.lora_A.weight"])
        assert torch.equal(A_st[32:32 + r], sd[pre + "v_proj.lora_A.weight"])
        assert torch.equal(A_st[16:32], torch.zeros(16, CFG.hidden_size))  # k
        assert torch.allclose(B_st[:CFG.q_size, :r],
                              sd[pre + "q_proj.lora_B.weight"] * (alpha / r))
        assert torch.equal(B_st[:CFG.q_size, r:], torch.zeros(CFG.q_size, 48 - r))


def test_loader_rejects_bad_adapters(tmp_path):
    sd = adapter_tensors(CFG, 4, seed=4)
    k = "base_model.model.model.layers.1.mlp.up_proj.lora_B.weight"
    bad = dict(sd)
    bad[k] = torch.zeros(CFG.intermediate_size + 8, 4)
    p = write_adapter(tmp_path / "shape", CFG, r=4, tensors=bad)
    with pytest.raises(LoraError, match="up_proj"):
        load_adapter(p, CFG, max_rank=16)

    p = write_adapter(tmp_path / "rank", CFG, r=32, seed=4)
    with pytest.raises(LoraError, match="lora_max_rank"):
        load_adapter(p, CFG, max_rank=16)

    p = write_adapter(tmp_path / "mod", CFG, r=4, seed=4,
                      target_modules=["q_proj", "embed_tokens"])
    with pytest.raises(LoraError, match="embed_tokens"):
        load_adapter(p, CFG, max_rank=16)

    # one layer more than the base model has
    extra = dict(sd)
    extra["base_model.model.model.layers.2.mlp.up_proj.lora_A.weight"] = \
        torch.zeros(4, CFG.hidden_size)
    extra["base_model.model.model.layers.2.mlp.up_proj.lora_B.weight"] = \
        torch.zeros(CFG.intermediate_size, 4)
    p = write_adapter(tmp_path / "layers", CFG, r=4, tensors=extra)
    with pytest.raises(LoraError, match="layers.2"):
        load_adapter(p, CFG, max_rank=16)
    # one layer fewer
    fewer = {k_: v for k_, v in sd.items() if ".layers.1." not in k_}
    p = write_adapter(tmp_path / "fewer", CFG, r=4, tensors=fewer)
    with pytest.raises(LoraError, match="layers"):
        load_adapter(p, CFG, max_rank=16)


def test_max_rank_bounded_by_the_kernel_rank():
    check_max_rank(16)
    with pytest.raises(LoraError, match="qkv"):
        check_max_rank(32)
    with pytest.raises(LoraError, match="R <= 64"):
        LoraPool(CFG, slots=1, max_rank=64, device="cpu")


def test_pool_slots_are_stable_refcounted_and_zeroed(tmp_path):
    pool = LoraPool(CFG, slots=2, max_rank=16, device="cpu")
    px = write_adapter(tmp_path / "x", CFG, seed=1)
    A, B = pool.pair(0, "qkv")
    assert A.shape == (2, 48, CFG.hidden_size) and not A.any()
    ptrs = (A.data_ptr(), B.data_ptr())
    s = pool.acquire(px)
    assert pool.acquire(px) == s
    assert pool.resident() == [{"adapter": px, "slot": s, "refcount": 2}]
    A, B = pool.pair(0, "qkv")
    assert (A.data_ptr(), B.data_ptr()) == ptrs  # in-place load
    assert A[s].any() and B[s].any() and not A[1 - s].any()
    pool.release(px)
    assert A[s].any()
    pool.release(px)
    assert not A[s].any() and not B[s].any() and pool.resident() == []


# ------------------------------------------------------------------- engine

def _engine(tmp_path, tag="e", lora_slots=2, **eng):
    cfg = load_config(path="/nonexistent.yaml", env={})
    root = str(tmp_path / tag)
    cfg.data["store"]["path"] = root
    cfg.data["engine"].update(sync_mode=True, kv_pool_gb=0.01,
                              lora_slots=lora_slots, **eng)
    store = Store(root + "/state", sync="never")
    engine = LLMEngine(store, cfg, device="cpu", state_root=root)
    return engine, Manager(store, engine, cfg)


def _start(manager, name, lora=""):
    a = manager.deploy(name=name, model="tiny-llama", lora=lora)
    manager.start(a.id)
    return a


def test_config_defaults_and_env_override():
    cfg = load_config(path="/nonexistent.yaml", env={})
    assert cfg.get("engine", "lora_slots") == 0
    assert cfg.get("engine", "lora_max_rank") == 16
    cfg = load_config(path="/nonexistent.yaml", env={
        "AGENTAINER_ENGINE_LORA_SLOTS": "4",
        "AGENTAINER_ENGINE_LORA_MAX_RANK": "8"})
    assert cfg.get("engine", "lora_slots") == 4
    assert cfg.get("engine", "lora_max_rank") == 8


def test_zero_adapter_equals_base_and_real_adapter_differs(tmp_path):
    engine, manager = _engine(tmp_path)
    try:
        zero = write_adapter(tmp_path / "zero", CFG, seed=5, b_std=0.0)
        px = write_adapter(tmp_path / "x", CFG, seed=SEED_X)
        base = _start(manager, "base")
        az = _start(manager, "zero", lora=zero)
        ax = _start(manager, "x", lora=px)
        ax2 = _start(manager, "x2", lora=px)
        t_base = gen_tokens(engine, base, PROMPT)
        assert len(t_base) == 8
        # (a) B = 0: the adapter path runs and adds exactly nothing
        assert gen_tokens(engine, az, PROMPT) == t_base
        # (b) deterministic, and not the base model's continuation
        t_x = gen_tokens(engine, ax, PROMPT)
        assert gen_tokens(engine, ax2, PROMPT) == t_x
        assert t_x != t_base
        st = engine.stats()["models"]["tiny-llama"]["lora"]
        assert st["slots"] == 2 and st["max_rank"] == 16
        assert sorted((r["adapter"], r["refcount"]) for r in st["resident"]) \
            == sorted([(zero, 1), (px, 2)])
    finally:
        engine.shutdown()


def test_mixed_batch_routes_each_row_to_its_adapter(tmp_path):
    """Base, X and Y rows decoding in ONE batch get what each gets alone."""
    engine, manager = _engine(tmp_path)
    try:
        px = write_adapter(tmp_path / "x", CFG, seed=SEED_X)
        py = write_adapter(tmp_path / "y", CFG, seed=SEED_Y)
        agents = [_start(manager, "b"), _start(manager, "x", lora=px),
                  _start(manager, "y", lora=py)]
        alone = [gen_tokens(engine, a, PROMPT) for a in agents]
        assert len({tuple(t) for t in alone}) == 3
        inst = engine._instances["tiny-llama"]
        twins = [_start(manager, "b2"), _start(manager, "x2", lora=px),
                 _start(manager, "y2", lora=py)]
        from agentainer_amd.engine.llm import GenRequest
        reqs = []
        for a in twins:
            req = GenRequest(agent_id=a.id, prompt_tokens=list(PROMPT),
                             max_new=8, temperature=0.0, top_p=1.0, seed=0)
            b = inst.binding(a.id)
            with inst._lock:
                b.queue.put(req)
                inst._pump_agent(b)
            reqs.append(req)
        for _ in range(16):
            inst.step()
        assert all(r.done.is_set() and not r.error for r in reqs)
        assert [r.generated for r in reqs] == alone
    finally:
        engine.shutdown()


def test_stop_resume_keeps_the_adapter(tmp_path):
    engine, manager = _engine(tmp_path)
    try:
        px = write_adapter(tmp_path / "x", CFG, seed=SEED_X)
        a = _start(manager, "a", lora=px)
        ctl = _start(manager, "ctl", lora=px)
        base = _start(manager, "base")
        assert gen_tokens(engine, a, PROMPT) == gen_tokens(engine, ctl, PROMPT)
        manager.stop(a.id)
        pool = engine._instances["tiny-llama"].lora_pool
        assert pool.resident()[0]["refcount"] == 1
        manager.resume(a.id)
        assert manager.get(a.id).lora == px
        assert pool.resident()[0]["refcount"] == 2
        p2 = list(range(40, 72))
        out = gen_tokens(engine, a, p2)
        assert out == gen_tokens(engine, ctl, p2)  # restored KV + adapter
        gen_tokens(engine, base, PROMPT)
        assert out != gen_tokens(engine, base, p2)
    finally:
        engine.shutdown()


def test_no_free_slot_fails_attach_until_one_frees(tmp_path):
    engine, manager = _engine(tmp_path)
    try:
        px = write_adapter(tmp_path / "x", CFG, seed=SEED_X)
        py = write_adapter(tmp_path / "y", CFG, seed=SEED_Y)
        pz = write_adapter(tmp_path / "z", CFG, seed=SEED_Z)
        ax = _start(manager, "x", lora=px)
        _start(manager, "y", lora=py)
        az = manager.deploy(name="z", model="tiny-llama", lora=pz)
        with pytest.raises(LoraError, match="no free LoRA slot"):
            manager.start(az.id)
        assert manager.get(az.id).status == FAILED
        assert not engine.is_attached(az.id)
        manager.stop(ax.id)  # X's last agent: its slot is freed
        manager.resume(az.id)
        assert manager.get(az.id).status == RUNNING
        res = engine.stats()["models"]["tiny-llama"]["lora"]["resident"]
        assert sorted(r["adapter"] for r in res) == sorted([py, pz])
        assert len(gen_tokens(engine, az, PROMPT)) == 8
    finally:
        engine.shutdown()


def test_lora_agent_needs_lora_slots(tmp_path):
    engine, manager = _engine(tmp_path, lora_slots=0)
    try:
        px = write_adapter(tmp_path / "x", CFG, seed=SEED_X)
        a = manager.deploy(name="x", model="tiny-llama", lora=px)
        with pytest.raises(LoraError, match="engine.lora_slots"):
            manager.start(a.id)
        assert manager.get(a.id).status == FAILED
        inst = engine._instances["tiny-llama"]
        assert inst.lora_pool is None and inst.dev_adapter_ids is None
        assert engine.stats()["models"]["tiny-llama"]["lora"] is None
    finally:
        engine.shutdown()


def test_lora_rejected_on_mixtral_and_missing_directory(tmp_path):
    engine, manager = _engine(tmp_path)
    try:
        from agentainer_amd.engine.base import ModelNotFound
        with pytest.raises(ModelNotFound, match="does not exist"):
            manager.deploy(name="m", model="tiny-llama",
                           lora=str(tmp_path / "nowhere"))
        os.makedirs(tmp_path / "broken")
        (tmp_path / "broken" / "adapter_config.json").write_text("{not json")
        with pytest.raises(ModelNotFound, match="adapter_config.json"):
            manager.deploy(name="m", model="tiny-llama",
                           lora=str(tmp_path / "broken"))
        px = write_adapter(tmp_path / "x", CFG, seed=SEED_X)
        a = manager.deploy(name="mx", model="tiny-mixtral", lora=px)
        with pytest.raises(LoraError, match="not supported"):
            manager.start(a.id)
    finally:
        engine.shutdown()


def test_device_decode_path_gathers_ids_per_row(tmp_path):
    """The slot-fed decode body (what the GPU captures), emulated on CPU:
    the adapter mirror sits next to the length mirror, pad slot -1."""
    engine, manager = _engine(tmp_path, async_decode_emulate=True,
                              async_decode=False)
    ref_engine, ref_manager = _engine(tmp_path, tag="ref")
    try:
        px = write_adapter(tmp_path / "x", CFG, seed=SEED_X)
        ax, ab = _start(manager, "x", lora=px), _start(manager, "b")
        rx, rb = _start(ref_manager, "x", lora=px), _start(ref_manager, "b")
        inst = engine._instances["tiny-llama"]
        assert inst.dev_decode and inst.dev_adapter_ids is not None
        mirror = inst.dev_adapter_ids
        assert mirror[inst._pad_slot].item() == -1
        assert mirror[inst.kvm.slot(ax.id)].item() == inst.binding(ax.id).adapter_slot
        assert mirror[inst.kvm.slot(ab.id)].item() == -1
        assert gen_tokens(engine, ax, PROMPT) == gen_tokens(ref_engine, rx, PROMPT)
        assert gen_tokens(engine, ab, PROMPT) == gen_tokens(ref_engine, rb, PROMPT)
        slot = inst.kvm.slot(ax.id)
        manager.stop(ax.id)
        assert mirror[slot].item() == -1
    finally:
        engine.shutdown()
        ref_engine.shutdown()


# ----------------------------------------------------------- prefix sharing

SYSPROMPT = ("You are a terse assistant for the flight-booking team. "
             "Answer in one sentence and never guess prices.")


def _sys_agent(engine, manager, name, lora, msg):
    """Start an agent with the shared system prompt and run its first
    turn, framed the way LLMEngine._build_prompt frames it."""
    a = manager.deploy(name=name, model="tiny-llama", lora=lora,
                       system_prompt=SYSPROMPT)
    manager.start(a.id)
    tok = engine._instances["tiny-llama"].tokenizer
    prompt = tok.encode(f"[system] {SYSPROMPT}\n") + tok.encode(f"[user] {msg}\n")
    return a, gen_tokens(engine, a, prompt)


def test_prefix_sharing_is_keyed_by_adapter(tmp_path):
    px = write_adapter(tmp_path / "x", CFG, seed=SEED_X)
    py = write_adapter(tmp_path / "y", CFG, seed=SEED_Y)
    engine, manager = _engine(tmp_path, "shared")
    ctl, ctl_manager = _engine(tmp_path, "control", prefix_sharing=False)
    try:
        x1, _ = _sys_agent(engine, manager, "x1", px, "where is my bag?")
        x2, _ = _sys_agent(engine, manager, "x2", px, "can I change seats?")
        y, out_y = _sys_agent(engine, manager, "y", py, "where is my bag?")
        b, out_b = _sys_agent(engine, manager, "b", "", "where is my bag?")
        inst = engine._instances["tiny-llama"]
        n_pg = len(inst.binding(x1.id).prefix_tokens) // inst.kvm.page_size
        assert n_pg >= 2
        head = {a.id: inst.kvm._seqs[a.id].pages[:n_pg] for a in (x1, x2, y, b)}
        # exactly the two X agents share pages
        assert head[x1.id] == head[x2.id]
        assert not set(head[y.id]) & set(head[x1.id])
        assert not set(head[b.id]) & set(head[x1.id])
        assert not set(head[b.id]) & set(head[y.id])
        assert len(inst._prefixes) == 3  # one per adapter identity + base
        # Y (which adopted its own lazily created prefix) equals a control
        # Y agent with no prefix sharing at all; likewise the base agent
        _, ctl_y = _sys_agent(ctl, ctl_manager, "y", py, "where is my bag?")
        _, ctl_b = _sys_agent(ctl, ctl_manager, "b", "", "where is my bag?")
        assert not ctl._instances["tiny-llama"]._prefixes
        assert out_y == ctl_y
        assert out_b == ctl_b
        assert out_y != out_b
    finally:
        engine.shutdown()
        ctl.shutdown()


# -------------------------------------------------------- field propagation

def test_lora_field_through_yaml_api_and_backup(runtime, tmp_path):
    px = write_adapter(tmp_path / "x", CFG, seed=1)
    # deployment YAML
    p = tmp_path / "d.yaml"
    p.write_text("kind: AgentDeployment\nspec:\n  agents:\n"
                 f"    - name: tuned\n      model: echo\n      lora: {px}\n"
                 "      replicas: 2\n"
                 "    - name: plain\n      model: echo\n")
    specs = load_deployment(str(p))
    assert [s.lora for s in specs] == [px, px, ""]
    assert specs[0].to_dict()["lora"] == px
    # REST deploy body -> agent record
    from fastapi.testclient import TestClient

    from agentainer_amd.api import create_app
    from agentainer_amd.config import DEFAULT_TOKEN
    auth = {"Authorization": f"Bearer {DEFAULT_TOKEN}"}
    with TestClient(create_app(runtime)) as c:
        r = c.post("/agents", json=specs[0].to_dict(), headers=auth)
        assert r.status_code == 200, r.text
        aid = r.json()["data"]["id"]
        assert r.json()["data"]["lora"] == px
        assert c.get(f"/agents/{aid}", headers=auth).json()["data"]["lora"] == px
        r = c.post("/agents", json={"name": "bad", "model": "echo",
                                    "lora": str(tmp_path / "missing")},
                   headers=auth)
        assert r.status_code == 400 and "does not exist" in r.json()["message"]
    assert runtime.agents.get(aid).lora == px
    # backup -> restore
    bk = runtime.backups.create("snap")
    assert json.dumps(bk).count(px) >= 1
    restored = runtime.backups.restore(bk["id"])
    assert [a.lora for a in restored if a.name == "tuned-1-restored"] == [px]


def test_cli_deploy_passes_lora(monkeypatch):
    from click.testing import CliRunner

    from agentainer_amd import cli as cli_mod
    sent = {}

    def fake_call(self, method, path, body=None, **kw):
        sent.update(method=method, path=path, body=body)
        return {"data": {"name": "n", "id": "agent-1"}}

    monkeypatch.setattr(cli_mod.Client, "call", fake_call)
    res = CliRunner().invoke(cli_mod.cli, ["deploy", "tiny-llama", "--lora",
                                           "/adapters/support"])
    assert res.exit_code == 0, res.output
    assert sent["path"] == "/agents"
    assert sent["body"]["lora"] == "/adapters/support"
