"""Shared helpers of the LoRA tests: write PEFT-style adapter directories
with seeded random weights, and drive one greedy generation through a
sync-mode engine."""

import json
import os

import torch
from safetensors.torch import save_file

from agentainer_amd.engine.llm import GenRequest
from agentainer_amd.models.lora import FUSED, _PARENT, proj_dims

ALL_MODULES = tuple(m for mods in FUSED.values() for m in mods)


def module_dims(cfg):
    """HF module name -> (in, out) for a LlamaConfig."""
    out = {}
    for proj, (K, outs) in proj_dims(cfg).items():
        for m, n in zip(FUSED[proj], outs):
            out[m] = (K, n)
    return out


def adapter_tensors(cfg, r, seed, modules=ALL_MODULES, b_std=0.1,
                    n_layers=None):
    """Seeded random lora_A [r, in] ~ N(0, 1/sqrt(in)) and lora_B [out, r]
    ~ N(0, b_std) for every layer and listed module (b_std = 0: the
    identity adapter)."""
    gen = torch.Generator().manual_seed(seed)
    dims = module_dims(cfg)
    sd = {}
    for i in range(cfg.n_layers if n_layers is None else n_layers):
        for m in modules:
            K, n = dims[m]
            base = f"base_model.model.model.layers.{i}.{_PARENT[m]}.{m}."
            sd[base + "lora_A.weight"] = (
                torch.randn(r, K, generator=gen) / K ** 0.5)
            sd[base + "lora_B.weight"] = torch.randn(n, r, generator=gen) * b_std
    return sd


def write_adapter(path, cfg, r=8, alpha=16.0, seed=0, modules=ALL_MODULES,
                  b_std=0.1, tensors=None, target_modules=None):
    os.makedirs(path, exist_ok=True)
    sd = tensors if tensors is not None else adapter_tensors(
        cfg, r, seed, modules, b_std)
    with open(os.path.join(path, "adapter_config.json"), "w") as f:
        json.dump({"peft_type": "LORA", "r": r, "lora_alpha": alpha,
                   "target_modules": list(
                       modules if target_modules is None else target_modules)},
                  f)
    save_file({k: v.contiguous() for k, v in sd.items()},
              os.path.join(path, "adapter_model.safetensors"))
    return str(path)


def gen_tokens(engine, agent, prompt, max_new=8):
    """One greedy request through a sync-mode engine, stepped to the end."""
    inst = engine._instances[agent.model]
    req = GenRequest(agent_id=agent.id, prompt_tokens=list(prompt),
                     max_new=max_new, temperature=0.0, top_p=1.0, seed=0)
    b = inst.binding(agent.id)
    with inst._lock:
        b.queue.put(req)
        inst._pump_agent(b)
    for _ in range(max_new + 8):
        inst.step()
        if req.done.is_set():
            break
    if inst.is_gpu:
        torch.cuda.synchronize()
    assert req.done.is_set() and not req.error, req.error
    return req.generated
