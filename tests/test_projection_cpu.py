"""ops.Projection off-GPU, and the parameter registration it must not
disturb: the loader and the TP tests address parameters by name, and
random_init draws from one generator in named_parameters() order."""

import hashlib

import pytest
import torch
import torch.nn.functional as F

from agentainer_amd import ops
from agentainer_amd.models.llama import LLAMA_CONFIGS, LlamaForCausalLM
from agentainer_amd.models.mixtral import MIXTRAL_CONFIGS, MixtralForCausalLM


LLAMA_NAMES = [
    "embed", "final_ln",
    "layers.0.input_ln", "layers.0.post_ln",
    "layers.0.attn.qkv_proj", "layers.0.attn.o_proj",
    "layers.0.mlp.gate_up", "layers.0.mlp.down",
    "layers.1.input_ln", "layers.1.post_ln",
    "layers.1.attn.qkv_proj", "layers.1.attn.o_proj",
    "layers.1.mlp.gate_up", "layers.1.mlp.down",
]
MIXTRAL_NAMES = [
    "embed", "final_ln", "lm_head",
    "layers.0.input_ln", "layers.0.post_ln",
    "layers.0.attn.qkv_proj", "layers.0.attn.o_proj",
    "layers.0.moe.router",
    "layers.0.moe.gate_up.0", "layers.0.moe.gate_up.1",
    "layers.0.moe.gate_up.2", "layers.0.moe.gate_up.3",
    "layers.0.moe.down.0", "layers.0.moe.down.1",
    "layers.0.moe.down.2", "layers.0.moe.down.3",
    "layers.1.input_ln", "layers.1.post_ln",
    "layers.1.attn.qkv_proj", "layers.1.attn.o_proj",
    "layers.1.moe.router",
    "layers.1.moe.gate_up.0", "layers.1.moe.gate_up.1",
    "layers.1.moe.gate_up.2", "layers.1.moe.gate_up.3",
    "layers.1.moe.down.0", "layers.1.moe.down.1",
    "layers.1.moe.down.2", "layers.1.moe.down.3",
]


@pytest.mark.parametrize("cls,cfg,names,digest", [
    (LlamaForCausalLM, LLAMA_CONFIGS["tiny-llama"], LLAMA_NAMES,
     "79457b668cc20097"),
    (MixtralForCausalLM, MIXTRAL_CONFIGS["tiny-mixtral"], MIXTRAL_NAMES,
     "9d457c6ec387fb61"),
])
def test_parameter_registration_unchanged(cls, cfg, names, digest):
    model = cls(cfg, device="cpu", seed=0)
    assert len(names) == (14 if cls is LlamaForCausalLM else 29)
    assert [n for n, _ in model.named_parameters()] == names
    h = hashlib.sha256()
    for _, p in model.named_parameters():
        h.update(p.detach().view(torch.int16).numpy().tobytes())
    assert h.hexdigest().startswith(digest)


def _xw():
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(3, 256, generator=g) * 0.5).to(torch.bfloat16)
    w = (torch.randn(64, 256, generator=g) * 0.1).to(torch.bfloat16)
    return x, torch.nn.Parameter(w)


@pytest.mark.parametrize("quant,kind", [(None, None), ("", "bf16"),
                                        ("fp8", "fp8"), ("mxfp4", "mxfp4")])
def test_projection_on_cpu_is_f_linear(quant, kind):
    """Every state computes F.linear on CPU: the quantized forms are
    GPU-only and must never run here."""
    x, w = _xw()
    proj = ops.Projection(w)
    if quant is not None:
        assert proj.pack(quant) is proj
    assert proj.w is w
    assert proj.kind == kind
    # exactly one form (none before pack)
    assert (proj.packed is not None) == (kind == "bf16")
    assert (proj.quant is not None) == (kind in ("fp8", "mxfp4"))
    want = F.linear(x, w)
    assert torch.equal(proj(x), want)
    got = proj(x, defer=True)
    assert type(got) is torch.Tensor and got.dtype == torch.bfloat16
    assert torch.equal(got, want)


def test_repack_replaces_the_form():
    _, w = _xw()
    proj = ops.Projection(w).pack("fp8")
    proj.pack()
    assert proj.kind == "bf16" and proj.quant is None
    assert torch.equal(proj.packed, ops.pack_weight(w.data))
    proj.pack("mxfp4")
    assert proj.kind == "mxfp4" and proj.packed is None
