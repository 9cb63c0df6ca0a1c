"""CPU side of the deferred split-K reduction: without a GPU there are no
partials, so linear_partial is linear and the norm takes its tensor."""

import torch

from agentainer_amd import ops
from agentainer_amd.models.llama import LLAMA_CONFIGS, LlamaMLP


def test_linear_partial_on_cpu_is_a_tensor():
    torch.manual_seed(0)
    x = torch.randn(5, 256, dtype=torch.bfloat16)
    w = torch.randn(64, 256, dtype=torch.bfloat16)
    res = torch.randn(5, 64, dtype=torch.bfloat16)
    nw = torch.randn(64, dtype=torch.bfloat16)
    y = ops.linear_partial(x, w, None)
    assert isinstance(y, torch.Tensor) and y.dtype == torch.bfloat16
    assert torch.equal(y, ops.linear(x, w, None))
    res_a, res_b = res.clone(), res.clone()
    out_a, out_b = torch.empty_like(res), torch.empty_like(res)
    ops.fused_add_rmsnorm(out_a, ops.linear(x, w, None), res_a, nw, 1e-5)
    ops.fused_add_rmsnorm(out_b, y, res_b, nw, 1e-5)
    assert torch.equal(out_a, out_b) and torch.equal(res_a, res_b)


def test_mlp_defer_keyword_is_a_no_op_on_cpu():
    torch.manual_seed(1)
    mlp = LlamaMLP(LLAMA_CONFIGS["tiny-llama"])
    for p in mlp.parameters():
        p.data.normal_(0.0, 0.02)
    h = torch.randn(3, 512, dtype=torch.bfloat16)
    assert torch.equal(mlp(h, defer_reduce=True), mlp(h))
