"""ops.Projection on the GPU: it takes exactly the GEMM that the public
ops functions take for the same weight form, bit for bit.

N = 512, K = 1024 are the smallest shapes every kernel here accepts with
split-K 4; M = 64 is the full tile and 65 the first row count that must
fall off the skinny and quantized routes."""

import pytest
import torch
import torch.nn.functional as F

from agentainer_amd import ops

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs MI355X", allow_module_level=True)


@pytest.fixture(autouse=True, scope="module")
def _require_hip():
    assert ops.hip_available(), "HIP extension must be present on the GPU box"


DEV = "cuda"
N, K = 512, 1024
MS = [1, 17, 64, 65]
EPS = 1e-5

_cache = {}


def _w():
    """The weight, its quantized forms and a norm weight; made once and
    shared, never modified."""
    if not _cache:
        g = torch.Generator(device="cpu").manual_seed(29)
        w = (torch.randn(N, K, generator=g) * 0.1).to(torch.bfloat16).to(DEV)
        _cache["w"] = w
        _cache["fp8"] = ops.quantize_weight_fp8(w)
        _cache["mxfp4"] = ops.quantize_weight_mxfp4(w)
        _cache["norm"] = (1.0 + 0.1 * torch.randn(N, generator=g)
                          ).to(torch.bfloat16).to(DEV)
    return _cache


def _x(M):
    g = torch.Generator(device="cpu").manual_seed(100 + M)
    return (torch.randn(M, K, generator=g) * 0.5).to(torch.bfloat16).to(DEV)


def _res(M):
    g = torch.Generator(device="cpu").manual_seed(200 + M)
    return torch.randn(M, N, generator=g).to(torch.bfloat16).to(DEV)


@pytest.mark.parametrize("M", MS)
def test_bf16_route(M, monkeypatch):
    monkeypatch.setitem(ops._SKINNY_SHAPES, (N, K), (4, 128, 2))
    monkeypatch.setattr(ops, "SPLITK_DEFER_DISABLED", False)
    w, x = _w()["w"], _x(M)
    proj = ops.Projection(w).pack()
    assert proj.kind == "bf16"
    want = ops.linear(x, w, ops.pack_weight(w))
    assert torch.equal(proj(x), want)
    got = proj(x, defer=True)
    if M > 64:
        assert torch.equal(got, want)
        return
    assert isinstance(got, ops.SplitKPartial) and got.split == 4
    norm = _w()["norm"]
    res_a, res_b = _res(M), _res(M)
    out_a, out_b = torch.empty_like(res_a), torch.empty_like(res_b)
    ops.fused_add_rmsnorm(out_b, got, res_b, norm, EPS)
    ops.fused_add_rmsnorm(out_a, want, res_a, norm, EPS)
    assert torch.equal(out_a, out_b) and torch.equal(res_a, res_b)
    monkeypatch.setattr(ops, "SPLITK_DEFER_DISABLED", True)
    got = proj(x, defer=True)
    assert type(got) is torch.Tensor and torch.equal(got, want)


@pytest.mark.parametrize("kind", ["fp8", "mxfp4"])
@pytest.mark.parametrize("M", MS)
def test_quant_route(M, kind):
    w, x = _w()["w"], _x(M)
    proj = ops.Projection(w).pack(kind)
    assert proj.kind == kind and proj.packed is None
    if M <= 64:
        fn = ops.linear_fp8 if kind == "fp8" else ops.linear_mxfp4
        want = fn(x, *_w()[kind], N)
    else:
        want = F.linear(x, w)
    assert torch.equal(proj(x), want)
    got = proj(x, defer=True)
    assert type(got) is torch.Tensor and torch.equal(got, want)
