"""Wide-tile (NW tiles per wave) packed skinny GEMM.

Contract: for a given (split, kc) every output element accumulates the same
products in the same order whatever NW is, so the bf16 output and the f32
split-K partials are bit-identical to NW=1. Also checked against fp32."""

import pytest
import torch

from agentainer_amd import ops

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs MI355X", allow_module_level=True)


@pytest.fixture(autouse=True, scope="module")
def _require_hip():
    assert ops.hip_available(), "HIP extension must be present on the GPU box"


DEV = "cuda"
MS = [1, 17, 64]

# ---------------- NW bit-identity ----------------

NW_SHAPES = [(256, 256, 1, 128), (256, 512, 2, 128), (512, 1024, 4, 128),
             (256, 512, 1, 256)]


def _xw(M, N, K, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = (torch.randn(M, K, generator=g) * 0.5).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) * 0.1).to(torch.bfloat16)
    return x, w


_nw1_cache = {}


def _nw1(M, N, K, split, kc):
    """(x, packed w, bf16 out, f32 partials or None) of the NW=1 kernel;
    computed once per case and shared, never modified."""
    key = (M, N, K, split, kc)
    if key not in _nw1_cache:
        mod = ops._load_hip()
        x, w = _xw(M, N, K, seed=17 * M + N + K)
        xd, wp = x.to(DEV), ops.pack_weight(w.to(DEV))
        ws = torch.full((max(split * M * N, 1),), float("nan"),
                        dtype=torch.float32, device=DEV)
        out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
        mod.skinny_gemm_packed(out, xd, wp, N, K, ws, split, False, kc, True, 1)
        _nw1_cache[key] = (xd, wp, out, ws.clone() if split > 1 else None)
    return _nw1_cache[key]


@pytest.mark.parametrize("nw", [2, 4])
@pytest.mark.parametrize("N,K,split,kc", NW_SHAPES)
@pytest.mark.parametrize("M", MS)
def test_nw_bit_identical(M, N, K, split, kc, nw):
    mod = ops._load_hip()
    xd, wp, want, want_ws = _nw1(M, N, K, split, kc)
    ws = torch.full((max(split * M * N, 1),), float("nan"),
                    dtype=torch.float32, device=DEV)
    out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    mod.skinny_gemm_packed(out, xd, wp, N, K, ws, split, False, kc, True, nw)
    assert torch.equal(out, want)
    if split > 1:
        ws.fill_(float("nan"))  # the partial-only call must rewrite every slab
        unwritten = torch.empty(0, dtype=torch.bfloat16, device=DEV)
        mod.skinny_gemm_packed(unwritten, xd, wp, N, K, ws, split, False, kc,
                               False, nw)
        assert not torch.isnan(ws).any(), "a split-K slab was not rewritten"
        assert torch.equal(ws, want_ws)


def test_nw_rejects_bad_arguments():
    mod = ops._load_hip()
    N, K = 192, 256
    x, w = _xw(4, N, K, seed=1)
    xd, wp = x.to(DEV), ops.pack_weight(w.to(DEV))
    ws = torch.empty(1, dtype=torch.float32, device=DEV)
    out = torch.empty(4, N, dtype=torch.bfloat16, device=DEV)
    mod.skinny_gemm_packed(out, xd, wp, N, K, ws, 1, False, 128, True, 1)
    with pytest.raises(RuntimeError):  # 192 is no multiple of 64 * 2
        mod.skinny_gemm_packed(out, xd, wp, N, K, ws, 1, False, 128, True, 2)
    with pytest.raises(RuntimeError):  # nw is 1, 2 or 4
        mod.skinny_gemm_packed(out, xd, wp, N, K, ws, 1, False, 128, True, 3)


@pytest.mark.parametrize("nw", [2, 4])
def test_nw_matches_fp32_reference(nw):
    """The project's criterion for skinny GEMMs: max-abs error over the
    reference's max-abs below 0.02."""
    M, N, K, split, kc = 17, 512, 1024, 4, 128
    mod = ops._load_hip()
    x, w = _xw(M, N, K, seed=17 * M + N + K)  # the inputs of _nw1
    xd, wp, _, _ = _nw1(M, N, K, split, kc)
    ws = torch.empty(split * M * N, dtype=torch.float32, device=DEV)
    out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    mod.skinny_gemm_packed(out, xd, wp, N, K, ws, split, False, kc, True, nw)
    want = x.float() @ w.float().T
    rel = ((out.float().cpu() - want).abs().max() / want.abs().max()).item()
    assert rel < 0.02, f"max-abs error / max-abs reference = {rel:.3e}"


def test_dispatch_passes_tuned_nw(monkeypatch):
    """ops.linear hands the table's nw to the kernel, and the result is the
    NW=1 result."""
    mod = ops._load_hip()
    M, N, K = 17, 512, 1024
    xd, wp, want, _ = _nw1(M, N, K, 4, 128)
    seen = []
    orig = mod.skinny_gemm_packed

    def spy(*args):
        seen.append(args[6:])
        return orig(*args)

    monkeypatch.setattr(mod, "skinny_gemm_packed", spy)
    monkeypatch.setitem(ops._SKINNY_SHAPES, (N, K), (4, 128, 2))
    w = torch.empty(N, K, dtype=torch.bfloat16, device=DEV)  # shape only
    got = ops.linear(xd, w, wp)
    assert seen == [(4, ops.SKINNY_NT, 128, True, 2)]
    assert torch.equal(got, want)
