"""ops — dispatch layer over the gfx950 HIP kernels.

Policy (the driver's "native code not loaded" check depends on this):
  * On a CUDA/ROCm device: the in-tree HIP extension (_hip_ops.so) is
    REQUIRED. If it is missing or fails to import, GPU ops raise
    RuntimeError — there is no silent eager fallback on a GPU box.
  * On CPU: the fp32 torch references (ops.reference) run, so the engine
    and control plane are testable without a GPU.

Build the extension with `python -m agentainer_amd.ops.build` (or via
__graft_entry__.build()).
"""

from __future__ import annotations

import os
from typing import Optional

import torch

from . import reference

_hip = None
_hip_err: Optional[str] = None


def _load_hip():
    global _hip, _hip_err
    if _hip is not None or _hip_err is not None:
        return _hip
    so = os.path.join(os.path.dirname(__file__), "_hip_ops.so")
    if not os.path.exists(so):
        _hip_err = f"HIP extension not built ({so} missing); run python -m agentainer_amd.ops.build"
        return None
    try:
        import importlib.util

        spec = importlib.util.spec_from_file_location("agentainer_amd.ops._hip_ops", so)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        _hip = mod
    except Exception as exc:  # noqa: BLE001
        _hip_err = f"HIP extension failed to load: {exc}"
    return _hip


def hip_available() -> bool:
    return _load_hip() is not None


def _dispatch(name: str, *tensors: torch.Tensor):
    """Return the HIP module if the leading tensor is on GPU, else None.
    On GPU with no extension: fail loudly (never a silent fallback)."""
    if tensors[0].is_cuda:
        mod = _load_hip()
        if mod is None:
            raise RuntimeError(
                f"op {name!r} on GPU requires the gfx950 HIP extension: {_hip_err}")
        return mod
    return None


def rmsnorm(out, x, w, eps: float = 1e-5):
    mod = _dispatch("rmsnorm", x)
    if mod:
        mod.rmsnorm(out, x, w, float(eps))
    else:
        reference.rmsnorm(out, x, w, eps)
    return out


def fused_add_rmsnorm(out, x, residual, w, eps: float = 1e-5):
    """residual += x; out = rmsnorm(residual) * w. x is a tensor, or the
    SplitKPartial that linear_partial returned: the norm kernel then sums
    the GEMM's split-K partials itself (bit-identical to combining first)."""
    if isinstance(x, SplitKPartial):
        mod = _dispatch("splitk_add_rmsnorm", residual)
        mod.splitk_add_rmsnorm(out, x.consume(), x.split, x.M, x.N, residual,
                               w, float(eps))
        return out
    mod = _dispatch("fused_add_rmsnorm", x)
    if mod:
        mod.fused_add_rmsnorm(out, x, residual, w, float(eps))
    else:
        reference.fused_add_rmsnorm(out, x, residual, w, eps)
    return out


def silu_mul(out, gate, up):
    mod = _dispatch("silu_mul", gate)
    if mod:
        mod.silu_mul(out, gate, up)
    else:
        reference.silu_mul(out, gate, up)
    return out


make_cos_sin_table = reference.make_cos_sin_table


def rope_inplace(q, k, cos_sin, positions):
    mod = _dispatch("rope_inplace", q)
    if mod:
        mod.rope_inplace(q, k, cos_sin, positions)
    else:
        reference.rope_inplace(q, k, cos_sin, positions)


def rope_append(q, k, v, k_cache, v_cache, cos_sin, positions, slot_mapping):
    """Fused rope_inplace(q,k) + kv_append(k,v). CPU falls back to the two
    reference ops."""
    mod = _dispatch("rope_append", q)
    if mod:
        mod.rope_append(q, k, v, k_cache, v_cache, cos_sin, positions,
                        slot_mapping)
    else:
        reference.rope_inplace(q, k, cos_sin, positions)
        reference.kv_append(k_cache, v_cache, k, v, slot_mapping)


def kv_append(k_cache, v_cache, k, v, slot_mapping):
    mod = _dispatch("kv_append", k)
    if mod:
        mod.kv_append(k_cache, v_cache, k, v, slot_mapping)
    else:
        reference.kv_append(k_cache, v_cache, k, v, slot_mapping)


def paged_decode_attention(out, q, k_cache, v_cache, page_table, seq_lens,
                           scale: float):
    mod = _dispatch("paged_decode_attention", q)
    if mod:
        mod.paged_decode_attention(out, q, k_cache, v_cache, page_table,
                                   seq_lens, float(scale))
    else:
        reference.paged_decode_attention(out, q, k_cache, v_cache, page_table,
                                         seq_lens, scale)
    return out


def paged_prefill_attention(out, q, k_cache, v_cache, page_table, seq_lens,
                            query_starts, query_lens, scale: float,
                            max_qlen: int = 0):
    mod = _dispatch("paged_prefill_attention", q)
    if mod:
        mod.paged_prefill_attention(out, q, k_cache, v_cache, page_table,
                                    seq_lens, query_starts, query_lens,
                                    float(scale), int(max_qlen))
    else:
        reference.paged_prefill_attention(out, q, k_cache, v_cache, page_table,
                                          seq_lens, query_starts, query_lens,
                                          scale)
    return out


def greedy_sample(out, logits):
    mod = _dispatch("greedy_sample", logits)
    if mod:
        mod.greedy_sample(out, logits)
    else:
        reference.greedy_sample(out, logits)
    return out


def topp_sample(out, logits, temps, top_ps, seeds):
    mod = _dispatch("topp_sample", logits)
    if mod:
        mod.topp_sample(out, logits, temps, top_ps, seeds)
    else:
        reference.topp_sample(out, logits, temps, top_ps, seeds)
    return out


_sample_ws_cache = {}


def _sample_ws(device, n: int) -> torch.Tensor:
    # keyed like _lora_ws: the deferred prefill sample and the decode
    # sample may run on different streams
    stream = (torch.cuda.current_stream(device).cuda_stream
              if device.type == "cuda" else 0)
    key = (device, stream)
    ws = _sample_ws_cache.get(key)
    if ws is None or ws.numel() < n:
        ws = torch.empty(n, dtype=torch.float32, device=device)
        _sample_ws_cache[key] = ws
    return ws


def sample_ex(out, logits, temps, top_ps, seeds, top_ks, min_ps, reps, press,
              freqs, edits, pending=None, ws=None):
    """Extended sampler: penalties, logit_bias, top-k, min-p, top-p
    (semantics: reference.sample_ex). logits bf16 [B, V]; the scalar
    parameters are per-row Python sequences; edits[b] is a sequence of
    (token, 2 * count + in_prompt, bias) with unique tokens; pending is a
    device int64 [B] of in-flight tokens (-1: none) or None. Each CSR
    array goes to the device in one copy. ws (f32, >= B*V) receives the
    edited rows; by default a cached per-(device, stream) workspace."""
    B, V = logits.shape
    dev = logits.device
    ptr = [0]
    tok, cnt, bias = [], [], []
    for row in edits:
        if row:
            t, c, b = zip(*row)
            tok.extend(t); cnt.extend(c); bias.extend(b)
        ptr.append(len(tok))
    assert len(ptr) == B + 1

    def vec(vals, dtype):
        return torch.tensor(list(vals), dtype=dtype).to(dev, non_blocking=True)

    args = (vec(temps, torch.float32), vec(top_ps, torch.float32),
            vec(min_ps, torch.float32), vec(reps, torch.float32),
            vec(press, torch.float32), vec(freqs, torch.float32),
            vec(top_ks, torch.int32), vec(seeds, torch.int64),
            vec(ptr, torch.int32), vec(tok, torch.int32),
            vec(cnt, torch.int32), vec(bias, torch.float32))
    if pending is None:
        pending = torch.full((B,), -1, dtype=torch.int64, device=dev)
    mod = _dispatch("sample_ex", logits)
    if mod:
        if ws is None:
            ws = _sample_ws(dev, B * V)
        logits = logits.contiguous()
        if logits.data_ptr() % 16:  # a view into a larger buffer
            logits = logits.clone()
        mod.sample_ex(out, logits, ws, *args, pending)
    else:
        reference.sample_ex(out, logits, ws, *args, pending)
    return out


def token_logprobs(logits, rows, chosen, K: int):
    """Raw logprobs of the sampled tokens and the top K (0..20) of each
    requested row (semantics: reference.token_logprobs). logits bf16
    [B, V], read in place; rows int32 [R] picks the rows, in any order;
    chosen int64 [B] is the sampler's output. Returns (chosen_lp f32 [R],
    top_id int32 [R, K], top_lp f32 [R, K]) on the logits' device; the
    launch is asynchronous."""
    mod = _dispatch("token_logprobs", logits)
    if not mod:
        return reference.token_logprobs(logits, rows, chosen, K)
    R, K = rows.numel(), int(K)
    dev = logits.device
    chosen_lp = torch.empty(R, dtype=torch.float32, device=dev)
    top_id = torch.empty(R, K, dtype=torch.int32, device=dev)
    top_lp = torch.empty(R, K, dtype=torch.float32, device=dev)
    mod.token_logprobs(chosen_lp, top_id, top_lp, logits, rows, chosen, K)
    return chosen_lp, top_id, top_lp


_ws_cache = {}
_EMPTY_WS = {}
SKINNY_DISABLED = os.environ.get("AGENTAINER_DISABLE_SKINNY", "0") == "1"
SKINNY_FORCED = os.environ.get("AGENTAINER_FORCE_SKINNY", "0") == "1"
# A/B hook: linear_partial always combines (no deferred split-K reduction)
SPLITK_DEFER_DISABLED = (
    os.environ.get("AGENTAINER_DISABLE_SPLITK_DEFER", "0") == "1")
# shapes where the hand-written skinny GEMM beat hipBLASLt on MI355X, as
# (split_k, k_chunk, tiles per wave), decided by in-graph kernel averages
# (profiles/README.md, "Wide-tile skinny GEMM"). The library keeps qkv
# (19.2 us vs 20.6 best skinny, cold) and gate_up (48-50 us vs 53-57; a
# SwiGLU epilogue did not make up the difference: 59.3 vs 52.0 + 4.9).
_SKINNY_SHAPES = {
    # o-proj 14.5 us in-graph. nw=2 loses at split 4 (19.4 vs 17.4 cold);
    # (8, 128, 2) runs 12.0 us but would change the accumulation order
    (4096, 4096): (4, 128, 1),
    # down-proj: nw 1 -> 2 took it from 36.1-36.8 to 30.5-31.6 us in-graph,
    # bit-identical (same split and k_chunk)
    (4096, 14336): (8, 128, 2),
}
SKINNY_NT = os.environ.get("AGENTAINER_SKINNY_NT", "0") == "1"
SKINNY_KC = int(os.environ.get("AGENTAINER_SKINNY_KC", "0"))  # 0 = tuned
# A/B hook: extra tuned shapes as "N:K:split:kc[:nw],..." (perf experiments)
for _spec in os.environ.get("AGENTAINER_SKINNY_SHAPES", "").split(","):
    if _spec.strip():
        _n, _k, _s, _c, *_w = (int(v) for v in _spec.split(":"))
        _SKINNY_SHAPES[(_n, _k)] = (_s, _c, _w[0] if _w else 1)


def _skinny_split(ntiles: int, K: int) -> int:
    # target ~256 blocks (1 per CU — measured optimum: 2 blocks/CU halve
    # the per-block LDS and contend on the chunk barriers)
    split = 1
    while split < 16 and ntiles * split < 256 and K % (256 * split * 2) == 0:
        split *= 2
    return split


def _fragment_linear(w: torch.Tensor) -> torch.Tensor:
    # [N, K] -> flat packed[n_tile][k_chunk][lane][8], 2- or 1-byte elements
    N, K = w.shape
    return (w.view(N // 16, 16, K // 32, 4, 8)
            .permute(0, 2, 3, 1, 4).contiguous().view(-1))


def pack_weight(w: torch.Tensor) -> torch.Tensor:
    """Shuffle a static [N, K] weight into MFMA-fragment-linear layout
    packed[n_tile][k_chunk][lane][8] so the skinny GEMM's weight stream is
    contiguous per wave. Done once at model load; flat [N*K] result."""
    N, K = w.shape
    assert N % 16 == 0 and K % 32 == 0
    return _fragment_linear(w)


class _Workspace:
    """One cached split-K buffer; gen counts how often it was handed out."""
    __slots__ = ("buf", "gen")

    def __init__(self, buf: torch.Tensor):
        self.buf = buf
        self.gen = 0


class SplitKPartial:
    """A skinny GEMM's result still in split-K form: ws holds the f32
    partials [split, M, N], to be summed by the consumer
    (fused_add_rmsnorm). It borrows a cached workspace, so it must be
    consumed before that workspace is handed out again — consume() raises
    otherwise instead of reading another GEMM's partials."""
    __slots__ = ("ws", "split", "M", "N", "_slot", "_gen")

    def __init__(self, slot: _Workspace, split: int, M: int, N: int):
        self.ws, self.split, self.M, self.N = slot.buf, split, M, N
        self._slot, self._gen = slot, slot.gen

    def consume(self) -> torch.Tensor:
        if self._slot.gen != self._gen or self._slot.buf is not self.ws:
            raise RuntimeError(
                "stale SplitKPartial: its split-K workspace was handed out "
                "again before the partials were consumed")
        return self.ws


def _skinny_ws_slot(device, N: int, split: int) -> _Workspace:
    # keyed by the current stream too: a side-stream prefill with <= 64
    # padded tokens takes the skinny path and must not write the buffer an
    # in-flight decode graph on another stream is still reading
    stream = torch.cuda.current_stream(device).cuda_stream
    key = (device, stream, N, split)
    slot = _ws_cache.get(key)
    if slot is None or slot.buf.numel() < split * 64 * N:
        slot = _Workspace(torch.empty(split * 64 * N, dtype=torch.float32,
                                      device=device))
        _ws_cache[key] = slot
    slot.gen += 1
    return slot


def _skinny_ws(device, N: int, split: int) -> torch.Tensor:
    if split > 1:
        return _skinny_ws_slot(device, N, split).buf
    ws = _EMPTY_WS.get(device)
    if ws is None:
        ws = torch.empty(1, dtype=torch.float32, device=device)
        _EMPTY_WS[device] = ws
    return ws


def linear(x: torch.Tensor, w: torch.Tensor,
           w_packed: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x[M,K] @ w[N,K]^T. Decode-shaped (M<=64) GPU GEMMs go to the
    hand-written skinny MFMA kernel — packed-weight variant when the
    caller pre-packed W (streams at the HBM roofline); everything else to
    hipBLASLt via F.linear."""
    return _linear(x, w, w_packed, False)


def linear_partial(x: torch.Tensor, w: torch.Tensor,
                   w_packed: Optional[torch.Tensor] = None):
    """linear() for a result whose only consumer is fused_add_rmsnorm:
    same dispatch, but a split-K skinny GEMM skips its combine launch and
    returns a SplitKPartial for the norm to reduce. Everything else (CPU,
    hipBLASLt, split 1, SPLITK_DEFER_DISABLED) returns the bf16 tensor."""
    return _linear(x, w, w_packed, not SPLITK_DEFER_DISABLED)


def _linear(x, w, w_packed, defer: bool):
    M, K = x.shape
    N = w.size(0)
    tuned = _SKINNY_SHAPES.get((N, K))
    if (x.is_cuda and M <= 64 and N % 64 == 0 and K % 256 == 0
            and (tuned is not None or SKINNY_FORCED) and not SKINNY_DISABLED):
        mod = _dispatch("skinny_gemm", x)
        split, kc, nw = tuned if tuned else (_skinny_split(N // 64, K), 128, 1)
        if SKINNY_KC:
            kc = SKINNY_KC
        if K % (kc * split):
            split = _skinny_split(N // 64, K)
        defer = defer and split > 1 and M >= 1
        if defer:
            slot = _skinny_ws_slot(x.device, N, split)
            ws = slot.buf
            out = torch.empty(0, dtype=x.dtype, device=x.device)  # unwritten
        else:
            ws = _skinny_ws(x.device, N, split)
            out = torch.empty(M, N, dtype=x.dtype, device=x.device)
        if w_packed is not None:
            mod.skinny_gemm_packed(out, x.contiguous(), w_packed, N, K, ws,
                                   split, SKINNY_NT, kc, not defer, nw)
        else:
            mod.skinny_gemm(out, x.contiguous(), w, ws, split, not defer)
        return SplitKPartial(slot, split, M, N) if defer else out
    return torch.nn.functional.linear(x, w)


def quantize_weight_fp8(w: torch.Tensor):
    """Offline per-output-channel OCP e4m3 quantization of a [N, K] weight:
    returns (fragment-linear packed bytes, f32 scales[N]). Serves the fp8
    MFMA expert decode GEMM (BASELINE config 5)."""
    sw = w.float().abs().amax(dim=1).clamp(min=1e-8) / 448.0
    scaled = (w.float() / sw[:, None]).clamp(-448.0, 448.0)
    try:
        w8 = scaled.to(torch.float8_e4m3fn).view(torch.uint8)
    except (RuntimeError, TypeError):
        w8 = scaled.cpu().to(torch.float8_e4m3fn).view(torch.uint8).to(w.device)
    return _fragment_linear(w8), sw.float().contiguous()


def linear_fp8(x: torch.Tensor, w_packed: torch.Tensor, sw: torch.Tensor,
               N: int) -> torch.Tensor:
    """x[M,K] bf16 @ fp8-quantized W^T: dynamic per-token activation quant
    then the fp8 MFMA skinny GEMM (half the weight bytes of bf16)."""
    M, K = x.shape
    mod = _dispatch("skinny_gemm_fp8", x)
    assert mod is not None, "linear_fp8 is GPU-only"
    xc = x.contiguous()
    x8 = torch.empty(M, K, dtype=torch.uint8, device=x.device)
    sx = torch.empty(M, dtype=torch.float32, device=x.device)
    mod.quant_fp8_rows(x8, sx, xc)
    split = _skinny_split(N // 64, K)
    ws = _skinny_ws(x.device, N, split)
    out = torch.empty(M, N, dtype=x.dtype, device=x.device)
    mod.skinny_gemm_fp8(out, x8, sx, w_packed, sw, N, K, ws, split)
    return out


# e2m1 (fp4) code values, index = code (bit 3 = sign)
_FP4_GRID = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
# operand-role combo for the scaled MFMA (validated on hardware via
# tests/test_gpu_ops.py::test_mxfp4_gemm; override for probing only)
MXFP4_COMBO = int(os.environ.get("AGENTAINER_MXFP4_COMBO", "0"))


def quantize_weight_mxfp4(w: torch.Tensor):
    """Offline MXFP4 quantization of a [N, K] weight for the block-scaled
    MFMA expert GEMM (gfx950 v_mfma_scale_f32_16x16x128_f8f6f4): e2m1
    codes, 2 per byte, with one e8m0 scale per (row, 64-element k-block)
    — the scale granularity the instruction's scale lanes expose
    (tools/mx_probe.py). Returns (packed codes [N*K/2] u8 fragment-linear,
    scales [N/16 * K/128 * 32] u8 e8m0, kernel-ordered)."""
    N, K = w.shape
    assert N % 16 == 0 and K % 128 == 0, "MXFP4: N%16==0, K%128==0"
    wf = w.float().view(N, K // 32, 32)          # true MX block-32
    amax = wf.abs().amax(dim=-1).clamp(min=1e-8)
    # e8m0 scale 2^e with amax/2^e <= 6 (e2m1 max)
    e = torch.ceil(torch.log2(amax / 6.0)).clamp(-127, 127)
    scale = torch.pow(2.0, e)
    q = wf / scale.unsqueeze(-1)
    # nearest e2m1 via bucketize on the midpoints (device-native: this
    # runs at model load for up to 512 Mixtral expert matrices)
    mids = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0],
                        device=wf.device)
    idx = torch.bucketize(q.abs().contiguous(), mids)
    codes = (idx + torch.where(q < 0, 8, 0)).to(torch.uint8).view(N, K)
    # pack 2 codes/byte along k (lo nibble = even k)
    by = (codes[:, 0::2] | (codes[:, 1::2] << 4))  # [N, K/2]
    # fragment-linear: B lane map (probed):
    # B[(l/16)*32 + j][l%16] -> W[tile*16 + l%16][kc*128 + (l/16)*32 + j],
    # 32 codes = 16 bytes per lane
    byv = by.view(N // 16, 16, K // 128, 4, 16)     # [T][col][kc][q][16B]
    packed = byv.permute(0, 2, 3, 1, 4).contiguous().view(-1)
    # scales: one e8m0 per (col, 32-block); scale lane l covers
    # (kb = l/16, col = l%16) -> scv[T][kc][kb][col], 64 B per fragment
    e8 = (e + 127).clamp(0, 254).to(torch.uint8).view(N, K // 32)
    scv = e8.view(N // 16, 16, K // 128, 4).permute(0, 2, 3, 1).contiguous()
    return packed.to(w.device), scv.view(-1).to(w.device)


def dequantize_mxfp4(packed: torch.Tensor, scales: torch.Tensor,
                     N: int, K: int) -> torch.Tensor:
    """CPU reference inverse of quantize_weight_mxfp4 (tests/oracles)."""
    p = packed.cpu().view(N // 16, K // 128, 4, 16, 16)
    by = p.permute(0, 3, 1, 2, 4).contiguous().view(N, K // 2)
    lo = (by & 0xF).long()
    hi = (by >> 4).long()
    codes = torch.stack([lo, hi], dim=-1).view(N, K)
    vals = _FP4_GRID[codes & 7] * torch.where(codes >= 8, -1.0, 1.0)
    sc = scales.cpu().view(N // 16, K // 128, 4, 16).permute(0, 3, 1, 2)
    sc = sc.contiguous().view(N, K // 32).float()
    sc = torch.pow(2.0, sc - 127)
    return (vals.view(N, K // 32, 32) * sc.unsqueeze(-1)).view(N, K)


def linear_mxfp4(x: torch.Tensor, w_packed: torch.Tensor,
                 w_scales: torch.Tensor, N: int) -> torch.Tensor:
    """x[M,K] bf16 @ MXFP4 W^T: per-row e2m1 activation quant + the
    block-scaled 16x16x128 fp4 MFMA — quarter the weight bytes of bf16.
    (Mixed fp8-activation x fp4-weight through the scaled MFMA NaNs on
    this silicon/compiler — tools/mx_probe.py — so both operands run
    e2m1; activations carry a per-row f32 scale applied in the
    epilogue.)"""
    M, K = x.shape
    mod = _dispatch("skinny_gemm_mxfp4", x)
    assert mod is not None, "linear_mxfp4 is GPU-only"
    xc = x.contiguous()
    x8 = torch.empty(M, K // 2, dtype=torch.uint8, device=x.device)
    sx = torch.empty(M, dtype=torch.float32, device=x.device)
    mod.quant_fp4_rows(x8, sx, xc)
    split = _skinny_split(N // 64, K)
    ws = _skinny_ws(x.device, N, split)
    out = torch.empty(M, N, dtype=x.dtype, device=x.device)
    mod.skinny_gemm_mxfp4(out, x8, sx, w_packed, w_scales, N, K, ws, split,
                          MXFP4_COMBO)
    return out


def linear_quant(x: torch.Tensor, qt) -> torch.Tensor:
    """Dispatch a quantized decode GEMM: qt = (kind, packed, scales, N)
    with kind "mxfp4" or "fp8" (engine.dense_quant / expert paths)."""
    kind, packed, scales, N = qt
    if kind == "mxfp4":
        return linear_mxfp4(x, packed, scales, N)
    return linear_fp8(x, packed, scales, N)


class Projection:
    """A static [N, K] projection weight (kept by reference) with at most
    one decode form, and the one rule for which GEMM it takes: pack()
    builds the bf16 fragment-linear copy, pack("fp8" | "mxfp4") the
    quantized form instead."""
    __slots__ = ("w", "packed", "quant")

    def __init__(self, w: torch.Tensor):
        self.w = w
        self.packed = None  # pack_weight(w)
        self.quant = None   # linear_quant's (kind, packed, scales, N)

    @property
    def kind(self) -> Optional[str]:
        if self.quant is not None:
            return self.quant[0]
        return "bf16" if self.packed is not None else None

    @torch.no_grad()
    def pack(self, quant: str = "") -> "Projection":
        self.packed = self.quant = None
        if quant == "":
            self.packed = pack_weight(self.w.data)
        else:
            quantize = {"fp8": quantize_weight_fp8,
                        "mxfp4": quantize_weight_mxfp4}[quant]
            self.quant = (quant, *quantize(self.w.data), self.w.size(0))
        return self

    def __call__(self, x: torch.Tensor, defer: bool = False):
        """x[M,K] @ w^T. The quantized form serves decode-shaped GPU
        batches and wins over defer; everything else is linear(), or
        with defer linear_partial() (the result may be a SplitKPartial)."""
        if self.quant is not None and x.size(0) <= 64 and x.is_cuda:
            return linear_quant(x, self.quant)
        return _linear(x, self.w, self.packed,
                       defer and not SPLITK_DEFER_DISABLED)


def lora_shrink(v, x, A, ids):
    """v[t, :] = A[ids[t]] @ x[t] (f32 [T, R]); rows with ids[t] < 0 get
    zeros. x bf16 [T, K] (row-strided), A bf16 [S, R, K], ids int32 [T]."""
    mod = _dispatch("lora_shrink", x)
    if mod:
        mod.lora_shrink(v, x, A, ids)
    else:
        reference.lora_shrink(v, x, A, ids)
    return v


def lora_expand_add(y, v, B, ids):
    """y[t, :] += B[ids[t]] @ v[t] in place (y bf16 [T, N], row-strided;
    B bf16 [S, N, R]); rows with ids[t] < 0 are left untouched."""
    mod = _dispatch("lora_expand_add", y)
    if mod:
        mod.lora_expand_add(y, v, B, ids)
    else:
        reference.lora_expand_add(y, v, B, ids)
    return y


_lora_ws_cache = {}


def _lora_ws(device, n: int) -> torch.Tensor:
    # keyed like _skinny_ws_slot: a side-stream prefill must not write the
    # rank-space buffer a decode graph on another stream is still reading
    stream = (torch.cuda.current_stream(device).cuda_stream
              if device.type == "cuda" else 0)
    key = (device, stream)
    ws = _lora_ws_cache.get(key)
    if ws is None or ws.numel() < n:
        ws = torch.empty(n, dtype=torch.float32, device=device)
        _lora_ws_cache[key] = ws
    return ws


def lora_apply(y, x, A, B, ids):
    """y += B[ids] @ (A[ids] @ x) per row: shrink into a cached f32
    workspace, then expand-add into y in place."""
    T, R = x.size(0), A.size(1)
    if T == 0:
        return y
    v = _lora_ws(x.device, T * R)[:T * R].view(T, R)
    lora_shrink(v, x, A, ids)
    lora_expand_add(y, v, B, ids)
    return y


def gather_kv_pages(dst, k_cache, v_cache, page_ids):
    mod = _dispatch("gather_kv_pages", k_cache)
    if mod:
        mod.gather_kv_pages(dst, k_cache, v_cache, page_ids)
    else:
        reference.gather_kv_pages(dst, k_cache, v_cache, page_ids)


def scatter_kv_pages(k_cache, v_cache, src, page_ids):
    mod = _dispatch("scatter_kv_pages", k_cache)
    if mod:
        mod.scatter_kv_pages(k_cache, v_cache, src, page_ids)
    else:
        reference.scatter_kv_pages(k_cache, v_cache, src, page_ids)
