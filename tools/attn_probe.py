"""Isolated attention probes.

python tools/attn_probe.py [ctx] [batch] [fp8]
    decode attention: time + effective KV bandwidth.
python tools/attn_probe.py decode-sweep [rounds] [iters]
    decode attention at ctx 144 / 320 / 1024 / 4096, bf16 and fp8 pages:
    device-event median (min, max) and effective KV bandwidth.
python tools/attn_probe.py rope [rounds] [iters]
    rope_append at T = 64 and T = 16384, bf16 and fp8 pools.
python tools/attn_probe.py prefill [rounds] [iters]
    paged prefill attention at three shapes (bench, multi-turn, one long
    prompt), bf16 and fp8 pages: device-event time (median of `rounds`
    rounds of `iters` calls), TFLOP/s of the causal MFMA work and GB/s of
    the minimum traffic (q + out + each K/V token once).
"""
import math
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from agentainer_amd import ops

n_q, n_kv, D, PS = 32, 8, 128, 16

# (name, sequences, cached prefix, new tokens)
PREFILL_SHAPES = [("bench 64x256 ctx0", 64, 0, 256),
                  ("multi-turn 64x256 ctx1024", 64, 1024, 256),
                  ("long 1x4096 ctx0", 1, 0, 4096)]


def probe_decode(argv):
    ctx = int(argv[1]) if len(argv) > 1 else 320
    B = int(argv[2]) if len(argv) > 2 else 64
    dt = torch.float8_e4m3fn if (len(argv) > 3 and argv[3] == "fp8") \
        else torch.bfloat16
    max_pages = -(-ctx // PS)
    P = B * max_pages + 1
    kc = torch.randn(P, n_kv, D // 8, PS, 8, device="cuda").to(dt)
    vc = torch.randn(P, n_kv, PS, D, device="cuda").to(dt)
    pt = torch.arange(1, P, dtype=torch.int32, device="cuda").view(B, max_pages)
    sl = torch.full((B,), ctx, dtype=torch.int32, device="cuda")
    q = torch.randn(B, n_q, D, dtype=torch.bfloat16, device="cuda")
    out = torch.empty_like(q)
    scale = 1.0 / math.sqrt(D)
    for _ in range(20):
        ops.paged_decode_attention(out, q, kc, vc, pt, sl, scale)
    torch.cuda.synchronize()
    t0 = time.time()
    iters = 300
    for _ in range(iters):
        ops.paged_decode_attention(out, q, kc, vc, pt, sl, scale)
    torch.cuda.synchronize()
    el = (time.time() - t0) / iters
    kv_bytes = B * n_kv * ctx * 2 * D * kc.element_size()
    print(f"ctx={ctx} B={B} {str(dt).split('.')[-1]}: {el*1e6:8.1f} us  "
          f"KV {kv_bytes/1e6:.1f} MB  {kv_bytes/el/1e12:5.2f} TB/s")


def probe_decode_sweep(argv):
    """ctx 144 / 320 / 1024 / 4096 at B = 64, bf16 and fp8 pages, shuffled
    page tables, q a strided view of a qkv buffer as the model passes it.
    Device-event time: median (min, max) of `rounds` rounds of `iters`."""
    rounds = int(argv[2]) if len(argv) > 2 else 7
    iters = int(argv[3]) if len(argv) > 3 else 50
    B = 64
    scale = 1.0 / math.sqrt(D)
    for ctx in (144, 320, 1024, 4096):
        max_pages = -(-ctx // PS)
        P = B * max_pages + 1
        pt = (torch.randperm(P - 1, device="cuda").to(torch.int32) + 1) \
            .view(B, max_pages)
        sl = torch.full((B,), ctx, dtype=torch.int32, device="cuda")
        qkv = torch.randn(B, (n_q + 2 * n_kv) * D, dtype=torch.bfloat16,
                          device="cuda")
        q = qkv[:, :n_q * D].view(B, n_q, D)
        out = torch.empty(B, n_q, D, dtype=torch.bfloat16, device="cuda")
        for dt in (torch.bfloat16, torch.float8_e4m3fn):
            kc = torch.randn(P, n_kv, D // 8, PS, 8, device="cuda").to(dt)
            vc = torch.randn(P, n_kv, PS, D, device="cuda").to(dt)
            for _ in range(10):
                ops.paged_decode_attention(out, q, kc, vc, pt, sl, scale)
            torch.cuda.synchronize()
            times = []
            for _ in range(rounds):
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    ops.paged_decode_attention(out, q, kc, vc, pt, sl, scale)
                e1.record()
                e1.synchronize()
                times.append(e0.elapsed_time(e1) * 1e-3 / iters)
            el = statistics.median(times)
            kv_bytes = B * n_kv * ctx * 2 * D * kc.element_size()
            print(f"decode ctx={ctx:5d} B={B} {str(dt).split('.')[-1]:13s} "
                  f"{el*1e6:8.1f} us (min {min(times)*1e6:.1f} max "
                  f"{max(times)*1e6:.1f})  {kv_bytes/el/1e12:5.2f} TB/s",
                  flush=True)
            del kc, vc


def probe_rope_append(argv):
    """rope_append at the decode (T = 64) and prefill (T = 16384) shapes,
    strided q/k/v views of a qkv buffer, bf16 and fp8 pools."""
    rounds = int(argv[2]) if len(argv) > 2 else 7
    iters = int(argv[3]) if len(argv) > 3 else 50
    table = ops.make_cos_sin_table(8192, D, device="cuda")
    for T in (64, 16384):
        P = T // PS + 2
        qkv = torch.randn(T, (n_q + 2 * n_kv) * D, dtype=torch.bfloat16,
                          device="cuda")
        q = qkv[:, :n_q * D].view(T, n_q, D)
        k = qkv[:, n_q * D:(n_q + n_kv) * D].view(T, n_kv, D)
        v = qkv[:, (n_q + n_kv) * D:].view(T, n_kv, D)
        pos = (torch.arange(T, device="cuda") % 8192).to(torch.int32)
        slots = torch.randperm(T, device="cuda") + PS
        for dt in (torch.bfloat16, torch.float8_e4m3fn):
            kc = torch.zeros(P, n_kv, D // 8, PS, 8, device="cuda").to(dt)
            vc = torch.zeros(P, n_kv, PS, D, device="cuda").to(dt)
            for _ in range(10):
                ops.rope_append(q, k, v, kc, vc, table, pos, slots)
            torch.cuda.synchronize()
            times = []
            for _ in range(rounds):
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    ops.rope_append(q, k, v, kc, vc, table, pos, slots)
                e1.record()
                e1.synchronize()
                times.append(e0.elapsed_time(e1) * 1e-3 / iters)
            el = statistics.median(times)
            print(f"rope_append T={T:6d} {str(dt).split('.')[-1]:13s} "
                  f"{el*1e6:8.1f} us (min {min(times)*1e6:.1f} max "
                  f"{max(times)*1e6:.1f})", flush=True)


def probe_prefill(argv):
    rounds = int(argv[2]) if len(argv) > 2 else 7
    iters = int(argv[3]) if len(argv) > 3 else 20
    scale = 1.0 / math.sqrt(D)
    for name, B, ctx, new in PREFILL_SHAPES:
        total = ctx + new
        max_pages = -(-total // PS)
        P = B * max_pages + 1
        # q is the model's strided view of the fused qkv projection
        qkv = torch.randn(B * new, (n_q + 2 * n_kv) * D, dtype=torch.bfloat16,
                          device="cuda")
        q = qkv[:, :n_q * D].view(B * new, n_q, D)
        out = torch.empty(B * new, n_q, D, dtype=torch.bfloat16, device="cuda")
        pt = (torch.randperm(P - 1, device="cuda").to(torch.int32) + 1) \
            .view(B, max_pages)
        sl = torch.full((B,), total, dtype=torch.int32, device="cuda")
        qs = torch.arange(B, dtype=torch.int32, device="cuda") * new
        ql = torch.full((B,), new, dtype=torch.int32, device="cuda")
        flop = 4.0 * D * n_q * B * (new * ctx + new * (new + 1) / 2)
        for dt in (torch.bfloat16, torch.float8_e4m3fn):
            kc = torch.randn(P, n_kv, D // 8, PS, 8, device="cuda").to(dt)
            vc = torch.randn(P, n_kv, PS, D, device="cuda").to(dt)
            nbytes = (2 * B * new * n_q * D * 2
                      + 2 * B * total * n_kv * D * kc.element_size())

            def call():
                ops.paged_prefill_attention(out, q, kc, vc, pt, sl, qs, ql,
                                            scale, new)
            for _ in range(5):
                call()
            torch.cuda.synchronize()
            times = []
            for _ in range(rounds):
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    call()
                e1.record()
                e1.synchronize()
                times.append(e0.elapsed_time(e1) * 1e-3 / iters)
            el = statistics.median(times)
            print(f"prefill {name:26s} {str(dt).split('.')[-1]:13s} "
                  f"{el*1e6:8.1f} us (min {min(times)*1e6:.1f} max "
                  f"{max(times)*1e6:.1f})  {flop/el/1e12:6.1f} TFLOP/s  "
                  f"{nbytes/el/1e9:7.1f} GB/s", flush=True)
            del kc, vc


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "prefill":
        probe_prefill(sys.argv)
    elif len(sys.argv) > 1 and sys.argv[1] == "decode-sweep":
        probe_decode_sweep(sys.argv)
    elif len(sys.argv) > 1 and sys.argv[1] == "rope":
        probe_rope_append(sys.argv)
    else:
        probe_decode(sys.argv)
