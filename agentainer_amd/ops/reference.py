"""Pure-PyTorch fp32 reference implementations of every HIP op.

Dual purpose (SURVEY.md §4 test strategy):
  * the numerics oracle for the GPU kernel tests (kernel output vs the
    fp32 reference of the same op, tolerance-gated);
  * the CPU execution path of the engine, so the full control plane +
    scheduler run (and are tested) on GPU-less CI.

Tensors use the same shapes/layouts as the HIP kernels, including the
paged-cache layouts k_cache [P, n_kv, D/8, PS, 8] / v_cache [P, n_kv, PS, D].
"""

from __future__ import annotations


import torch


def rmsnorm(out: torch.Tensor, x: torch.Tensor, w: torch.Tensor, eps: float) -> None:
    xf = x.float()
    r = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    out.copy_((r * w.float()).to(out.dtype))


def fused_add_rmsnorm(out: torch.Tensor, x: torch.Tensor, residual: torch.Tensor,
                      w: torch.Tensor, eps: float) -> None:
    s = (x.float() + residual.float())
    residual.copy_(s.to(residual.dtype))
    sf = residual.float()  # match kernel: normalizes the bf16-rounded sum
    r = sf * torch.rsqrt(sf.pow(2).mean(-1, keepdim=True) + eps)
    out.copy_((r * w.float()).to(out.dtype))


def silu_mul(out: torch.Tensor, gate: torch.Tensor, up: torch.Tensor) -> None:
    g = gate.float()
    out.copy_((g * torch.sigmoid(g) * up.float()).to(out.dtype))


def make_cos_sin_table(max_pos: int, dim: int, theta: float = 500000.0,
                       device="cpu") -> torch.Tensor:
    """[max_pos, dim] f32 rows laid out [cos(0..d/2) | sin(0..d/2)]."""
    inv = 1.0 / (theta ** (torch.arange(0, dim, 2, dtype=torch.float64) / dim))
    pos = torch.arange(max_pos, dtype=torch.float64)
    ang = torch.outer(pos, inv)
    tab = torch.cat([torch.cos(ang), torch.sin(ang)], dim=-1).float()
    return tab.contiguous().to(device)


def rope_inplace(q: torch.Tensor, k: torch.Tensor, cos_sin: torch.Tensor,
                 positions: torch.Tensor) -> None:
    D = q.size(-1)
    half = D // 2
    c = cos_sin[positions.long(), :half].unsqueeze(1).float()  # [T,1,half]
    s = cos_sin[positions.long(), half:].unsqueeze(1).float()
    for t in (q, k):
        x1 = t[..., :half].float()
        x2 = t[..., half:].float()
        t[..., :half] = (x1 * c - x2 * s).to(t.dtype)
        t[..., half:] = (x1 * s + x2 * c).to(t.dtype)


def kv_append(k_cache: torch.Tensor, v_cache: torch.Tensor, k: torch.Tensor,
              v: torch.Tensor, slot_mapping: torch.Tensor) -> None:
    n_kv, D = k.size(1), k.size(2)
    PS = k_cache.size(3)
    for t in range(k.size(0)):
        slot = int(slot_mapping[t])
        if slot < 0:
            continue
        page, off = slot // PS, slot % PS
        # k_cache [P, n_kv, D/8, PS, 8]; .to() casts bf16 -> fp8 when the
        # pool is e4m3 (index-assignment alone won't cast to float8)
        k_cache[page, :, :, off, :] = (
            k[t].reshape(n_kv, D // 8, 8).to(k_cache.dtype))
        v_cache[page, :, off, :] = v[t].to(v_cache.dtype)


def _gather_kv(k_cache, v_cache, page_table_row, length, g):
    """K/V [length, D] f32 for kv head g of one sequence."""
    PS = k_cache.size(3)
    D = v_cache.size(3)
    ks, vs = [], []
    for tok in range(length):
        page = int(page_table_row[tok // PS])
        off = tok % PS
        ks.append(k_cache[page, g, :, off, :].reshape(D).float())
        vs.append(v_cache[page, g, off, :].float())
    return torch.stack(ks), torch.stack(vs)


def paged_decode_attention(out: torch.Tensor, q: torch.Tensor,
                           k_cache: torch.Tensor, v_cache: torch.Tensor,
                           page_table: torch.Tensor, seq_lens: torch.Tensor,
                           scale: float) -> None:
    B, n_q, D = q.shape
    n_kv = k_cache.size(1)
    ratio = n_q // n_kv
    for b in range(B):
        length = int(seq_lens[b])
        if length <= 0:
            out[b] = 0  # graph pad row (dev_seq_lens == -1); HIP kernel skips
            continue
        for g in range(n_kv):
            K, V = _gather_kv(k_cache, v_cache, page_table[b], length, g)
            for qh in range(g * ratio, (g + 1) * ratio):
                s = (K @ q[b, qh].float()) * scale
                p = torch.softmax(s, dim=-1)
                out[b, qh] = (p @ V).to(out.dtype)


def paged_prefill_attention(out: torch.Tensor, q: torch.Tensor,
                            k_cache: torch.Tensor, v_cache: torch.Tensor,
                            page_table: torch.Tensor, seq_lens: torch.Tensor,
                            query_starts: torch.Tensor, query_lens: torch.Tensor,
                            scale: float) -> None:
    n_q = q.size(1)
    n_kv = k_cache.size(1)
    ratio = n_q // n_kv
    B = seq_lens.numel()
    for b in range(B):
        qlen = int(query_lens[b])
        if qlen == 0:
            continue
        total = int(seq_lens[b])
        start = int(query_starts[b])
        ctx_start = total - qlen
        for g in range(n_kv):
            K, V = _gather_kv(k_cache, v_cache, page_table[b], total, g)
            for qh in range(g * ratio, (g + 1) * ratio):
                Q = q[start:start + qlen, qh].float()       # [qlen, D]
                s = Q @ K.t() * scale                       # [qlen, total]
                qpos = ctx_start + torch.arange(qlen).unsqueeze(1)
                kpos = torch.arange(total).unsqueeze(0)
                s = s.masked_fill(kpos > qpos, float("-inf"))
                p = torch.softmax(s, dim=-1)
                out[start:start + qlen, qh] = (p @ V).to(out.dtype)


def greedy_sample(out: torch.Tensor, logits: torch.Tensor) -> None:
    out.copy_(logits.float().argmax(dim=-1))


def topp_sample(out: torch.Tensor, logits: torch.Tensor, temps: torch.Tensor,
                top_ps: torch.Tensor, seeds: torch.Tensor) -> None:
    """Reference nucleus sampling. Uses torch RNG seeded per row so results
    are deterministic given seeds (NOT bitwise-matched to the HIP kernel —
    distribution-level tests only)."""
    B, V = logits.shape
    for b in range(B):
        gen = torch.Generator(device="cpu").manual_seed(int(seeds[b]) & 0x7FFFFFFF)
        p = torch.softmax(logits[b].float() / max(float(temps[b]), 1e-6), dim=-1)
        sp, idx = p.sort(descending=True)
        cum = sp.cumsum(0)
        cut = int(torch.searchsorted(cum, float(top_ps[b])).item()) + 1
        cut = min(cut, V)
        sp = sp[:cut] / sp[:cut].sum()
        pick = idx[torch.multinomial(sp.cpu(), 1, generator=gen)]
        out[b] = pick.to(out.device)


SAMPLE_EX_CAP = 1024  # candidate capacity of the extended sampler
_M64 = (1 << 64) - 1


def uniform01(seed: int, row: int) -> float:
    """Integer port of the kernels' per-row hash (csrc/common.h): the
    CPU reference and the GPU draw from the same u for (seed, row)."""
    x = ((int(seed) & _M64) ^ (0x9E3779B97F4A7C15 * (int(row) + 1))) & _M64
    x ^= x >> 12
    x ^= (x << 25) & _M64
    x ^= x >> 27
    x = (x * 0x2545F4914F6CDD1D) & _M64
    return ((x >> 40) & 0xFFFFFF) / 16777216.0


def sample_ex_edit_row(logits_row: torch.Tensor, rep: float, pres: float,
                       freq: float, toks, cnts, biases,
                       pending: int = -1) -> torch.Tensor:
    """The edited f32 logits of one row (the kernel's workspace row).
    toks are unique; cnts[i] = 2 * c + in_prompt; pending (-1: none) is
    one more generated occurrence that the host lists do not hold yet."""
    V = logits_row.numel()
    l = logits_row.detach().float().cpu().clone()
    toks = [int(t) for t in toks]
    cnts = [int(c) for c in cnts]
    biases = [float(b) for b in biases]
    if 0 <= pending < V:
        if pending in toks:
            cnts[toks.index(pending)] += 2
        else:
            toks.append(int(pending)); cnts.append(2); biases.append(0.0)
    if not toks:
        return l
    idx = torch.tensor(toks, dtype=torch.long)
    cnt = torch.tensor(cnts, dtype=torch.int64)
    c = (cnt >> 1).to(torch.float32)
    v = l[idx]
    f32 = lambda x: torch.tensor(float(x), dtype=torch.float32)
    # 1. repetition (sign-dependent), 2. frequency + presence, 3. bias;
    # every step rounds to f32, as the kernel's explicit roundings do
    v = torch.where(cnt > 0, torch.where(v > 0, v / f32(rep), v * f32(rep)), v)
    pen = f32(freq) * c + torch.where(c > 0, f32(pres), f32(0.0))
    v = v - pen
    v = v + torch.tensor(biases, dtype=torch.float32)
    l[idx] = v
    return l


def sample_ex_kept(edited: torch.Tensor, temp: float, top_p: float,
                   min_p: float, top_k: int):
    """float64 selection of one sampled row: (ids of the kept prefix in
    (p desc, id asc) order, their cumulative p)."""
    V = edited.numel()
    s = edited.double() / float(temp)
    p = torch.exp(s - s.max())
    total = p.sum()
    n0 = min(int(top_k) if int(top_k) > 0 else SAMPLE_EX_CAP, SAMPLE_EX_CAP, V)
    # stable sort on -p keeps ascending ids among equal p
    order = torch.sort(-p, stable=True).indices[:n0]
    sp = p[order]
    n_minp = int((sp >= float(min_p) * sp[0]).sum())
    cum = sp.cumsum(0)
    n_topp = n0
    if float(top_p) < 1.0:
        hit = (cum / total >= float(top_p)).nonzero()
        if hit.numel():
            n_topp = int(hit[0]) + 1
    keep = max(1, min(n0, n_minp, n_topp))
    return order[:keep], cum[:keep]


def sample_ex(out: torch.Tensor, logits: torch.Tensor, ws, temps, top_ps,
              min_ps, reps, press, freqs, top_ks, seeds, edit_ptr, edit_tok,
              edit_cnt, edit_bias, pending_tok, rows=None) -> None:
    """Definition of the extended sampler (csrc/sample_ex.hip follows it).

    Per row, in f32 on the bf16 logit l of token t, with seen(t) = t is in
    the request's prompt or was generated, c(t) = times generated:
      1. seen:  l = l / rep if l > 0 else l * rep
      2. l -= freq * c + pres * (c > 0)
      3. l += bias(t)
    The edits come as CSR rows of unique tokens with
    edit_cnt = 2 * c + in_prompt; pending_tok[b] >= 0 counts as one more
    generated occurrence (async decode: the newest token is still on the
    device). temperature <= 0 takes the argmax of the edited row, lowest
    id on ties. Otherwise s = l / T, p = exp(s - max), total = sum of p
    over the whole row; tokens are sorted by (p desc, id asc); the
    candidates are the first n0 = min(top_k or 1024, 1024, V); the kept
    prefix has length min(n0, n_minp, n_topp) with n_minp the count of
    candidates with p >= min_p * p_max and n_topp the smallest n whose
    cumulative p / total >= top_p (top_p >= 1: no nucleus cut); the draw
    is the inverse CDF over the kept prefix at u = uniform01(seed, row).

    Known limitation: a nucleus wider than 1024 tokens is truncated to
    the top 1024 (topp_sample truncates at 512).

    rows: the row index hashed with each seed (default: the batch index,
    as the kernel uses). ws, when given, receives the edited f32 rows."""
    B, V = logits.shape
    ptr = [int(x) for x in edit_ptr.tolist()]
    tok = edit_tok.tolist()
    cnt = edit_cnt.tolist()
    bias = edit_bias.tolist()
    pend = [int(x) for x in pending_tok.tolist()]
    for b in range(B):
        e0, e1 = ptr[b], ptr[b + 1]
        l = sample_ex_edit_row(logits[b], float(reps[b]), float(press[b]),
                               float(freqs[b]), tok[e0:e1], cnt[e0:e1],
                               bias[e0:e1], pend[b])
        if ws is not None:
            ws.view(-1)[b * V:(b + 1) * V] = l.to(ws.device)
        T = float(temps[b])
        if T <= 0.0:
            out[b] = int(l.argmax())  # first maximal index
            continue
        ids, cum = sample_ex_kept(l, T, float(top_ps[b]), float(min_ps[b]),
                                  int(top_ks[b]))
        u = uniform01(int(seeds[b]), b if rows is None else int(rows[b]))
        j = int(torch.searchsorted(cum, u * float(cum[-1])))
        out[b] = int(ids[min(j, ids.numel() - 1)])


TOP_LOGPROBS_MAX = 20


def token_logprobs(logits: torch.Tensor, rows: torch.Tensor,
                   chosen: torch.Tensor, K: int):
    """Logprobs of the model's own distribution (temperature 1, no
    penalties, bias or cuts), for the rows of bf16 logits [B, V] that the
    int32 `rows` [R] names, in that order. Returns (chosen_lp f32 [R],
    top_id int32 [R, K], top_lp f32 [R, K]).

    For b = rows[r]: lp = l - max(l) - log(sum(exp(l - max(l)))) over the
    logits widened to float, evaluated in float64 and rounded to f32 (this
    form keeps a token 80 nats below the maximum finite). chosen_lp[r] is
    lp[chosen[b]], inside the top K or not. top_id[r] holds the min(K, V)
    tokens that come first in the total order (logit descending, id
    ascending; logits compare as floats, so -0.0 ties with +0.0) and
    top_lp[r] their logprobs; slots past V hold -1 and -inf."""
    B, V = logits.shape
    K = int(K)
    assert 0 <= K <= TOP_LOGPROBS_MAX
    R = rows.numel()
    chosen_lp = torch.empty(R, dtype=torch.float32)
    top_id = torch.full((R, K), -1, dtype=torch.int32)
    top_lp = torch.full((R, K), float("-inf"), dtype=torch.float32)
    n = min(K, V)
    for r, b in enumerate(rows.tolist()):
        l = logits[b].detach().cpu().to(torch.float64) + 0.0  # -0.0 -> +0.0
        d = l - l.max()
        lp = (d - d.exp().sum().log()).to(torch.float32)
        chosen_lp[r] = lp[int(chosen[b])]
        if n:
            # a stable descending sort leaves equal logits in id order
            ids = torch.sort(l, descending=True, stable=True).indices[:n]
            top_id[r, :n] = ids.to(torch.int32)
            top_lp[r, :n] = lp[ids]
    dev = logits.device
    return chosen_lp.to(dev), top_id.to(dev), top_lp.to(dev)


def gather_kv_pages(dst: torch.Tensor, k_cache: torch.Tensor,
                    v_cache: torch.Tensor, page_ids: torch.Tensor) -> None:
    n_kv = k_cache.size(1)
    D = v_cache.size(3)
    PS = k_cache.size(3)
    plane = n_kv * D * PS
    flat = dst.view(-1)
    for i, p in enumerate(page_ids.tolist()):
        flat[i * 2 * plane:(i * 2 + 1) * plane] = k_cache[p].reshape(-1)
        flat[(i * 2 + 1) * plane:(i + 1) * 2 * plane] = v_cache[p].reshape(-1)


def scatter_kv_pages(k_cache: torch.Tensor, v_cache: torch.Tensor,
                     src: torch.Tensor, page_ids: torch.Tensor) -> None:
    n_kv = k_cache.size(1)
    D = v_cache.size(3)
    PS = k_cache.size(3)
    plane = n_kv * D * PS
    flat = src.view(-1)
    for i, p in enumerate(page_ids.tolist()):
        k_cache[p] = flat[i * 2 * plane:(i * 2 + 1) * plane].view_as(k_cache[p])
        v_cache[p] = flat[(i * 2 + 1) * plane:(i + 1) * 2 * plane].view_as(v_cache[p])


def lora_shrink(v: torch.Tensor, x: torch.Tensor, A: torch.Tensor,
                ids: torch.Tensor) -> None:
    """v[t] = A[ids[t]] @ x[t] in f32; rows with ids[t] < 0 get zeros and
    never index A."""
    v.zero_()
    live = (ids >= 0).nonzero().squeeze(1)
    if live.numel():
        a = A[ids[live].long()].float()                    # [n, R, K]
        v[live] = torch.einsum("nrk,nk->nr", a, x[live].float())


def lora_expand_add(y: torch.Tensor, v: torch.Tensor, B: torch.Tensor,
                    ids: torch.Tensor) -> None:
    """y[t] = bf16(f32(y[t]) + B[ids[t]] @ v[t]) in place; rows with
    ids[t] < 0 are not touched."""
    live = (ids >= 0).nonzero().squeeze(1)
    if live.numel():
        b = B[ids[live].long()].float()                    # [n, N, R]
        d = torch.einsum("nor,nr->no", b, v[live].float())
        y[live] = (y[live].float() + d).to(y.dtype)
