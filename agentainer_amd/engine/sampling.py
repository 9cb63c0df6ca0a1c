"""From a logits tensor to (tokens, logprobs): stateless functions over the
sampler kernels in ops. Rank 0 feeds them from GenRequests (request_rows),
TP workers from the async plan's rows; given bitwise-identical logits and
the same rows, every rank samples the same tokens."""

from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Tuple

import torch

from .. import ops
from .request import ExtSpec, GenRequest

SEED_MASK = 0x7FFFFFFFFFFFFFFF


def request_rows(reqs: List[GenRequest], carried: Optional[List[bool]] = None):
    """(temps, tops, seeds, ext) of a batch of requests. A row's effective
    seed is seed + len(generated). A row carried over on the device
    (async decode) has ONE unresolved token in flight ahead of this sample
    (generated is appended at resolve, one step later), so its counter
    runs one ahead: this keeps the sampled stream identical to the
    synchronous path's. ext is per-row GenRequest.ext_spec(), or None when
    no row is extended (the common case: nothing is built)."""
    seeds = [(r.seed + len(r.generated)
              + (1 if carried is not None and carried[i] else 0)) & SEED_MASK
             for i, r in enumerate(reqs)]
    ext = ([r.ext_spec() for r in reqs]
           if any(r.extended for r in reqs) else None)
    return ([r.temperature for r in reqs], [r.top_p for r in reqs], seeds, ext)


def bf16_rows(logits: torch.Tensor) -> torch.Tensor:
    """The logits as every kernel here reads them; the model's own bf16
    rows come back as they are."""
    return logits.to(torch.bfloat16).contiguous()


def sample(logits: torch.Tensor, temps: List[float], tops: List[float],
           seeds: List[int], ext: Optional[List[Optional[ExtSpec]]] = None,
           pending: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One token per row, int64 [B] on the logits' device.

    Rows form up to three groups, launched in this order: rows with an
    ext[i] (greedy or not) by ops.sample_ex, the other rows with
    temperature <= 0 by ops.greedy_sample, the rest by ops.topp_sample.
    Each group's rows keep their batch order, and a kernel sees a row's
    index within its group (the top-p draw is seeded with it). pending
    (device int64 [B], -1 = none) holds each row's token that is still in
    flight on the device (async decode)."""
    B = logits.size(0)
    dev = logits.device
    out = torch.empty(B, dtype=torch.long, device=dev)
    ext_rows = ([i for i in range(B) if ext[i] is not None]
                if ext is not None else [])
    plain = ([i for i in range(B) if ext[i] is None]
             if ext_rows else range(B))
    greedy_rows = [i for i in plain if temps[i] <= 0.0]
    samp_rows = [i for i in plain if temps[i] > 0.0]
    lb = bf16_rows(logits)

    def group(rows: List[int], launch: Callable) -> None:
        """launch(out, logits) over rows: on the whole batch in place,
        else gather / launch / scatter."""
        if not rows:
            return
        if len(rows) == B:
            launch(out, lb)
        else:
            sub = torch.empty(len(rows), dtype=torch.long, device=dev)
            launch(sub, lb[rows].contiguous())
            out[rows] = sub

    def launch_ex(o, lg):
        specs = [ext[i] for i in ext_rows]
        pend = pending
        if pend is not None and len(ext_rows) < B:
            pend = pend.index_select(0, torch.tensor(
                ext_rows, dtype=torch.long, device=dev))
        ops.sample_ex(
            o, lg, [temps[i] for i in ext_rows], [tops[i] for i in ext_rows],
            [seeds[i] for i in ext_rows], [sp.top_k for sp in specs],
            [sp.min_p for sp in specs], [sp.rep for sp in specs],
            [sp.pres for sp in specs], [sp.freq for sp in specs],
            [sp.edits for sp in specs], pending=pend)

    def launch_topp(o, lg):
        def vec(vals, dtype):
            return torch.tensor([vals[i] for i in samp_rows], dtype=dtype,
                                device=dev)
        ops.topp_sample(o, lg, vec(temps, torch.float32),
                        vec(tops, torch.float32), vec(seeds, torch.int64))

    group(ext_rows, launch_ex)
    group(greedy_rows, ops.greedy_sample)
    group(samp_rows, launch_topp)
    return out


@dataclass
class PendingLogprobs:
    """A launched ops.token_logprobs call: the rows that asked, each one's
    top_logprobs, and the kernel's three outputs still on the device."""
    rows: List[int]
    tops: List[int]
    chosen_lp: torch.Tensor
    top_id: torch.Tensor
    top_lp: torch.Tensor

    def fetch(self) -> Dict[int, Tuple]:
        """Bring the result to the host (a sync point, taken beside the
        sampled tokens' own): row -> (logprob, [(token, logprob)] cut down
        to that row's top_logprobs)."""
        chosen_lp, top_id, top_lp = (self.chosen_lp.tolist(),
                                     self.top_id.tolist(),
                                     self.top_lp.tolist())
        return {i: (chosen_lp[j],
                    [(t, p) for t, p in zip(top_id[j][:n], top_lp[j][:n])
                     if t >= 0])
                for j, (i, n) in enumerate(zip(self.rows, self.tops))}


def launch_logprobs(logits: torch.Tensor, reqs: List[GenRequest],
                    sampled: torch.Tensor) -> Optional[PendingLogprobs]:
    """ops.token_logprobs right behind the sampler, in its stream, over
    the rows that ask, with K the largest top_logprobs among them. logits
    are bf16_rows', the tensor the sampler was handed. Returns None
    (nothing launched or built) when no row asks. Rank 0 only: the kernel
    holds no collective and only rank 0 answers clients."""
    rows = [i for i, r in enumerate(reqs) if r.logprobs]
    if not rows:
        return None
    tops = [reqs[i].top_logprobs for i in rows]
    rows_t = torch.tensor(rows, dtype=torch.int32).to(
        logits.device, non_blocking=True)
    return PendingLogprobs(
        rows, tops, *ops.token_logprobs(logits, rows_t, sampled, max(tops)))
