"""Decode step state: the batch buckets with their staging buffers and
captured graphs, and the record of a speculative step in flight.
ModelInstance owns the capture, the launch and the resolve; what is here
are the buffers and the copies that feed them."""

from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any, List, Optional, Set

import torch

from .request import GenRequest
from .sampling import PendingLogprobs


def bucket(n: int) -> int:
    """Decode batch sizes are rounded up to a power of two: one captured
    graph per bucket."""
    b = 1
    while b < n:
        b <<= 1
    return b


def prefill_bucket(n: int) -> int:
    """Round a prefill token count up to a small set of GEMM shapes.

    hipBLASLt runs its (CPU-expensive) algorithm heuristic per NEW
    problem shape; real-text prompts make nearly every prefill batch
    a never-seen M, which measured as ~100 ms of pure CPU per prefill
    under HTTP serving (tools/server_load.py engine_mode.pf_cpu_ms).
    Bucketing M to powers of two keeps the library cache warm after
    one occurrence of each bucket."""
    b = 32
    while b < n:
        b <<= 1
    return b


@dataclass
class SpecStep:
    """The speculative decode step in flight: its rows, their device
    sample, the rows found finished after the launch (their outputs are
    discarded), and the logprobs kernel's own output tensors (or None),
    not the graph's logits buffer that the next replay overwrites."""
    reqs: List[GenRequest]
    sampled: torch.Tensor
    invalid: Set[int] = field(default_factory=set)
    logprobs: Optional[PendingLogprobs] = None


@dataclass
class DecodeBucket:
    """One batch bucket's graph inputs (rows: sequence slots, ids: input
    tokens, inc: length increments), their pinned staging twins, and the
    captured graph with its logits buffer (None: run eager)."""
    rows: torch.Tensor
    ids: torch.Tensor
    inc: torch.Tensor
    rows_pin: torch.Tensor
    ids_pin: torch.Tensor
    h2d_ev: Optional[Any] = None  # set by the first stage() on a GPU
    graph: Optional[Any] = None
    logits: Optional[torch.Tensor] = None

    @classmethod
    def alloc(cls, size: int, pad_slot: int, device: str) -> "DecodeBucket":
        pin = device.startswith("cuda")
        return cls(
            rows=torch.full((size,), pad_slot, dtype=torch.long, device=device),
            ids=torch.zeros(size, dtype=torch.long, device=device),
            inc=torch.ones(size, dtype=torch.int32, device=device),
            rows_pin=torch.full((size,), pad_slot, dtype=torch.long,
                                pin_memory=pin),
            ids_pin=torch.zeros(size, dtype=torch.long, pin_memory=pin))

    def stage(self, slots: List[int], feed: List[int], pad_slot: int,
              ids_full: bool) -> None:
        """Copy one step's row slots and host-known input tokens (feed[i]
        < 0: none) to the graph inputs. ids_full keeps the synchronous
        path's copy of the pad rows' stale ids: eager Mixtral at 65+ rows
        shapes its expert GEMMs by them."""
        B = len(slots)
        is_gpu = self.rows.is_cuda
        # the PREVIOUS step's non-blocking H2D copies read these pinned
        # staging buffers; wait for that DMA before rewriting them (a
        # torn read would feed wrong slots/tokens into the graph)
        ev = self.h2d_ev if is_gpu else None
        if ev is not None:
            ev.synchronize()
        self.rows_pin[:B] = torch.tensor(slots, dtype=torch.long)
        self.rows_pin[B:] = pad_slot
        self.rows.copy_(self.rows_pin, non_blocking=True)
        self.ids_pin[:B] = torch.tensor([max(t, 0) for t in feed],
                                        dtype=torch.long)
        n = None if ids_full else B
        self.ids[:n].copy_(self.ids_pin[:n], non_blocking=True)
        if is_gpu:
            if ev is None:
                ev = self.h2d_ev = torch.cuda.Event()
            ev.record()
