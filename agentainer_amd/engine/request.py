"""What a client asks of the engine: one generation request, its sampling
controls as validated from the API, and the binding of an agent to a model.
Plain host-side records; nothing here touches a tensor."""

from __future__ import annotations

import queue
import threading
from dataclasses import dataclass, field
from typing import Any, Dict, List, NamedTuple, Optional, Tuple

DEFAULT_MAX_NEW = 64


class ExtSpec(NamedTuple):
    """One row's extended sampling controls, as ops.sample_ex takes them.
    edits lists each touched token once as (token, 2 * count + in_prompt,
    bias). The TP plan's tail (plan.encode_async) carries the same fields."""
    top_k: int
    min_p: float
    rep: float
    pres: float
    freq: float
    edits: List[Tuple[int, int, float]]


@dataclass(eq=False)
class GenRequest:
    agent_id: str
    prompt_tokens: List[int]
    max_new: int
    temperature: float
    top_p: float
    seed: int
    done: threading.Event = field(default_factory=threading.Event)
    generated: List[int] = field(default_factory=list)
    error: Optional[str] = None
    enq_t: float = 0.0
    first_token_t: float = 0.0
    fin_t: float = 0.0
    trace_id: str = ""  # WAL request id — end-to-end tracing
    # streaming: the scheduler puts each sampled token id here as it is
    # produced, then None when the request finishes (SSE /chat path)
    stream_q: Optional[Any] = None
    # chunked prefill: tokens of the prompt already written to KV, and the
    # length of the slice admitted for the CURRENT step (set by _admit)
    prefill_pos: int = 0
    slice_len: int = 0
    # set by _admit: the first prefill slice starts from a truncated KV
    # sequence (the prefill plan carries it to TP workers)
    needs_reset: bool = False
    # extended sampling controls (ops.sample_ex); a request with all of
    # them at these off values keeps the greedy_sample / topp_sample path
    top_k: int = 0
    min_p: float = 0.0
    repetition_penalty: float = 1.0
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0
    logit_bias: Dict[int, float] = field(default_factory=dict)
    # penalty state: ids of the prompt, and how often each id was
    # generated (kept by add_token, wherever `generated` grows)
    prompt_set: Optional[frozenset] = None
    gen_counts: Dict[int, int] = field(default_factory=dict)
    # logprobs of the model's own distribution (ops.token_logprobs): with
    # `logprobs` on, token_logprobs holds one entry per generated token,
    # {"token", "logprob", "top": [{"token", "logprob"}] * top_logprobs}
    logprobs: bool = False
    top_logprobs: int = 0
    token_logprobs: List[Dict[str, Any]] = field(default_factory=list)

    # whether any control above is on; fixed at construction so that the
    # per-step routing check costs one attribute read per row
    extended: bool = field(init=False, default=False)

    def __post_init__(self):
        if self.prompt_set is None:
            self.prompt_set = frozenset(self.prompt_tokens)
        self.extended = bool(
            self.top_k > 0 or self.min_p > 0.0
            or self.repetition_penalty != 1.0 or self.presence_penalty != 0.0
            or self.frequency_penalty != 0.0 or self.logit_bias)

    def add_token(self, tok: int, lp: Optional[Tuple] = None) -> None:
        """lp: a requesting row's (logprob, [(token, logprob), ...]) from
        sampling.PendingLogprobs.fetch."""
        self.generated.append(tok)
        self.gen_counts[tok] = self.gen_counts.get(tok, 0) + 1
        if self.logprobs:
            self.token_logprobs.append({
                "token": tok, "logprob": lp[0],
                "top": [{"token": t, "logprob": p} for t, p in lp[1]]})

    def ext_spec(self) -> Optional[ExtSpec]:
        """The ExtSpec of an extended request, else None. Tokens that no
        active control can change are left out of edits."""
        if not self.extended:
            return None
        toks = set(self.logit_bias)
        if self.repetition_penalty != 1.0:
            toks |= self.prompt_set
        if (self.repetition_penalty != 1.0 or self.presence_penalty != 0.0
                or self.frequency_penalty != 0.0):
            toks.update(self.gen_counts)
        edits = [(t, 2 * self.gen_counts.get(t, 0) + (t in self.prompt_set),
                  self.logit_bias.get(t, 0.0)) for t in sorted(toks)]
        return ExtSpec(self.top_k, self.min_p, self.repetition_penalty,
                       self.presence_penalty, self.frequency_penalty, edits)


SAMPLING_TOP_K_MAX = 1024
SAMPLING_MAX_BIASES = 300
SAMPLING_TOP_LOGPROBS_MAX = 20  # ops.token_logprobs' K


def parse_sampling_controls(sampling: Dict[str, Any], vocab: int) -> Dict[str, Any]:
    """Validate the extended sampling keys of a merged sampling dict and
    return them as GenRequest keyword arguments (`logprobs` and
    `top_logprobs` only when logprobs are asked for). Raises ValueError on
    an ill-typed or out-of-range value."""
    def num(key, default, lo, hi, lo_open=False):
        v = sampling.get(key, default)
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise ValueError(f"sampling.{key} must be a number, got {v!r}")
        v = float(v)
        if (v != v or abs(v) == float("inf") or v > hi or v < lo
                or (lo_open and v <= lo)):
            raise ValueError(f"sampling.{key}={v} out of range")
        return v

    top_k = sampling.get("top_k", 0)
    if isinstance(top_k, bool) or not isinstance(top_k, int):
        raise ValueError(f"sampling.top_k must be an integer, got {top_k!r}")
    if not 0 <= top_k <= SAMPLING_TOP_K_MAX:
        raise ValueError(
            f"sampling.top_k={top_k} out of range [0, {SAMPLING_TOP_K_MAX}]")
    raw = sampling.get("logit_bias") or {}
    if not isinstance(raw, dict):
        raise ValueError("sampling.logit_bias must be an object {token_id: bias}")
    if len(raw) > SAMPLING_MAX_BIASES:
        raise ValueError(f"sampling.logit_bias has {len(raw)} entries "
                         f"(max {SAMPLING_MAX_BIASES})")
    bias: Dict[int, float] = {}
    for k, v in raw.items():
        try:
            t = int(k)
        except (TypeError, ValueError):
            raise ValueError(f"sampling.logit_bias key {k!r} is not a token id")
        if isinstance(k, (bool, float)) or not 0 <= t < vocab:
            raise ValueError(
                f"sampling.logit_bias token id {k!r} outside [0, {vocab})")
        if isinstance(v, bool) or not isinstance(v, (int, float)) \
                or not -100.0 <= float(v) <= 100.0:
            raise ValueError(
                f"sampling.logit_bias[{k}]={v!r} outside [-100, 100]")
        if t in bias:
            raise ValueError(f"sampling.logit_bias token id {t} given twice")
        bias[t] = float(v)
    want_lp = sampling.get("logprobs", False)
    if not isinstance(want_lp, bool):
        raise ValueError(f"sampling.logprobs must be a boolean, got {want_lp!r}")
    top_lp = sampling.get("top_logprobs", 0)
    if isinstance(top_lp, bool) or not isinstance(top_lp, int):
        raise ValueError(
            f"sampling.top_logprobs must be an integer, got {top_lp!r}")
    if not 0 <= top_lp <= SAMPLING_TOP_LOGPROBS_MAX:
        raise ValueError(f"sampling.top_logprobs={top_lp} out of range "
                         f"[0, {SAMPLING_TOP_LOGPROBS_MAX}]")
    if top_lp and not want_lp:
        raise ValueError("sampling.top_logprobs requires sampling.logprobs")
    controls = dict(
        top_k=top_k,
        min_p=num("min_p", 0.0, 0.0, 1.0),
        repetition_penalty=num("repetition_penalty", 1.0, 0.0,
                               float("inf"), lo_open=True),
        presence_penalty=num("presence_penalty", 0.0, -2.0, 2.0),
        frequency_penalty=num("frequency_penalty", 0.0, -2.0, 2.0),
        logit_bias=bias,
    )
    if want_lp:
        controls.update(logprobs=True, top_logprobs=top_lp)
    return controls


@dataclass
class AgentBinding:
    agent: Any
    model_name: str
    seq_id: str
    paused: bool = False
    requests: int = 0
    tokens: int = 0
    # /clear: the next admitted request prefills onto a reset KV sequence
    # (plan-mirrored to TP workers via needs_reset)
    pending_reset: bool = False
    queue: "queue.Queue[GenRequest]" = field(default_factory=queue.Queue)
    active: Optional[GenRequest] = None
    # whole-page token prefix shared with other agents (system prompt),
    # None when the system prompt is shorter than one KV page
    prefix_tokens: Optional[List[int]] = None
    # LoRA adapter (canonical directory path) and its pool slot; "" / -1
    # for a base-model agent
    adapter: str = ""
    adapter_slot: int = -1
