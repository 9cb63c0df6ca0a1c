"""Wire format of the TP plan channel's int-vector commands: rank 0 encodes,
workers decode (parallel.dist.send_ints / recv_cmd); op 0 is reserved for
pickled commands. tests/test_decode_plan.py pins the bytes."""

from __future__ import annotations

import struct
from dataclasses import dataclass, field
from typing import Callable, List, Optional, Tuple

from .. import parallel as par
from .request import ExtSpec

OP_DECODE = 1   # [OP, model_idx, B, slot*B, token*B] — the per-step hot path
OP_BARRIER = 2  # [OP] — timing fence (bench.py --tp)
# async (speculative) decode: rollbacks from the previous resolve are
# prepended, then per-row (slot, token|-1, prev_idx, eff_seed, temp_bits,
# top_p_bits) — workers feed carried-over rows from their OWN previous
# device sample (logits are bitwise-identical across ranks after the
# all-reduce, and sampling is seed-deterministic, so every rank samples
# the same token without any extra communication)
# When a row uses the extended sampling controls a tail follows the 6*B
# block: n_ext, then per extended row [row, top_k, bits(min_p, rep, pres,
# freq, top_p), n_edits, (tok, cnt, bias bits) * n_edits]; without one the
# vector is unchanged. A tail too long for the fixed plan buffer (long
# prompts under a repetition penalty) travels ahead as a pickled
# ("ext_tail", model name, tail) command and the vector carries n_ext = -1.
OP_DECODE_ASYNC = 3  # [OP, model_idx, B, nrb, rb_slot*nrb, row*6*B(, tail)]
OP_ROLLBACK = 4      # [OP, model_idx, n, slot*n] — flush before other cmds


def _f2i(x: float) -> int:
    """float32 bit pattern as int (plan-channel encoding)."""
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


def _i2f(x: int) -> float:
    return struct.unpack("<f", struct.pack("<I", int(x) & 0xFFFFFFFF))[0]


@dataclass
class AsyncDecodePlan:
    """One speculative decode step. Per row: KV slot, input token or -1,
    index into the previous step's device sample or -1, effective seed,
    temperature, top_p; ext is None or per-row GenRequest.ext_spec()."""
    slots: List[int]
    feed: List[int]
    prev_idx: List[int]
    seeds: List[int]
    temps: List[float]
    tops: List[float]
    ext: Optional[List[Optional[ExtSpec]]] = None
    rollbacks: List[int] = field(default_factory=list)


def header(cmd: List[int]) -> Tuple[int, int]:
    """(op, model_idx) of a received vector; -1 where it names no model."""
    return cmd[0], cmd[1] if len(cmd) > 1 else -1


def encode_sync(model_idx: int, slots, toks) -> List[int]:
    return [OP_DECODE, model_idx, len(slots), *slots, *toks]


def decode_sync(cmd: List[int]) -> Tuple[List[int], List[int]]:
    B = cmd[2]
    return cmd[3:3 + B], cmd[3 + B:3 + 2 * B]


def encode_rollback(model_idx: int, slots: List[int]) -> List[int]:
    return [OP_ROLLBACK, model_idx, len(slots), *slots]


def decode_rollback(cmd: List[int]) -> List[int]:
    return cmd[3:3 + cmd[2]]


def encode_async(model_idx: int, name: str, p: AsyncDecodePlan) -> List[int]:
    """A plan's vector; an over-long tail is broadcast ahead of it here."""
    vec = [OP_DECODE_ASYNC, model_idx, len(p.slots), len(p.rollbacks),
           *p.rollbacks]
    for i, slot in enumerate(p.slots):
        vec += [slot, p.feed[i], p.prev_idx[i], p.seeds[i],
                _f2i(p.temps[i]), _f2i(p.tops[i])]
    if p.ext is None:
        return vec
    rows = [i for i, sp in enumerate(p.ext) if sp is not None]
    tail = [len(rows)]
    for i in rows:
        sp = ExtSpec(*p.ext[i])  # a plain tuple of its fields will do too
        tail += [i, sp.top_k, _f2i(sp.min_p), _f2i(sp.rep), _f2i(sp.pres),
                 _f2i(sp.freq), _f2i(p.tops[i]), len(sp.edits)]
        for t, c, b in sp.edits:
            tail += [t, c, _f2i(b)]
    if 1 + len(vec) + len(tail) <= par.PLAN_CAP:
        vec += tail
    else:
        par.broadcast_obj(("ext_tail", name, tail))
        vec.append(-1)
    return vec


def decode_async(cmd: List[int], take_tail: Callable) -> AsyncDecodePlan:
    """Inverse of encode_async, floats rounded through float32. take_tail
    hands over the tail an "ext_tail" command stashed (n_ext = -1 only)."""
    B, nrb = cmd[2], cmd[3]
    off = 4 + nrb + 6 * B
    col = [cmd[4 + nrb + k:off:6] for k in range(6)]
    p = AsyncDecodePlan(col[0], col[1], col[2], col[3],
                        [_i2f(x) for x in col[4]], [_i2f(x) for x in col[5]],
                        rollbacks=cmd[4:4 + nrb])
    if off >= len(cmd):
        return p  # no tail: no extended row in this step
    tail = cmd
    if cmd[off] < 0:
        tail, off = take_tail(), 0
    n_ext = tail[off]
    off += 1
    p.ext = [None] * B
    for _ in range(n_ext):
        i, top_k, mp, rep, pres, freq, _tp, n = tail[off:off + 8]
        off += 8
        edits = [(tail[off + 3 * k], tail[off + 3 * k + 1],
                  _i2f(tail[off + 3 * k + 2])) for k in range(n)]
        off += 3 * n
        p.ext[i] = ExtSpec(top_k=top_k, min_p=_i2f(mp), rep=_i2f(rep),
                           pres=_i2f(pres), freq=_i2f(freq), edits=edits)
    return p
