"""The TP plan channel's int-vector format (engine/plan.py), as a format:
the bytes on the wire are pinned by literals, and every op decodes to what
was encoded. No engine, no process group."""

import struct

import pytest

from agentainer_amd import parallel as par
from agentainer_amd.engine import llm, plan
from agentainer_amd.engine.plan import AsyncDecodePlan


def f32(x):
    return struct.unpack("<f", struct.pack("<f", x))[0]


def rounded(p):
    """The plan as a worker sees it: floats through float32."""
    ext = p.ext and [None if sp is None else
                     (sp[0], *(f32(v) for v in sp[1:5]),
                      [(t, c, f32(b)) for t, c, b in sp[5]]) for sp in p.ext]
    return AsyncDecodePlan(p.slots, p.feed, p.prev_idx, p.seeds,
                           [f32(t) for t in p.temps], [f32(t) for t in p.tops],
                           ext, p.rollbacks)


def no_tail():
    raise AssertionError("no tail was sent ahead")


TWO_ROWS = AsyncDecodePlan(slots=[3, 4], feed=[17, -1], prev_idx=[-1, 0],
                           seeds=[9, 124], temps=[0.0, 0.7], tops=[1.0, 0.9],
                           rollbacks=[5])
TWO_ROWS_VEC = [3, 2, 2, 1, 5, 3, 17, -1, 9, 0, 1065353216,
                4, -1, 0, 124, 1060320051, 1063675494]

EXT = [None, (40, 0.05, 1.3, -0.5, 0.25, [(0, 1, 0.0), (7, 5, -100.0)])]


def test_llm_still_exports_the_wire_names():
    assert (llm.OP_DECODE, llm.OP_BARRIER, llm.OP_DECODE_ASYNC,
            llm.OP_ROLLBACK) == (1, 2, 3, 4)
    assert llm.par is par


def test_async_vector_literal():
    assert plan.encode_async(2, "m", TWO_ROWS) == TWO_ROWS_VEC
    assert plan.header(TWO_ROWS_VEC) == (plan.OP_DECODE_ASYNC, 2)
    assert plan.decode_async(TWO_ROWS_VEC, no_tail) == rounded(TWO_ROWS)


def test_sync_vector_literal():
    vec = plan.encode_sync(2, [3, 4], [17, 99])
    assert vec == [1, 2, 2, 3, 4, 17, 99]
    assert plan.header(vec) == (plan.OP_DECODE, 2)
    assert plan.decode_sync(vec) == ([3, 4], [17, 99])


@pytest.mark.parametrize("rb", [[], [5], [7, 2, 9]])
def test_rollback_round_trip(rb):
    vec = plan.encode_rollback(1, rb)
    assert vec == [4, 1, len(rb)] + rb
    assert plan.header(vec) == (plan.OP_ROLLBACK, 1)
    assert plan.decode_rollback(vec) == rb


def test_barrier_addresses_no_model():
    assert plan.header([plan.OP_BARRIER]) == (plan.OP_BARRIER, -1)


@pytest.mark.parametrize("ext", [None, EXT, [None, None]])
@pytest.mark.parametrize("rb", [[], [5, 6]])
def test_async_round_trip(ext, rb):
    p = AsyncDecodePlan(TWO_ROWS.slots, TWO_ROWS.feed, TWO_ROWS.prev_idx,
                        TWO_ROWS.seeds, TWO_ROWS.temps, TWO_ROWS.tops,
                        ext, rb)
    vec = plan.encode_async(0, "m", p)
    base = 4 + len(rb) + 6 * 2
    if ext is None:
        assert len(vec) == base  # without a tail the vector is unchanged
    else:
        assert vec[base] == sum(sp is not None for sp in ext)
    assert plan.decode_async(vec, no_tail) == rounded(p)


def test_async_smallest_shapes():
    p = AsyncDecodePlan([0], [1], [-1], [0], [0.0], [1.0])
    vec = plan.encode_async(0, "m", p)
    assert vec == [3, 0, 1, 0, 0, 1, -1, 0, 0, 1065353216]
    assert plan.decode_async(vec, no_tail) == p
    assert plan.decode_sync(plan.encode_sync(0, [6], [2])) == ([6], [2])


def test_async_overflow_tail_travels_ahead(monkeypatch):
    sent = []
    monkeypatch.setattr(par, "broadcast_obj", sent.append)
    big = [(1, 0.0, 1.1, 0.0, 0.0, [(t, 1, 0.0) for t in range(9000)])]
    p = AsyncDecodePlan([0], [1], [-1], [0], [0.0], [1.0], big)
    vec = plan.encode_async(0, "m", p)
    assert vec[-1] == -1 and len(vec) == 11
    assert len(sent) == 1 and sent[0][:2] == ("ext_tail", "m")
    assert 1 + 10 + len(sent[0][2]) > par.PLAN_CAP  # it did not fit
    stash = [sent[0][2]]
    assert plan.decode_async(vec, stash.pop) == rounded(p)
    assert not stash  # taken exactly once
