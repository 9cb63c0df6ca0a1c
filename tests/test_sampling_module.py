"""engine.sampling: the row grouping around the three sampler kernels, the
effective-seed rule and the logprobs record, against the ops functions
called directly (ops.reference through the normal dispatch on the CPU)."""

import pytest
import torch

from agentainer_amd import ops
from agentainer_amd.engine import sampling
from agentainer_amd.engine.request import ExtSpec, GenRequest

B = 5
EXT_ROWS, GREEDY_ROWS, TOPP_ROWS = [0, 4], [1, 3], [2]


def _req(**kw):
    return GenRequest(agent_id="a", prompt_tokens=[1, 2, 2, 5], max_new=8,
                      temperature=kw.pop("temperature", 0.0),
                      top_p=kw.pop("top_p", 1.0), seed=kw.pop("seed", 0), **kw)


def _mixed():
    """(extended, greedy, top-p, greedy, extended); the last one greedy."""
    return [_req(temperature=0.8, top_p=0.9, seed=11, top_k=8,
                 repetition_penalty=1.3),
            _req(),
            _req(temperature=0.7, top_p=0.9, seed=5),
            _req(),
            _req(top_k=4, logit_bias={7: 5.0})]


def _logits(rows, V, device="cpu"):
    g = torch.Generator().manual_seed(3)
    return (torch.randn(rows, V, generator=g) * 2.5).to(torch.bfloat16).to(device)


def _direct(logits, temps, tops, seeds, ext):
    """The three ops calls on rows gathered in ascending order."""
    dev = logits.device
    lb = logits.to(torch.bfloat16).contiguous()
    out = torch.empty(B, dtype=torch.long, device=dev)

    def pick(vals, rows):
        return [vals[i] for i in rows]

    sub = torch.empty(len(EXT_ROWS), dtype=torch.long, device=dev)
    sp = pick(ext, EXT_ROWS)
    ops.sample_ex(sub, lb[EXT_ROWS].contiguous(), pick(temps, EXT_ROWS),
                  pick(tops, EXT_ROWS), pick(seeds, EXT_ROWS),
                  [s[0] for s in sp], [s[1] for s in sp], [s[2] for s in sp],
                  [s[3] for s in sp], [s[4] for s in sp], [s[5] for s in sp])
    out[EXT_ROWS] = sub
    sub = torch.empty(len(GREEDY_ROWS), dtype=torch.long, device=dev)
    ops.greedy_sample(sub, lb[GREEDY_ROWS].contiguous())
    out[GREEDY_ROWS] = sub
    sub = torch.empty(len(TOPP_ROWS), dtype=torch.long, device=dev)
    ops.topp_sample(
        sub, lb[TOPP_ROWS].contiguous(),
        torch.tensor(pick(temps, TOPP_ROWS), dtype=torch.float32, device=dev),
        torch.tensor(pick(tops, TOPP_ROWS), dtype=torch.float32, device=dev),
        torch.tensor(pick(seeds, TOPP_ROWS), dtype=torch.int64, device=dev))
    out[TOPP_ROWS] = sub
    return out


@pytest.fixture
def recorder(monkeypatch):
    """Every sampler call as (name, args, kwargs), the call still made."""
    calls = []
    for name in ("sample_ex", "greedy_sample", "topp_sample"):
        def wrapped(*a, _name=name, _real=getattr(ops, name), **k):
            calls.append((_name, a, k))
            return _real(*a, **k)
        monkeypatch.setattr(ops, name, wrapped)
    return calls


def test_grouping_equals_the_direct_calls(recorder):
    logits = _logits(B, 512)
    rows = sampling.request_rows(_mixed())
    assert [sp is not None for sp in rows[3]] == [True, False, False, False,
                                                  True]
    got = sampling.sample(logits, *rows)
    assert [c[0] for c in recorder] == ["sample_ex", "greedy_sample",
                                        "topp_sample"]
    # a kernel sees only its group's rows, in ascending row order
    for (_n, a, _k), want in zip(recorder, (EXT_ROWS, GREEDY_ROWS, TOPP_ROWS)):
        assert torch.equal(a[1], logits[want])
    del recorder[:]
    assert torch.equal(got, _direct(logits, *rows))


@pytest.mark.parametrize("temp,name", [(0.0, "greedy_sample"),
                                       (0.7, "topp_sample")])
def test_whole_batch_is_sampled_in_place(recorder, temp, name):
    logits = _logits(B, 512)
    reqs = [_req(temperature=temp, top_p=0.9, seed=i) for i in range(B)]
    temps, tops, seeds, ext = sampling.request_rows(reqs)
    assert ext is None
    got = sampling.sample(logits, temps, tops, seeds)
    (n, a, _k), = recorder
    assert n == name
    # the converted logits tensor itself, and the result tensor: no gather
    assert a[1].data_ptr() == logits.data_ptr() and a[1].shape == logits.shape
    assert a[0].data_ptr() == got.data_ptr()


def test_pending_is_cut_to_a_strict_subset_only(recorder):
    logits = _logits(B, 512)
    pending = torch.tensor([10, 20, -1, 30, 40], dtype=torch.int64)
    sampling.sample(logits, *sampling.request_rows(_mixed()), pending=pending)
    assert recorder[0][0] == "sample_ex"
    assert recorder[0][2]["pending"].tolist() == [10, 40]
    del recorder[:]
    reqs = [_req(top_k=4, seed=i) for i in range(B)]
    sampling.sample(logits, *sampling.request_rows(reqs), pending=pending)
    (n, a, k), = recorder
    assert n == "sample_ex" and k["pending"] is pending
    assert a[1].data_ptr() == logits.data_ptr()


def test_request_rows_states_the_seed_rule():
    fresh, carried, wraps = _req(seed=100), _req(seed=100), _req(seed=2**63 - 1)
    for r in (fresh, carried):
        r.add_token(3)
        r.add_token(4)
    wraps.add_token(3)
    temps, tops, seeds, ext = sampling.request_rows(
        [fresh, carried, wraps], carried=[False, True, False])
    assert seeds == [102, 103, 0]  # (2**63 - 1 + 1) masked to 63 bits
    assert temps == [0.0] * 3 and tops == [1.0] * 3
    assert ext is None
    assert sampling.request_rows([fresh, carried])[2] == [102, 102]
    ext = sampling.request_rows([fresh, _req(top_k=3)])[3]
    assert ext == [None, (3, 0.0, 1.0, 0.0, 0.0, [])]
    assert isinstance(ext[1], ExtSpec) and ext[1].top_k == 3


def test_launch_logprobs_without_a_requesting_row(monkeypatch):
    calls = []
    monkeypatch.setattr(ops, "token_logprobs",
                        lambda *a, **k: calls.append(1))
    logits = _logits(2, 512)
    sampled = torch.zeros(2, dtype=torch.long)
    assert sampling.launch_logprobs(logits, [_req(), _req()], sampled) is None
    assert not calls


def test_fetch_cuts_each_row_to_its_own_count():
    logits = _logits(4, 512)
    reqs = [_req(logprobs=True, top_logprobs=0), _req(),
            _req(logprobs=True, top_logprobs=3),
            _req(logprobs=True, top_logprobs=20)]
    sampled = torch.tensor([5, 6, 7, 8], dtype=torch.long)
    lp = sampling.launch_logprobs(logits, reqs, sampled)
    assert lp.rows == [0, 2, 3] and lp.tops == [0, 3, 20]
    assert lp.top_id.shape == (3, 20)
    got = lp.fetch()
    assert sorted(got) == [0, 2, 3]
    want = torch.log_softmax(logits.double(), -1)
    for i, n in zip(lp.rows, lp.tops):
        chosen, top = got[i]
        assert chosen == pytest.approx(want[i, int(sampled[i])].item(), abs=1e-5)
        order = torch.sort(logits[i].double(), descending=True, stable=True)
        assert [t for t, _p in top] == order.indices[:n].tolist()
    # fewer tokens than the count asked for: the -1 padding is dropped
    small = _logits(1, 8)
    lp = sampling.launch_logprobs(small, [_req(logprobs=True, top_logprobs=20)],
                                  torch.zeros(1, dtype=torch.long))
    assert (lp.top_id < 0).sum().item() == 12
    (_chosen, top), = lp.fetch().values()
    assert sorted(t for t, _p in top) == list(range(8))


@pytest.mark.gpu
def test_grouping_on_the_device():
    """The grouping test on the GPU kernels, the logits handed in as the
    graph's logits buffer arrives: the first rows of a larger bucket."""
    buf = _logits(8, 4104, "cuda")
    logits = buf[:B]
    rows = sampling.request_rows(_mixed())
    got = sampling.sample(logits, *rows)
    assert torch.equal(got, _direct(logits, *rows))
    assert torch.equal(buf, _logits(8, 4104, "cuda"))  # read only
