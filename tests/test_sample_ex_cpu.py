"""Extended sampler — the CPU reference (ops.reference.sample_ex, the
definition the gfx950 kernel follows) and the request routing."""

import pytest
import torch

from agentainer_amd import ops
from agentainer_amd.engine.llm import (GenRequest, ModelInstance,
                                       parse_sampling_controls)
from agentainer_amd.ops import reference

V = 16


def _row(vals):
    return torch.tensor([vals], dtype=torch.float32).to(torch.bfloat16)


def _sample(logits, temp=0.0, top_p=1.0, seed=0, top_k=0, min_p=0.0, rep=1.0,
            pres=0.0, freq=0.0, edits=(), pending=None, want_ws=False):
    B, Vv = logits.shape
    out = torch.empty(B, dtype=torch.long)
    ws = torch.zeros(B * Vv, dtype=torch.float32)
    pend = None if pending is None else torch.tensor([pending] * B)
    ops.sample_ex(out, logits, [temp] * B, [top_p] * B, [seed] * B,
                  [top_k] * B, [min_p] * B, [rep] * B, [pres] * B, [freq] * B,
                  [list(edits)] * B, pending=pend, ws=ws)
    return (out, ws.view(B, Vv)) if want_ws else out


# logits exactly representable in bf16
BASE = [2.0, -1.0, 0.5, 4.0, -3.0, 1.0, 0.0, 3.0,
        -0.5, 2.5, 1.5, -2.0, 0.25, 3.5, -4.0, 0.75]


def test_repetition_penalty_alone_is_sign_dependent():
    # token 3 (l=4 > 0) seen in the prompt, token 4 (l=-3 < 0) generated
    # once, token 7 carries a zero bias and is not seen: rep=2 divides the
    # positive logit and multiplies the negative one
    _, ws = _sample(_row(BASE), rep=2.0,
                    edits=[(3, 1, 0.0), (4, 2, 0.0), (7, 0, 0.0)], want_ws=True)
    want = list(BASE)
    want[3] = 2.0
    want[4] = -6.0
    assert ws[0].tolist() == want


def test_frequency_penalty_alone():
    # token 3 generated 3 times and in the prompt (cnt = 2*3+1), token 0
    # only in the prompt (c = 0: untouched)
    out, ws = _sample(_row(BASE), freq=0.5, edits=[(0, 1, 0.0), (3, 7, 0.0)],
                      want_ws=True)
    want = list(BASE)
    want[3] = 4.0 - 1.5
    assert ws[0].tolist() == want
    assert int(out[0]) == 13  # 3.5 now beats 2.5


def test_presence_penalty_alone():
    out, ws = _sample(_row(BASE), pres=1.0, edits=[(0, 1, 0.0), (3, 6, 0.0)],
                      want_ws=True)
    want = list(BASE)
    want[3] = 3.0  # once, however often it was generated
    assert ws[0].tolist() == want
    assert int(out[0]) == 13


def test_all_penalties_and_bias_in_order():
    # token 3: seen, c=2, bias +0.25: (4/2) - (0.5*2 + 1) + 0.25 = 0.25
    # token 4: in the prompt only, bias -1: (-3*2) - 0 - 1 = -7
    # token 6: bias only (not seen): 0 + 2 = 2
    _, ws = _sample(_row(BASE), rep=2.0, pres=1.0, freq=0.5,
                    edits=[(3, 4, 0.25), (4, 1, -1.0), (6, 0, 2.0)],
                    want_ws=True)
    want = list(BASE)
    want[3], want[4], want[6] = 0.25, -7.0, 2.0
    assert ws[0].tolist() == want


def test_top_k_1_is_argmax_of_edited_logits():
    for seed in range(20):
        out = _sample(_row(BASE), temp=1.0, seed=seed, top_k=1, freq=1.0,
                      edits=[(3, 4, 0.0)])  # 4 - 2 = 2: token 13 leads
        assert int(out[0]) == 13


def test_bias_bans_and_forces():
    for seed in range(50):
        out = _sample(_row(BASE), temp=1.0, seed=seed, edits=[(3, 0, -100.0)])
        assert int(out[0]) != 3
        out = _sample(_row(BASE), temp=1.0, seed=seed, edits=[(14, 0, 100.0)])
        assert int(out[0]) == 14
    assert int(_sample(_row(BASE), edits=[(3, 0, -100.0)])[0]) == 13
    assert int(_sample(_row(BASE), edits=[(14, 0, 100.0)])[0]) == 14


def test_all_equal_row_top_k_4_yields_lowest_ids():
    logits = torch.full((1, 64), 1.5, dtype=torch.bfloat16)
    seen = set()
    for seed in range(200):
        seen.add(int(_sample(logits, temp=1.0, seed=seed, top_k=4)[0]))
    assert seen == {0, 1, 2, 3}


@pytest.mark.parametrize("temp", [0.0, 1.0])
def test_pending_token_equals_folded_count(temp):
    kw = dict(temp=temp, seed=7, rep=1.5, pres=0.5, freq=0.25, top_k=3)
    base = [(3, 3, 0.0), (13, 1, 0.5)]
    # pending inside the CSR: its count goes up by one occurrence
    a = _sample(_row(BASE), edits=base, pending=3, want_ws=True, **kw)
    b = _sample(_row(BASE), edits=[(3, 5, 0.0), (13, 1, 0.5)], want_ws=True, **kw)
    assert torch.equal(a[1], b[1]) and torch.equal(a[0], b[0])
    # pending outside the CSR: a fresh (seen, c=1, bias=0) edit
    a = _sample(_row(BASE), edits=base, pending=7, want_ws=True, **kw)
    b = _sample(_row(BASE), edits=base + [(7, 2, 0.0)], want_ws=True, **kw)
    assert torch.equal(a[1], b[1]) and torch.equal(a[0], b[0])
    assert a[1][0, 7].item() == 3.0 / 1.5 - 0.75
    # -1: none
    a = _sample(_row(BASE), edits=base, pending=-1, want_ws=True, **kw)
    b = _sample(_row(BASE), edits=base, want_ws=True, **kw)
    assert torch.equal(a[1], b[1]) and torch.equal(a[0], b[0])


def test_top_p_1_keeps_n0():
    edited = torch.tensor(BASE)
    ids, cum = reference.sample_ex_kept(edited, 1.0, 1.0, 0.0, 5)
    assert ids.tolist() == [3, 13, 7, 9, 0] and cum.numel() == 5
    ids, _ = reference.sample_ex_kept(edited, 1.0, 1.0, 0.0, 0)
    assert ids.numel() == V  # n0 = min(CAP, V)
    # and the cuts: min_p = e^-1.25 keeps p >= that fraction of p_max
    ids, _ = reference.sample_ex_kept(edited, 1.0, 1.0, 0.3, 0)
    assert ids.tolist() == [3, 13, 7]
    ids, _ = reference.sample_ex_kept(edited, 1.0, 0.5, 0.0, 0)
    p = torch.softmax(edited.double(), 0)
    assert ids.tolist() == [3, 13] and p[3] < 0.5 <= p[3] + p[13]


def test_uniform01_port_known_values():
    # values of the kernel hash worked out by hand in 64-bit arithmetic
    def by_hand(seed, row):
        m = (1 << 64) - 1
        x = (seed ^ (0x9E3779B97F4A7C15 * (row + 1))) & m
        x ^= x >> 12
        x = (x ^ (x << 25)) & m
        x ^= x >> 27
        x = (x * 0x2545F4914F6CDD1D) & m
        return ((x >> 40) & 0xFFFFFF) / 2.0 ** 24
    for seed, row in [(0, 0), (123, 5), ((1 << 63) - 1, 255)]:
        u = reference.uniform01(seed, row)
        assert u == by_hand(seed, row) and 0.0 <= u < 1.0
    assert reference.uniform01(1, 0) != reference.uniform01(1, 1)


def test_draw_follows_the_inverse_cdf():
    logits = _row(BASE)
    ids, cum = reference.sample_ex_kept(torch.tensor(BASE), 1.0, 0.9, 0.0, 8)
    cdf = (cum / cum[-1]).tolist()
    for seed in range(64):
        j = ids.tolist().index(int(_sample(logits, temp=1.0, top_p=0.9,
                                           seed=seed, top_k=8)[0]))
        u = reference.uniform01(seed, 0)
        assert (cdf[j - 1] if j else 0.0) <= u <= cdf[j]


# ------------------------------ routing ------------------------------------

def _req(**kw):
    return GenRequest(agent_id="a", prompt_tokens=[1, 2, 2, 5], max_new=4,
                      temperature=kw.pop("temperature", 0.0), top_p=1.0,
                      seed=0, **kw)


def test_all_off_request_is_not_extended_and_skips_sample_ex(monkeypatch):
    calls = []
    real = ops.sample_ex
    monkeypatch.setattr(ops, "sample_ex",
                        lambda *a, **k: calls.append(1) or real(*a, **k))
    off = parse_sampling_controls({"temperature": 0.7, "top_p": 0.9}, 512)
    assert off == dict(top_k=0, min_p=0.0, repetition_penalty=1.0,
                       presence_penalty=0.0, frequency_penalty=0.0,
                       logit_bias={})
    plain, seeded = _req(**off), _req(temperature=0.7, **off)
    assert not plain.extended and plain.ext_spec() is None
    logits = torch.randn(2, 512, generator=torch.Generator().manual_seed(0))
    logits = logits.to(torch.bfloat16)
    inst = ModelInstance.__new__(ModelInstance)  # the samplers hold no state
    got = inst._sample_device(logits, [plain, seeded])
    assert not calls
    want = inst._sample_device_params(logits, [0.0, 0.7], [1.0, 1.0], [0, 0])
    assert torch.equal(got, want)  # today's greedy/top-p path, untouched
    ext = _req(top_k=5, temperature=0.7)
    assert ext.extended
    inst._sample_device(logits, [plain, ext])
    assert calls == [1]


def test_request_state_tracks_prompt_set_and_counts():
    r = _req(repetition_penalty=1.2, logit_bias={9: 1.0})
    assert r.prompt_set == {1, 2, 5}
    for t in (7, 2, 7):
        r.add_token(t)
    assert r.generated == [7, 2, 7] and r.gen_counts == {7: 2, 2: 1}
    assert r.ext_spec()[5] == [(1, 1, 0.0), (2, 3, 0.0), (5, 1, 0.0),
                               (7, 4, 0.0), (9, 0, 1.0)]
    # without a repetition penalty prompt-only tokens cannot change
    r = _req(frequency_penalty=0.5)
    r.add_token(2)
    assert r.ext_spec()[5] == [(2, 3, 0.0)]


@pytest.mark.parametrize("sampling", [
    {"top_k": -1}, {"top_k": 5000}, {"top_k": 1.5}, {"top_k": "4"},
    {"logit_bias": {"512": 1.0}}, {"logit_bias": {"-1": 1.0}},
    {"logit_bias": {str(i): 0.5 for i in range(301)}},
    {"logit_bias": {"3": 101}}, {"logit_bias": [3]},
    {"repetition_penalty": 0}, {"repetition_penalty": -1.0},
    {"min_p": 1.5}, {"min_p": "x"}, {"presence_penalty": 2.5},
    {"frequency_penalty": -2.5}, {"frequency_penalty": float("nan")},
])
def test_invalid_values_raise(sampling):
    with pytest.raises(ValueError):
        parse_sampling_controls(sampling, 512)


def test_valid_values_parse():
    got = parse_sampling_controls(
        {"top_k": 1024, "min_p": 1, "repetition_penalty": 1.3,
         "presence_penalty": -2, "frequency_penalty": 2,
         "logit_bias": {"511": -100, 0: 100.0}}, 512)
    assert got["top_k"] == 1024 and got["logit_bias"] == {511: -100.0, 0: 100.0}
    assert len(parse_sampling_controls(
        {"logit_bias": {i: 0.0 for i in range(300)}}, 512)["logit_bias"]) == 300


def test_cli_invoke_forwards_sampling(monkeypatch):
    from click.testing import CliRunner

    from agentainer_amd import cli as cli_mod

    sent = []

    def call(self, method, path, body=None, **kw):
        sent.append((method, path, body))
        return {"data": {"response": "ok"}}

    monkeypatch.setattr(cli_mod.Client, "call", call)
    runner = CliRunner()
    res = runner.invoke(cli_mod.cli, [
        "invoke", "agent-1", "-m", "hi", "--sampling",
        '{"top_k": 40, "logit_bias": {"65": -100}}'])
    assert res.exit_code == 0, res.output
    assert sent[0][2]["body"] == {
        "message": "hi",
        "sampling": {"top_k": 40, "logit_bias": {"65": -100}}}
    res = runner.invoke(cli_mod.cli, ["invoke", "agent-1", "-m", "hi"])
    assert sent[1][2]["body"] == {"message": "hi"}  # as before the option
    for bad in ("{not json", "[1, 2]"):
        res = runner.invoke(cli_mod.cli, ["invoke", "agent-1", "-m", "hi",
                                          "--sampling", bad])
        assert res.exit_code == 2 and len(sent) == 2
