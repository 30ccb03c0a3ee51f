"""Serving with logprobs, sampling penalties and logit_bias (CPU): engine, OpenAI-compatible
server, LiteLLM-compatible client, tensor-parallel engine.

The model is the tiny preset in fp32, so the engine's decode path and a full forward differ only
by summation order and the log-probabilities can be held to the kernel tests' bound
(tests/test_logits_proc.py ``LOGPROB``) against the fp64 log-softmax of the full-forward logits.
"""
import json
import os
import socket
import threading
import time

import pytest
import torch
import torch.multiprocessing as mp

from mxllm.data.tokenizer import ByteTokenizer
from mxllm.models import Llama, get_config
from mxllm.ops import decode as dops
from mxllm.serve import client
from mxllm.serve.engine import Engine, SamplingParams

from ._parity import assert_parity
from .test_logits_proc import LOGPROB

LOOP_PROMPT = [5, 9, 77, 1, 300]  # greedy decoding of the fp32 tiny model (seed 0) falls into a repeat loop
PROMPTS = [LOOP_PROMPT, list(range(3, 40)), [7, 7, 3], [250, 11, 42, 42, 17, 99, 3]]


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    return Llama(get_config("tiny"), dtype=torch.float32, seed=0).eval()


@pytest.fixture(scope="module")
def engine(model):
    return Engine(model, max_batch=4, max_seq=256)


def _run(eng, prompts, params):
    """Submit prompts with one SamplingParams each and step the engine until all are done."""
    reqs = [eng.submit(p, sp) for p, sp in zip(prompts, params)]
    if eng._thread is not None:
        for r in reqs:
            assert r.done.wait(120)
    else:
        while not all(r.done.is_set() for r in reqs):
            eng.step()
    return reqs


def _forward_logprobs(model, prompt, output):
    """fp64 log-softmax of the full-forward logits at every output position, and the row scales."""
    seq, rows = list(prompt), []
    with torch.no_grad():
        for t in output:
            rows.append(model(torch.tensor([seq]))[0, -1].float())
            seq.append(t)
    x = torch.stack(rows)
    return torch.log_softmax(x.double(), -1), x.abs().amax(-1).double(), x


def _assert_logprobs(model, prompt, r, n_top):
    ref, scale, x = _forward_logprobs(model, prompt, r.output)
    assert len(r.logprobs) == len(r.output)
    for i, (tok, (lp, top)) in enumerate(zip(r.output, r.logprobs)):
        assert len(top) == n_top
        assert_parity(torch.tensor([lp]), ref[i, tok].view(1), LOGPROB, scale=float(scale[i]), name=f"logprob[{i}]")
        ids = [t for t, _ in top]
        assert_parity(torch.tensor([v for _, v in top]), ref[i, ids], LOGPROB, scale=float(scale[i]), name=f"top[{i}]")
        assert [v for _, v in top] == sorted((v for _, v in top), reverse=True)
        assert set(ids) == set(x[i].topk(n_top).indices.tolist())


def test_greedy_logprobs_match_full_forward(engine, model):
    r = engine.generate([PROMPTS[1]], max_new_tokens=8, logprobs=5, return_requests=True)[0]
    assert r.output == engine.generate([PROMPTS[1]], max_new_tokens=8)[0]
    _assert_logprobs(model, PROMPTS[1], r, 5)
    for tok, (lp, top) in zip(r.output, r.logprobs):  # greedy: the chosen token heads the list, same bits
        assert top[0] == (tok, lp)


def test_batching_does_not_change_tokens_or_logprobs():
    """bf16 tiny model (the preset's own dtype): its rounded logits do not depend on the rows a
    GEMM runs beside, so the lists are identical, not merely close."""
    engine = Engine(Llama(get_config("tiny"), seed=0).eval(), max_batch=4, max_seq=256)
    sp = SamplingParams(max_new_tokens=7, logprobs=3)
    alone = _run(engine, [PROMPTS[1]], [sp])[0]
    others = [SamplingParams(max_new_tokens=9), SamplingParams(max_new_tokens=5, frequency_penalty=1.5,
                                                               repetition_penalty=1.2, logit_bias={9: -50}),
              SamplingParams(max_new_tokens=7, temperature=0.8, seed=3)]
    batched = _run(engine, [PROMPTS[0], PROMPTS[1], PROMPTS[2], PROMPTS[3]], [others[0], sp, others[1], others[2]])
    assert batched[1].output == alone.output
    assert batched[1].logprobs == alone.logprobs
    # the plain and the temperature neighbours draw what they draw alone, too
    assert batched[0].output == _run(engine, [PROMPTS[0]], [others[0]])[0].output
    assert batched[3].output == _run(engine, [PROMPTS[3]], [others[2]])[0].output


def test_logit_bias_bans_and_forces(engine):
    first = engine.generate([PROMPTS[2]], max_new_tokens=1)[0][0]
    banned = engine.generate([PROMPTS[2]], max_new_tokens=4, logit_bias={first: -100})[0]
    assert banned[0] != first and first not in banned
    forced = engine.generate([PROMPTS[2]], max_new_tokens=6, logit_bias={123: 100})[0]
    assert forced == [123] * 6


def test_frequency_penalty_breaks_a_repeat_loop(engine):
    plain = engine.generate([LOOP_PROMPT], max_new_tokens=12)[0]
    assert len(set(plain)) <= 6, plain  # the pinned prompt loops
    pen = engine.generate([LOOP_PROMPT], max_new_tokens=12, frequency_penalty=2.0)[0]
    assert len(set(pen)) > len(set(plain)), (plain, pen)


def test_repetition_penalty_covers_prompt_only_tokens(engine, monkeypatch):
    """First sampled token (prefill logits): the repetition penalty already sees the prompt."""
    seen = {}
    real = dops.adjust_logits_rows

    def spy(logits, state, slots, *a, **k):
        out = real(logits, state, slots, *a, **k)
        seen.setdefault("first", (logits.float().clone(), out.clone(), state[slots[0]].clone()))
        return out

    monkeypatch.setattr(dops, "adjust_logits_rows", spy)
    prompt = [7, 7, 3, 400]
    engine.generate([prompt], max_new_tokens=2, repetition_penalty=1.5)
    x, y, st = seen["first"]
    r = torch.tensor(1.5)
    for t in (7, 3, 400):  # prompt-only tokens: flagged, count 0, penalised
        assert int(st[t]) == dops.PROMPT_FLAG
        assert y[0, t] == (x[0, t] / r if x[0, t] > 0 else x[0, t] * r) and y[0, t] != x[0, t]
    rest = torch.ones(x.shape[1], dtype=torch.bool)
    rest[[7, 3, 400]] = False
    assert torch.equal(y[0, rest], x[0, rest]) and int((st != 0).sum()) == 3


def test_default_path_allocates_and_calls_nothing(model, monkeypatch):
    eng = Engine(model, max_batch=4, max_seq=256)
    calls = {"adjust": 0, "logprob": 0, "update": 0, "sample": []}
    for name, key in (("adjust_logits_rows", "adjust"), ("logprob_rows", "logprob"), ("token_state_update", "update")):
        real = getattr(dops, name)

        def counted(*a, _real=real, _key=key, **k):
            calls[_key] += 1
            return _real(*a, **k)

        monkeypatch.setattr(dops, name, counted)
    real_sample = dops.sample_rows

    def sample(logits, *a, **k):
        calls["sample"].append(logits.dtype)
        return real_sample(logits, *a, **k)

    monkeypatch.setattr(dops, "sample_rows", sample)
    out = eng.generate(PROMPTS, max_new_tokens=5, temperature=0.7, top_p=0.9, seed=4)
    assert eng._tok_state is None and eng._tok_bias is None
    assert calls["adjust"] == calls["logprob"] == calls["update"] == 0 and len(calls["sample"]) == 5
    # ... and the same tokens as an engine that has served penalised requests before
    eng.generate([PROMPTS[0]], max_new_tokens=3, presence_penalty=1.0, logit_bias={5: 2.0}, logprobs=1)
    assert eng._tok_state is not None and eng._tok_bias is not None and calls["adjust"] == 3
    assert eng.generate(PROMPTS, max_new_tokens=5, temperature=0.7, top_p=0.9, seed=4) == out
    assert calls["adjust"] == 3
    # logprobs alone: no adjusted copy, no counts
    eng.generate([PROMPTS[0]], max_new_tokens=2, logprobs=0)
    assert calls["adjust"] == 3 and calls["update"] == 3 and calls["logprob"] == 5


def test_validation(engine):
    for kw in ({"logprobs": 21}, {"logprobs": -1}, {"presence_penalty": 3}, {"frequency_penalty": -2.5},
               {"repetition_penalty": 0}, {"logit_bias": {5: 101}}, {"logit_bias": {"x": 1}},
               {"logit_bias": {i: 1 for i in range(301)}}):
        with pytest.raises(ValueError):
            SamplingParams(**kw)
    sp = SamplingParams(8, 0.0, 1.0, 0, (), 0, 0.5, -0.5, 1.1, {"17": 3}, 20)  # positional order
    assert sp.logit_bias == {17: 3.0} and sp.logprobs == 20 and sp.repetition_penalty == 1.1
    assert SamplingParams(5, 0.5, 0.9, 3, (1,), 2).logprobs is None
    # an id outside the vocabulary fails that request only
    bad, good = _run(engine, [PROMPTS[2], PROMPTS[2]],
                     [SamplingParams(max_new_tokens=3, logit_bias={512: 1.0}), SamplingParams(max_new_tokens=3)])
    assert bad.finish_reason == "error" and "logit_bias" in bad.error and bad.output == []
    assert good.finish_reason == "length" and len(good.output) == 3
    assert engine.generate([PROMPTS[2]], max_new_tokens=3)[0] == good.output


def test_score_matches_cross_entropy(engine, model):
    ids = PROMPTS[1]
    with torch.no_grad():
        logits = model(torch.tensor([ids]))[0].float()
    ref = torch.log_softmax(logits.double(), -1)
    want = ref[torch.arange(len(ids) - 1), torch.tensor(ids[1:])]

    def check(entries):
        assert entries[0] is None and len(entries) == len(ids)
        lp = torch.tensor([e[0] for e in entries[1:]])
        for i in range(len(lp)):
            assert_parity(lp[i:i + 1], want[i:i + 1], LOGPROB, scale=float(logits[i].abs().max()), name=f"score[{i}]")
        assert all(len(e[1]) == 2 and e[1][0][0] == int(logits[i].argmax()) for i, e in enumerate(entries[1:]))

    got = engine.score([ids, [4, 2]], top=2)
    assert len(got[1]) == 2 and engine.score([[9]]) == [[None]]
    check(got[0])
    engine.SCORE_ROWS = 5  # several chunks (an fp32 GEMM's sums depend on its row count: bound, not bits)
    try:
        check(engine.score([ids], top=2)[0])
    finally:
        del engine.SCORE_ROWS


# --------------------------------------------------------------------------- HTTP
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.fixture(scope="module")
def server(model):
    import uvicorn

    from mxllm.serve.server import build_app

    eng = Engine(model, max_batch=4, max_seq=256)
    port = _free_port()
    app = build_app(eng, ByteTokenizer(512), "tiny-lp")
    srv = uvicorn.Server(uvicorn.Config(app, host="127.0.0.1", port=port, log_level="error"))
    th = threading.Thread(target=srv.run, daemon=True)
    th.start()
    for _ in range(200):
        if srv.started:
            break
        time.sleep(0.05)
    client.register_local("tiny-lp", eng, ByteTokenizer(512))
    yield f"http://127.0.0.1:{port}/v1"
    client.unregister_local("tiny-lp")
    srv.should_exit = True
    th.join(10)
    eng.stop()


MSG = [{"role": "user", "content": "hello"}]


def _post(server, route, body):
    import httpx

    return httpx.post(server + route, json=body, timeout=60)


def test_http_chat_logprobs_shape(server):
    j = _post(server, "/chat/completions", {"messages": MSG, "max_tokens": 5, "logprobs": True,
                                            "top_logprobs": 3}).json()
    content = j["choices"][0]["logprobs"]["content"]
    assert len(content) == j["usage"]["completion_tokens"] == 5
    for e in content:
        assert set(e) == {"token", "logprob", "bytes", "top_logprobs"} and e["logprob"] <= 0
        assert e["bytes"] == list(e["token"].encode("utf-8")) and len(e["top_logprobs"]) == 3
        assert all(set(t) == {"token", "logprob", "bytes"} for t in e["top_logprobs"])
        assert e["top_logprobs"][0]["logprob"] == e["logprob"]  # greedy
    plain = _post(server, "/chat/completions", {"messages": MSG, "max_tokens": 5}).json()
    assert "logprobs" not in plain["choices"][0]
    assert plain["choices"][0]["message"]["content"] == j["choices"][0]["message"]["content"]


def test_http_completions_logprobs_shape(server):
    j = _post(server, "/completions", {"prompt": "abc", "max_tokens": 4, "logprobs": 2}).json()
    lp = j["choices"][0]["logprobs"]
    assert set(lp) == {"tokens", "token_logprobs", "top_logprobs", "text_offset"}
    assert len(lp["tokens"]) == len(lp["token_logprobs"]) == len(lp["top_logprobs"]) == len(lp["text_offset"]) == 4
    assert all(isinstance(d, dict) and 1 <= len(d) <= 2 for d in lp["top_logprobs"])
    assert lp["text_offset"][0] == 0 and all(v <= 0 for v in lp["token_logprobs"])


def test_http_stream_chunks_carry_logprobs(server):
    import httpx

    body = {"messages": MSG, "max_tokens": 6, "logprobs": True, "top_logprobs": 2}
    whole = _post(server, "/chat/completions", body).json()["choices"][0]["logprobs"]["content"]
    got = []
    with httpx.stream("POST", server + "/chat/completions", json=dict(body, stream=True), timeout=60) as s:
        for line in s.iter_lines():
            if line.startswith("data: ") and line[6:].strip() != "[DONE]":
                ch = json.loads(line[6:])["choices"][0]
                if ch.get("logprobs"):
                    got += ch["logprobs"]["content"]
    assert got == whole


def test_http_echo_scores_the_prompt(server, model):
    tok = ByteTokenizer(512)
    prompt = "score this prompt"
    j = _post(server, "/completions", {"prompt": prompt, "max_tokens": 0, "echo": True, "logprobs": 1}).json()
    ch = j["choices"][0]
    ids = tok.encode(prompt)
    assert ch["text"] == prompt and j["usage"]["completion_tokens"] == 0
    lp = ch["logprobs"]
    assert len(lp["tokens"]) == len(ids) and lp["token_logprobs"][0] is None and lp["top_logprobs"][0] is None
    with torch.no_grad():
        logits = model(torch.tensor([ids]))[0].float()
    ce = torch.nn.functional.cross_entropy(logits[:-1].double(), torch.tensor(ids[1:]), reduction="none")
    got = torch.tensor(lp["token_logprobs"][1:], dtype=torch.float32)
    for i in range(len(got)):
        assert_parity(got[i:i + 1], -ce[i:i + 1], LOGPROB, scale=float(logits[i].abs().max()), name=f"prompt[{i}]")
    # echo with generation: the prompt's entries come first
    j2 = _post(server, "/completions", {"prompt": prompt, "max_tokens": 3, "echo": True, "logprobs": 1}).json()
    lp2 = j2["choices"][0]["logprobs"]
    assert j2["choices"][0]["text"].startswith(prompt) and len(lp2["tokens"]) == len(ids) + 3
    assert lp2["token_logprobs"][:len(ids)] == lp["token_logprobs"]


def test_http_bad_values_are_400(server):
    for route, extra in (("/chat/completions", {"logprobs": True, "top_logprobs": 21}),
                         ("/chat/completions", {"presence_penalty": 3}),
                         ("/chat/completions", {"logit_bias": {"abc": 1}}),
                         ("/chat/completions", {"logit_bias": {"100000": 1}}),
                         ("/completions", {"logprobs": 25}),
                         ("/completions", {"repetition_penalty": 0}),
                         ("/completions", {"frequency_penalty": "much"})):
        body = dict({"messages": MSG, "prompt": "abc", "max_tokens": 2}, **extra)
        r = _post(server, route, body)
        assert r.status_code == 400, (route, extra, r.status_code, r.text)
        assert r.json()["error"]["type"] == "invalid_request_error"
    assert _post(server, "/chat/completions", {"messages": MSG, "max_tokens": 2}).status_code == 200


def test_http_penalties_and_bias_reach_the_engine(server):
    base = {"prompt": "aaaa", "max_tokens": 8}
    plain = _post(server, "/completions", base).json()["choices"][0]["text"]
    forced = _post(server, "/completions", dict(base, logit_bias={"66": 100})).json()["choices"][0]["text"]
    assert forced == ByteTokenizer(512).decode([66] * 8) == "B" * 8 and forced != plain
    pen = _post(server, "/completions", dict(base, frequency_penalty=2.0, repetition_penalty=1.3)).json()
    assert pen["choices"][0]["text"] != plain


@pytest.mark.parametrize("route", ["http", "local"])
def test_client_fills_logprobs(server, route):
    base = server if route == "http" else "local"
    r = client.completion("tiny-lp", MSG, api_base=base, max_tokens=4, timeout=60, logprobs=True, top_logprobs=2)
    content = r.choices[0].logprobs["content"]
    assert len(content) == 4 and all(len(e["top_logprobs"]) == 2 for e in content)
    assert client.completion("tiny-lp", MSG, api_base=base, max_tokens=4, timeout=60).choices[0].logprobs is None
    t = client.text_completion("tiny-lp", "abc", api_base=base, max_tokens=3, timeout=60, logprobs=1)
    lp = t.choices[0].logprobs
    assert len(lp["tokens"]) == 3 and len(lp["token_logprobs"]) == 3 and all(len(d) == 1 for d in lp["top_logprobs"])
    chunks = list(client.completion("tiny-lp", MSG, api_base=base, max_tokens=4, timeout=60, stream=True,
                                    logprobs=True, top_logprobs=2, frequency_penalty=0.5))
    got = [e for c in chunks if c.choices[0].logprobs for e in c.choices[0].logprobs["content"]]
    assert len(got) == 4


def test_client_routes_agree(server):
    kw = dict(max_tokens=5, timeout=60, logprobs=True, top_logprobs=2, logit_bias={"70": 4.0}, presence_penalty=0.5)
    a = client.completion("tiny-lp", MSG, api_base=server, **kw)
    b = client.completion("tiny-lp", MSG, api_base="local", **kw)
    assert a.choices[0].message.content == b.choices[0].message.content
    assert a.choices[0].logprobs == b.choices[0].logprobs


# --------------------------------------------------------------------------- tensor parallel
def _tp_model():
    cfg = get_config("tiny").replace(n_layers=2, vocab_size=301, n_heads=8, n_kv_heads=4, ffn=256)
    return Llama(cfg, dtype=torch.float32, seed=5).eval()


TP_PROMPTS = [[1, 5, 9, 13, 200], [7, 7, 3]]


def _tp_params():
    return [SamplingParams(max_new_tokens=8, frequency_penalty=1.5, logprobs=2), SamplingParams(max_new_tokens=6)]


def _tp_worker(rank, world, port, out_q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), MXLLM_FORCE_CPU="1")
    torch.set_num_threads(1)
    import torch.distributed as dist

    from mxllm.parallel import runtime
    from mxllm.parallel.tensor import shard_llama

    runtime.init(rank=rank, world_size=world)
    local = shard_llama(_tp_model(), rank, world)
    eng = Engine(local, max_batch=4, max_seq=64, tp_group=dist.group.WORLD)
    reqs = _run(eng, TP_PROMPTS, _tp_params())
    if rank == 0:
        out_q.put(([r.output for r in reqs], [r.logprobs for r in reqs]))
    runtime.cleanup()


def test_tp_engine_with_penalties_matches_single_process():
    ref = _run(Engine(_tp_model(), max_batch=4, max_seq=64), TP_PROMPTS, _tp_params())
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_tp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    outs, lps = q.get(timeout=240)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert outs == [r.output for r in ref]
    assert len(lps[0]) == 8 and lps[1] == []
    for (a, ta), (b, tb) in zip(lps[0], ref[0].logprobs):
        assert abs(a - b) < 1e-4 and [i for i, _ in ta] == [i for i, _ in tb]
