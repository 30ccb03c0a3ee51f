"""Speculative decoding on the CPU reference path (``tiny`` and ``tiny-d128``, fp32): the prompt-lookup
drafter (mxllm/serve/speculate.py), the accept op (``mxllm.ops.decode.spec_accept``), the verify attention's
CPU expression, and ``Engine(speculate=K, drafter=...)``.

The drafts are deterministic, so acceptance is "the draw equals the draft" and the speculative engine must
emit the plain engine's token stream, greedy and sampled, whatever the drafter proposes.  Injected drafters:
``oracle`` proposes the plain engine's recorded continuation (everything accepted), ``wrong`` a token the
plain engine did not emit (nothing accepted), ``half`` two right tokens and then a wrong one.

The comparison is exact, so the test first asserts its own precondition on the plain engine's logits: a verify
step runs its GEMMs over more rows than a plain step, which may round an fp32 logit differently, so the top-2
margin of every plain step is at least 1e-3 (greedy) and every sampled draw is unchanged when the logits are
moved by +-1e-3 in an alternating pattern (sampled).  If a seed breaks the precondition, pick another seed.
"""
import math
import random

import pytest
import torch

from mxllm.models import Llama, get_config
from mxllm.ops import decode as dops
from mxllm.serve.engine import Engine, SamplingParams
from mxllm.serve.speculate import NgramIndex, prompt_lookup
from tests import _lora_serve as L

MAX_SEQ, POOL, NEW, K = 1024, 4096, 12, 3
STATS_KEYS = ["requests_finished", "tokens_generated", "mean_ttft_s", "mean_latency_s", "prefill_tokens_per_s",
              "decode_tokens_per_s", "decode_steps", "kv_cache_dtype", "kv_cache_bytes", "lora_adapters",
              "prefix_cache_query_tokens", "prefix_cache_hit_tokens", "prefill_chunks"]
SPEC_KEYS = ["spec_steps", "spec_draft_tokens", "spec_accepted_tokens"]


def toks(n, seed, vocab=512):
    return torch.randint(3, vocab - 3, (n,), generator=torch.Generator().manual_seed(seed)).tolist()


# the last one crosses a 256-token block while decoding; seeds 114 .. 116 meet the precondition (100 and 107 did not)
PROMPTS = [toks(5, 114), toks(41, 115), toks(250, 116)]


# =========================================================================== drafter
def test_prompt_lookup_proposes_the_continuation_of_the_most_recent_match():
    #       0  1  2  3  4  5  6  7  8  9
    t = [7, 8, 9, 1, 7, 8, 9, 2, 7, 8, 9]
    assert prompt_lookup(t, 3) == [2, 7, 8]  # 7 8 9 ended last at 6 (not at 2, whose follower is 1)
    assert prompt_lookup(t, 1) == [2]
    assert prompt_lookup(t, 8) == [2, 7, 8, 9]  # runs into the tail and stops at the end


def test_prompt_lookup_prefers_the_longer_ngram():
    # ... 5 6 -> 1 (older), 6 -> 2 (more recent): the 2-gram wins over the more recent 1-gram
    t = [4, 5, 6, 1, 3, 6, 2, 0, 5, 6]
    assert prompt_lookup(t, 2) == [1, 3]
    assert prompt_lookup([9, 6, 2, 0, 5, 6], 2) == [2, 0]  # no earlier 5 6: the 1-gram


def test_prompt_lookup_without_a_match_and_never_more_than_k():
    assert prompt_lookup([1, 2, 3, 4], 3) == []
    assert prompt_lookup([], 3) == [] and prompt_lookup([5], 3) == []
    assert prompt_lookup([5, 5], 3) == [5]  # the earlier 5 has one follower
    assert prompt_lookup([1, 2, 1, 2, 1, 2], 0) == []
    for k in range(1, 6):
        assert prompt_lookup([1, 2, 3] * 5, k) == [1, 2, 3][:k]  # the most recent match has three followers
        assert prompt_lookup([1, 2, 3] * 5 + [9, 1, 2, 3], k) == [9, 1, 2, 3][:k]  # ... and the later one four


def test_incremental_index_equals_the_search_after_every_append():
    rng = random.Random(5)
    idx, seq = NgramIndex(), []
    for _ in range(200):
        t = rng.randrange(6)
        idx.append(t)
        seq.append(t)
        for k in (1, 3, 5):
            assert idx.propose(k) == prompt_lookup(seq, k), (seq, k)
    other = NgramIndex(seq[:50])
    other.sync(seq)
    assert other.propose(4) == prompt_lookup(seq, 4) and len(other) == 200


# =========================================================================== accept op
def test_spec_accept_cpu():
    n = 4
    tokens = torch.tensor([[10, 11, 12, 13], [10, 11, 12, 13], [10, 11, 12, 13], [10, 11, 12, 13], [10, 0, 0, 0],
                           [10, 11, 12, 0], [0, 0, 0, 0]])
    drawn = torch.tensor([[99, 12, 13, 14],   # no draft right: the correction is row 0's draw
                          [11, 12, 77, 14],   # two right, the third wrong: the correction is row 2's draw
                          [11, 12, 13, 14],   # all right: the bonus is the last row's draw
                          [11, 55, 13, 14],   # a later match after a mismatch does not count
                          [42, 11, 12, 13],   # one row: its draw
                          [11, 12, 0, 9],     # nq = 3: row 3 is padding, although its "draft" 0 was drawn on row 2
                          [1, 2, 3, 4]])      # nq = 0
    nq = torch.tensor([4, 4, 4, 4, 1, 3, 0], dtype=torch.int32)
    out = dops.spec_accept(drawn, tokens, nq)
    assert out.dtype == torch.int32 and tuple(out.shape) == (7, n + 1)
    assert out.tolist() == [[0, 99, -1, -1, -1], [2, 11, 12, 77, -1], [3, 11, 12, 13, 14], [1, 11, 55, -1, -1],
                            [0, 42, -1, -1, -1], [2, 11, 12, 0, -1], [-1, -1, -1, -1, -1]]
    with pytest.raises(ValueError):
        dops.spec_accept(drawn, tokens[:, :3], nq)


# =========================================================================== verify attention, CPU expression
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "kv8"])
def test_verify_attn_cpu_rows_are_decode_rows(fp8):
    from mxllm.serve.quant import kv8_quantize

    g = torch.Generator().manual_seed(3)
    Hq, Hkv, D, n, blk = 4, 2, 128, 3, 256
    bt = torch.tensor([[2, 0], [1, 3]], dtype=torch.int32)
    k = torch.randn(4, Hkv, blk, D, generator=g).to(torch.bfloat16)
    v = torch.randn(4, Hkv, blk, D, generator=g).to(torch.bfloat16)
    q = torch.randn(3 * n, Hq, D, generator=g).to(torch.bfloat16)
    lens, nq, slots = torch.tensor([254, 7, 100]), torch.tensor([3, 1, 0]), torch.tensor([1, 0, 1])
    scale = 1 / math.sqrt(D)
    if fp8:
        (kc, ks), (vc, vs) = kv8_quantize(k), kv8_quantize(v)
        out = dops.verify_attn(q, kc, vc, lens, nq, slots, n, 512, scale, bt, ks, vs)
    else:
        out = dops.verify_attn(q, k, v, lens, nq, slots, n, 512, scale, bt)
    assert tuple(out.shape) == (3 * n, Hq * D)
    for b in range(3):
        for j in range(n):
            if j >= int(nq[b]):
                assert not out[b * n + j].any()
                continue
            one = (q[b * n + j:b * n + j + 1], torch.tensor([int(lens[b]) + j]), slots[b:b + 1])
            if fp8:
                want = dops.decode_attn_kv8(one[0], kc, ks, vc, vs, one[1], one[2], 512, scale, 1, bt)
            else:  # the expression of decode_attention's CPU path
                kk = dops._kv_at(k, bt, int(slots[b]), 0, int(lens[b]) + j + 1).float().repeat_interleave(Hq // Hkv, 0)
                vv = dops._kv_at(v, bt, int(slots[b]), 0, int(lens[b]) + j + 1).float().repeat_interleave(Hq // Hkv, 0)
                sc = torch.einsum("hd,hld->hl", q[b * n + j].float(), kk) * scale
                want = torch.einsum("hl,hld->hd", sc.softmax(-1), vv).reshape(1, -1).to(q.dtype)
            assert torch.equal(out[b * n + j:b * n + j + 1], want), (b, j)


# =========================================================================== engine
def _record_logits(eng):
    """Every logits tensor the engine samples from, with the requests of the draw."""
    seen, orig = [], eng._sample

    def sample(logits, reqs, first=False):
        seen.append((logits[:len(reqs)].detach().float().clone(), list(reqs), first))
        return orig(logits, reqs, first)

    eng._sample = sample
    return seen


def _plain(model, params, **kw):
    """The plain engine's outputs for PROMPTS with the test's precondition asserted on its logits."""
    eng = Engine(model, max_batch=4, max_seq=MAX_SEQ, kv_pool_tokens=POOL, **kw)
    seen = _record_logits(eng)
    reqs = [eng.submit(p, params) for p in PROMPTS]
    while not all(r.done.is_set() for r in reqs):
        eng.step()
    flip = torch.tensor([1.0, -1.0]).repeat(model.cfg.vocab_size // 2)
    for logits, rs, first in seen:
        if params.temperature <= 0:
            top = logits.topk(2, -1).values
            assert float((top[:, 0] - top[:, 1]).min()) >= 1e-3, "precondition: a top-2 margin below 1e-3; pick another seed"
            continue
        ps = [r.params for r in rs]
        steps = [len(r.output) for r in rs]  # (recorded after the run: only the draws' stability is checked)
        args = ([p.temperature for p in ps], [p.top_p for p in ps], [p.top_k for p in ps], [p.seed for p in ps], steps)
        want = dops.sample_rows(logits, *args).tolist()
        for sign in (1e-3, -1e-3):
            assert dops.sample_rows(logits + sign * flip, *args).tolist() == want, \
                "precondition: a draw changes under a 1e-3 move of the logits; pick another seed"
    return [r.output for r in reqs], eng


def _drafter(kind, base, vocab):
    """``oracle`` / ``wrong`` / ``half`` over the plain engine's outputs ``base`` of PROMPTS."""
    def draft(tokens, k):
        for p, out in zip(PROMPTS, base):
            if tokens[:len(p)] == p and len(tokens) > len(p):
                at = len(tokens) - len(p)
                right = out[at:at + k]
                if kind == "oracle":
                    return right
                if kind == "wrong":
                    return [(t + 1) % vocab for t in right[:1]] * k
                return [t if j % 3 < 2 else (t + 1) % vocab for j, t in enumerate(right)]
        raise AssertionError("the drafter was asked about an unknown request")

    return draft


@pytest.fixture(scope="module", params=["tiny", "tiny-d128"])
def models(request):
    cfg = get_config(request.param)
    model = Llama(cfg, seed=0, dtype=torch.float32).eval()
    greedy = SamplingParams(max_new_tokens=NEW)
    sampled = SamplingParams(max_new_tokens=NEW, temperature=0.8, top_p=0.9, seed=1234)
    return cfg, model, {"greedy": (greedy, _plain(model, greedy)[0]), "sampled": (sampled, _plain(model, sampled)[0])}


def _spec(model, drafter, **kw):
    kw.setdefault("kv_pool_tokens", POOL)
    return Engine(model, max_batch=4, max_seq=MAX_SEQ, speculate=K, drafter=drafter, **kw)


def _run(eng, params, prompts=PROMPTS):
    reqs = [eng.submit(p, params) for p in prompts]
    while not all(r.done.is_set() for r in reqs):
        eng.step()
    assert all(r.error is None for r in reqs), [r.error for r in reqs]
    return reqs


@pytest.mark.parametrize("mode", ["greedy", "sampled"])
@pytest.mark.parametrize("kind", ["oracle", "wrong", "half"])
def test_engine_emits_the_plain_stream(models, kind, mode):
    cfg, model, plain = models
    params, base = plain[mode]
    eng = _spec(model, _drafter(kind, base, cfg.vocab_size))
    reqs = _run(eng, params)
    assert [r.output for r in reqs] == base
    st = eng.stats()
    assert st["spec_steps"] > 0 and st["spec_draft_tokens"] > 0
    assert st["tokens_generated"] == len(PROMPTS) * NEW
    if kind == "oracle":
        assert st["spec_accepted_tokens"] == st["spec_draft_tokens"]
        # the first token comes from the prefill, the other NEW - 1 in runs of at most K + 1
        assert st["decode_steps"] == st["spec_steps"] == math.ceil((NEW - 1) / (K + 1))
    elif kind == "wrong":
        assert st["spec_accepted_tokens"] == 0 and st["decode_steps"] == NEW - 1
    else:
        assert 0 < st["spec_accepted_tokens"] < st["spec_draft_tokens"]


def test_lens_blocks_and_prefix_cache(models):
    """lens = prompt + emitted - 1 at the end of a request as in the plain engine, and both the paged pool and
    the prefix cache get every block back."""
    cfg, model, plain = models
    params, base = plain["greedy"]
    for kw in (dict(), dict(prefix_cache=True), dict(prefix_cache=True, prefill_chunk=64)):
        eng = _spec(model, _drafter("half", base, cfg.vocab_size), **kw)
        ends, orig = [], eng._finish

        def finish(r, reason, eng=eng, ends=ends, orig=orig):
            ends.append((len(r.prompt) + len(r.output) - 1, eng.lens[r.slot]))
            orig(r, reason)

        eng._finish = finish
        assert [r.output for r in _run(eng, params)] == base
        assert len(ends) == len(PROMPTS) and all(a == b for a, b in ends), ends
        kv = eng.kv
        assert len(kv.free) + len(kv.lru) == kv.n_blocks - 1  # (one block is the spare slot's)
        assert not kw or not any(kv.ref)  # (the counts are kept with the prefix cache on)
        assert sorted(eng.free_slots) == list(range(4)) and not eng.active


def test_max_new_tokens_is_exact_when_a_run_would_overshoot(models):
    cfg, model, plain = models
    params, base = plain["greedy"]
    for new in (1, 2, 5, 6, 7):
        eng = _spec(model, _drafter("oracle", base, cfg.vocab_size))
        reqs = _run(eng, SamplingParams(max_new_tokens=new))
        assert [r.output for r in reqs] == [b[:new] for b in base], new
        assert all(r.finish_reason == "length" for r in reqs)
        # no row was ever placed past prompt + max_new_tokens - 1, the last position a request reads
        assert all(eng.lens[s] <= len(p) + new - 1 for s, p in zip(range(3), PROMPTS))


def test_eos_inside_an_accepted_run_ends_the_request_there(models):
    cfg, model, plain = models
    params, base = plain["greedy"]
    stop = base[1][6]  # inside the second run of request 1 (tokens 5 .. 8)
    want = Engine(model, max_batch=4, max_seq=MAX_SEQ, kv_pool_tokens=POOL, eos_ids=(stop,)).generate(
        PROMPTS, max_new_tokens=NEW)
    assert want[1] == base[1][:base[1].index(stop) + 1] and len(want[1]) < NEW
    eng = _spec(model, _drafter("oracle", base, cfg.vocab_size), eos_ids=(stop,))
    reqs = _run(eng, params)
    assert [r.output for r in reqs] == want
    assert reqs[1].finish_reason == "stop"
    # a stop_ids token of one request
    eng = _spec(model, _drafter("oracle", base, cfg.vocab_size))
    r = _run(eng, SamplingParams(max_new_tokens=NEW, stop_ids=(stop,)), [PROMPTS[1]])[0]
    assert r.output == want[1] and r.finish_reason == "stop"


def test_special_requests_get_no_drafts(models):
    cfg, model, plain = models
    asked = []

    def drafter(tokens, k):
        asked.append(len(tokens))
        return [5] * k

    for kw in (dict(logprobs=2), dict(presence_penalty=0.5), dict(logit_bias={7: 1.5})):
        params = SamplingParams(max_new_tokens=NEW, **kw)
        want = Engine(model, max_batch=4, max_seq=MAX_SEQ, kv_pool_tokens=POOL).generate(
            PROMPTS[:2], max_new_tokens=NEW, **kw)
        eng = _spec(model, drafter)
        assert [r.output for r in _run(eng, params, PROMPTS[:2])] == want
        st = eng.stats()
        assert not asked and st["spec_steps"] == st["spec_draft_tokens"] == 0 and st["decode_steps"] == NEW - 1
    # a special request beside a drafted one: one row, the adjusted sampling path on that row
    params, base = plain["greedy"]
    eng = _spec(model, _drafter("oracle", base, cfg.vocab_size))
    a = eng.submit(PROMPTS[0], params)
    b = eng.submit(PROMPTS[1], SamplingParams(max_new_tokens=NEW, logprobs=1))
    while not (a.done.is_set() and b.done.is_set()):
        eng.step()
    assert a.output == base[0] and b.output == base[1] and len(b.logprobs) == NEW
    assert eng.stats()["spec_accepted_tokens"] == eng.stats()["spec_draft_tokens"] > 0


def test_a_step_with_an_adapter_row_is_the_plain_step(models):
    cfg, model, plain = models
    params, base = plain["greedy"]
    ref = Engine(model, max_batch=4, max_seq=MAX_SEQ, kv_pool_tokens=POOL, max_adapters=1, max_lora_rank=16)
    ref.load_adapter("A", L.random_adapter(cfg, 16, 1))
    want = ref.generate(PROMPTS[:2], max_new_tokens=NEW, adapters=["A", None])
    eng = _spec(model, lambda tokens, k: [5] * k, max_adapters=1, max_lora_rank=16)
    eng.load_adapter("A", L.random_adapter(cfg, 16, 1))
    verified = []
    eng.verify = lambda *a, **k: verified.append(a) or (_ for _ in ()).throw(AssertionError("a verify step ran"))
    assert eng.generate(PROMPTS[:2], max_new_tokens=NEW, adapters=["A", None]) == want
    assert not verified and eng.stats()["spec_steps"] == 0
    # without the adapter row the same engine speculates again
    del eng.verify
    eng.drafter = _drafter("oracle", base, cfg.vocab_size)
    assert eng.generate(PROMPTS[:2], max_new_tokens=NEW) == base[:2] and eng.stats()["spec_steps"] > 0


def test_default_drafter_is_prompt_lookup(models):
    """A prompt that repeats itself drafts from its own text; the stream is the plain engine's."""
    cfg, model, _ = models
    prompt = (toks(9, 21) * 6)[:50]
    want = Engine(model, max_batch=2, max_seq=MAX_SEQ).generate([prompt], max_new_tokens=NEW)
    eng = Engine(model, max_batch=2, max_seq=MAX_SEQ, speculate=K)
    r = _run(eng, SamplingParams(max_new_tokens=NEW), [prompt])[0]
    assert [r.output] == want
    assert eng.stats()["spec_draft_tokens"] > 0 and r.spec_index is not None
    assert r.spec_index.tokens == (prompt + r.output)[:len(r.spec_index)]


def test_option_errors(models, monkeypatch):
    cfg, model, _ = models
    with pytest.raises(ValueError, match="speculate must be >= 0"):
        Engine(model, speculate=-1)
    group = cfg.n_heads // cfg.n_kv_heads
    kmax = 32 // group - 1
    Engine(model, max_batch=1, max_seq=256, speculate=kmax)
    with pytest.raises(ValueError, match=f"speculate <= {kmax}"):
        Engine(model, max_batch=1, max_seq=256, speculate=kmax + 1)
    with pytest.raises(ValueError, match="tensor parallelism"):
        Engine(model, speculate=2, tp_group=object())
    monkeypatch.setenv("MXLLM_SPECULATE", "2")
    assert Engine(model, max_batch=1, max_seq=256).speculate == 2
    assert Engine(model, max_batch=1, max_seq=256, speculate=0).speculate == 0
    monkeypatch.setenv("MXLLM_SPECULATE", "0")
    assert Engine(model, max_batch=1, max_seq=256).speculate == 0
    with pytest.raises(ValueError, match="without speculate"):
        Engine(model, max_batch=1, max_seq=256).verify([0], [[1]])


def test_off_by_default_nothing_changes(models, monkeypatch):
    monkeypatch.delenv("MXLLM_SPECULATE", raising=False)
    cfg, model, plain = models
    params, base = plain["greedy"]
    eng = Engine(model, max_batch=4, max_seq=MAX_SEQ, kv_pool_tokens=POOL)
    assert eng.speculate == 0 and eng.kv.scratch_slot is None
    assert eng.generate(PROMPTS, max_new_tokens=NEW) == base
    st = eng.stats()
    assert list(st) == STATS_KEYS + SPEC_KEYS and all(st[k] == 0 for k in SPEC_KEYS)
    assert eng._graphs == {}
