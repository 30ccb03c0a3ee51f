"""Prefix cache and chunked prefill of the serving engine on the CPU reference path (``tiny`` model):
``Engine(prefix_cache=True, prefill_chunk=N)``, ``Engine.prefill_segments`` and the shared,
reference-counted blocks of mxllm/serve/kvcache.py.

Greedy output must not depend on how a prompt is prefilled: whole, in chunks of 1 / 7 / 256 tokens, or
after a prefix-cache hit.  (Checked on these inputs before relying on them: the tokens are equal.)  The
block accounting is exact: hit tokens, the shared block ids, shared blocks bitwise unchanged, reference
counts back to zero, free + evictable = the pool, LRU eviction from a chain's tail, adapters as part of the key.
"""
import pytest
import torch

from mxllm.models import Llama, get_config
from mxllm.serve.engine import Engine, SamplingParams
from mxllm.serve.kvcache import KVCache
from tests import _lora_serve as L

MAX_SEQ, POOL, NEW = 1024, 4096, 6


def toks(n, seed, vocab=512):
    return torch.randint(3, vocab - 3, (n,), generator=torch.Generator().manual_seed(seed)).tolist()


PROMPTS = [toks(3, 1), toks(41, 2), toks(300, 3), toks(600, 4)]
LONG = PROMPTS[3]
TAILED = LONG[:512] + toks(40, 9)  # 512 shared tokens = two full blocks, then another tail


@pytest.fixture(scope="module")
def tiny():
    cfg = get_config("tiny")
    model = Llama(cfg, seed=0).eval()
    plain = Engine(model, max_batch=4, max_seq=MAX_SEQ, kv_pool_tokens=POOL)
    base = plain.generate(PROMPTS, max_new_tokens=NEW)
    return cfg, model, base, plain.generate([TAILED], max_new_tokens=NEW)[0]


def sp():
    return SamplingParams(max_new_tokens=NEW)


def engine(model, **kw):
    kw.setdefault("kv_pool_tokens", POOL)
    return Engine(model, max_batch=4, max_seq=MAX_SEQ, **kw)


@pytest.mark.parametrize("chunk", [1, 7, 256])
def test_chunked_prefill_gives_the_same_tokens(tiny, chunk):
    _, model, base, _ = tiny
    eng = engine(model, prefill_chunk=chunk)
    assert eng.generate(PROMPTS, max_new_tokens=NEW) == base
    n_tok = sum(len(p) for p in PROMPTS)
    assert eng.stats()["prefill_chunks"] >= -(-n_tok // chunk)
    assert eng.prefill_tokens == n_tok and not eng.prefilling


def test_chunked_prefill_interleaves_with_decode(tiny):
    """A running request gets a decode step between the chunks of a long prompt."""
    _, model, base, _ = tiny
    eng = engine(model, prefill_chunk=64)
    short = eng.submit(PROMPTS[0], sp())
    eng.step()
    assert len(short.output) >= 1
    long = eng.submit(LONG, sp())
    before = len(short.output)
    eng.step()  # one 64-token chunk of the long prompt, then a decode step of the short request
    assert long.prefilled == 64 and not long.output and len(short.output) == before + 1
    while not long.done.is_set():
        eng.step()
    assert long.output == base[3]


def test_prefill_segments_matches_prefill_batch(tiny):
    _, model, _, _ = tiny
    a, b = engine(model), engine(model, prefill_chunk=100)
    for e in (a, b):
        e.reserve(0, 700)
        e.reserve(1, 100)
    want = a.prefill_batch([0, 1], [LONG, PROMPTS[1]])
    got = None
    for st in range(0, 600, 100):
        slots, chunks, starts = [0], [LONG[st:st + 100]], [st]
        if st == 0:
            slots, chunks, starts = [0, 1], chunks + [PROMPTS[1]], [0, 0]
        lg = b.prefill_segments(slots, chunks, starts)
        got = lg if st == 0 else torch.cat([lg, got[1:]])
    cos = torch.nn.functional.cosine_similarity(got.double(), want.double(), dim=-1)
    assert float(cos.min()) > 0.9999, cos
    assert b.lens[0] == 600 and b.lens[1] == 41


def test_prefix_cache_tokens_and_accounting(tiny):
    _, model, base, tailed = tiny
    eng = engine(model, prefix_cache=True)
    kv = eng.kv
    r1 = eng.generate([LONG], max_new_tokens=NEW, return_requests=True)[0]
    assert r1.output == base[3] and r1.cached_tokens == 0
    first = kv.match_prefix(LONG)  # the first request's two full prompt blocks
    assert len(first) == 2 and kv.evictable_blocks == 2
    snap = [(k[first].clone(), v[first].clone()) for k, v in zip(kv.k, kv.v)]

    r2 = eng.submit(LONG, sp())
    eng.step()
    assert r2.cached_tokens == 512 and kv.owned[r2.slot][:2] == first and [kv.ref[b] for b in first] == [1, 1]
    assert kv.bt_host[r2.slot, :2].tolist() == first and kv.bt[r2.slot, :2].tolist() == first
    r3 = eng.submit(TAILED, sp())
    eng.step()
    assert r3.cached_tokens == 512 and kv.owned[r3.slot][:2] == first and [kv.ref[b] for b in first] == [2, 2]
    assert kv.bt_host[r3.slot, :2].tolist() == first
    while not (r2.done.is_set() and r3.done.is_set()):
        eng.step()
    assert r2.output == base[3] and r3.output == tailed
    st = eng.stats()
    assert st["prefix_cache_hit_tokens"] == 1024 and st["prefix_cache_query_tokens"] == 600 + 600 + 552
    assert st["prefill_chunks"] == 3 and eng.prefill_tokens == 600 + 88 + 40
    for (k0, v0), k, v in zip(snap, kv.k, kv.v):  # shared blocks are never written
        assert torch.equal(k[first].view(torch.int16), k0.view(torch.int16))
        assert torch.equal(v[first].view(torch.int16), v0.view(torch.int16))
    assert not any(kv.ref) and not kv.owned
    assert kv.free_blocks + kv.evictable_blocks == POOL // 256
    assert sorted(kv.free + list(kv.lru)) == list(range(POOL // 256))


def test_two_requests_of_one_admission_pass_both_miss(tiny):
    _, model, base, _ = tiny
    eng = engine(model, prefix_cache=True)
    rs = eng.generate([LONG, LONG], max_new_tokens=NEW, return_requests=True)
    assert [r.cached_tokens for r in rs] == [0, 0] and [r.output for r in rs] == [base[3], base[3]]
    assert len(eng.kv.index) == 2  # the second request kept its own copies; the index the first one's
    assert eng.generate([LONG], max_new_tokens=NEW, return_requests=True)[0].cached_tokens == 512
    assert not any(eng.kv.ref) and eng.kv.free_blocks + eng.kv.evictable_blocks == POOL // 256


def test_multi_turn_reuses_prompt_and_output(tiny):
    """At finish the blocks below the written length are registered: prompt AND output."""
    _, model, _, _ = tiny
    eng = engine(model, prefix_cache=True)
    p = toks(250, 11)
    r = eng.generate([p], max_new_tokens=10, return_requests=True)[0]  # 259 positions written: one full block
    turn2 = p + r.output + toks(30, 12)
    assert len(eng.kv.match_prefix(turn2)) == 1
    plain = engine(model).generate([turn2], max_new_tokens=NEW)[0]
    r2 = eng.generate([turn2], max_new_tokens=NEW, return_requests=True)[0]
    assert r2.cached_tokens == 256 and r2.output == plain


def test_eviction_lru_chain_tail_first_never_a_referenced_block(tiny):
    _, model, _, _ = tiny
    eng = Engine(model, max_batch=4, max_seq=MAX_SEQ, kv_pool_tokens=6 * 256, prefix_cache=True)
    kv = eng.kv
    A, B = LONG, toks(600, 21)
    eng.generate([A], max_new_tokens=NEW)
    eng.generate([B], max_new_tokens=NEW)
    a, b = kv.match_prefix(A), kv.match_prefix(B)
    assert len(a) == 2 and len(b) == 2 and list(kv.lru) == [a[1], a[0], b[1], b[0]] and kv.free_blocks == 2
    evicted = []
    orig = kv._evict
    kv._evict = lambda: evicted.append(orig()) or evicted[-1]
    # a request that shares B's chain keeps it referenced while a 4-block request needs 2 evictions
    rb = eng.submit(B, sp())
    eng.step()
    assert rb.cached_tokens == 512 and [kv.ref[x] for x in b] == [1, 1] and list(kv.lru) == [a[1], a[0]]
    assert kv.free_blocks == 1 and kv.can_reserve(3 * 256) and not kv.can_reserve(4 * 256)
    c = eng.submit(toks(700, 22), sp())  # 3 blocks: the free one and A's chain, last block first
    eng.step()
    assert c.slot >= 0 and evicted == [a[1], a[0]]
    assert kv.match_prefix(A) == [] and kv.match_prefix(B) == b and [kv.ref[x] for x in b] == [1, 1]
    d = eng.submit(toks(300, 23), sp())  # 2 blocks: nothing free, nothing evictable -> waits, B's blocks stay
    eng.step()
    assert d.slot == -1 and evicted == [a[1], a[0]] and kv.match_prefix(B) == b
    while not all(r.done.is_set() for r in (rb, c, d)):
        eng.step()
    assert all(r.error is None and r.output for r in (rb, c, d))
    assert not any(kv.ref) and kv.free_blocks + kv.evictable_blocks == 6


def test_kvcache_chain_semantics():
    kv = KVCache(1, 1, 8, torch.float32, torch.device("cpu"), n_slots=3, max_seq=1024, pool_tokens=8 * 256,
                 prefix_cache=True)
    t = toks(800, 31)
    kv.reserve(0, 800)
    assert kv.register(0, t, None, upto=511) == 1  # only blocks fully below the written length
    assert kv.register(0, t, None, upto=800) == 2  # ... the rest later; block 0 is not entered twice
    own = list(kv.owned[0])
    assert kv.match_prefix(t) == own[:3] and kv.match_prefix(t[:768]) == own[:2]  # >= 1 token always computed
    assert kv.match_prefix(t[:256] + t[512:768]) == own[:1]  # block 2's tokens do not match as block 1
    assert kv.match_prefix(t, "adapter") == []
    # a second slot with the same tokens keeps its own copies
    kv.reserve(1, 800)
    assert kv.register(1, t, None) == 0 and kv.match_prefix(t) == own[:3]
    kv.release(1)
    assert kv.free_blocks == 4 and kv.evictable_blocks == 0
    kv.release(0)
    assert list(kv.lru) == [own[2], own[1], own[0]] and kv.free_blocks == 5  # own[3] was never full
    # entry ids are never reused: evict the chain's head only; its children are unreachable for good
    kv.lru.move_to_end(own[0], last=False)
    assert kv._evict() == own[0] and kv.match_prefix(t) == []
    kv.reserve(2, 256)
    kv.register(2, t[:256], None)
    assert len(kv.match_prefix(t)) == 1  # the new head has a new id: the old children do not hang off it
    with pytest.raises(ValueError):
        KVCache(1, 1, 8, torch.float32, torch.device("cpu"), n_slots=2, max_seq=512, prefix_cache=True)


def test_adapter_is_part_of_the_key(tiny):
    cfg, model, _, _ = tiny
    eng = engine(model, prefix_cache=True, max_adapters=2, max_lora_rank=16)
    eng.load_adapter("A", L.random_adapter(cfg, 16, 1))
    eng.load_adapter("B", L.random_adapter(cfg, 8, 2))
    ref = engine(model, max_adapters=2, max_lora_rank=16)
    ref.load_adapter("A", L.random_adapter(cfg, 16, 1))
    want = ref.generate([LONG], max_new_tokens=NEW, adapters=["A"])[0]

    def run(adapter):
        r = eng.generate([LONG], max_new_tokens=NEW, adapters=[adapter], return_requests=True)[0]
        return r.cached_tokens, r.output

    assert run("A") == (0, want)
    assert run("A") == (512, want)
    assert run("B")[0] == 0 and run(None)[0] == 0  # A's blocks serve neither B nor the base model
    assert run("B")[0] == 512 and run(None)[0] == 512
    n = len(eng.kv.index)
    eng.unload_adapter("A")
    assert len(eng.kv.index) == n - 2 and eng.kv.match_prefix(LONG, "A") == []
    assert len(eng.kv.match_prefix(LONG, "B")) == 2
    assert eng.kv.free_blocks + eng.kv.evictable_blocks == POOL // 256


def test_options_that_are_not_supported_raise(tiny):
    _, model, _, _ = tiny
    with pytest.raises(ValueError, match="kv_pool_tokens"):
        Engine(model, max_batch=2, max_seq=512, prefix_cache=True)
    for kw in (dict(prefix_cache=True), dict(prefill_chunk=64)):
        with pytest.raises(ValueError, match="tensor parallelism"):
            Engine(model, max_batch=2, max_seq=512, kv_pool_tokens=2048, tp_group=object(), **kw)
    with pytest.raises(ValueError, match="prefill_chunk"):
        engine(model, prefill_chunk=0)
    cfg128 = get_config("tiny-d128")
    m128 = Llama(cfg128, seed=0).eval().to(torch.bfloat16)
    for kw in (dict(prefix_cache=True), dict(prefill_chunk=64)):
        with pytest.raises(ValueError, match="fp8"):
            Engine(m128, max_batch=2, max_seq=512, kv_pool_tokens=2048, kv_dtype="fp8", **kw)
    assert not Engine(model, max_batch=2, max_seq=512).paged_prefill  # the defaults: today's paths


def test_env_switches(tiny, monkeypatch):
    _, model, base, _ = tiny
    monkeypatch.setenv("MXLLM_PREFIX_CACHE", "1")
    monkeypatch.setenv("MXLLM_PREFILL_CHUNK", "128")
    monkeypatch.setenv("MXLLM_KV_POOL_TOKENS", str(POOL))
    eng = Engine(model, max_batch=4, max_seq=MAX_SEQ)
    assert eng.prefix_cache and eng.prefill_chunk == 128 and eng.kv.prefix_cache
    assert eng.generate(PROMPTS, max_new_tokens=NEW) == base


def test_bad_prompt_lengths_are_rejected_at_admission(tiny):
    """Known before the first chunk runs: an empty prompt, a prompt that does not fit max_seq."""
    _, model, base, _ = tiny
    eng = Engine(model, max_batch=2, max_seq=512, kv_pool_tokens=2048, prefill_chunk=64)
    bad = [eng.submit(p, sp()) for p in ([], toks(512, 41))]
    ok = eng.submit(PROMPTS[1], sp())
    while not ok.done.is_set():
        eng.step()
    assert all(r.done.is_set() and r.finish_reason == "error" and "max_seq" in r.error for r in bad)
    assert ok.output == base[1] and eng.stats()["prefill_chunks"] == 1
