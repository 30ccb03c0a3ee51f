"""Prefix cache and chunked prefill of the serving engine on the GPU (``tiny-d128``: head_dim 128, so every
prefill chunk runs csrc/kernels/prefill_paged.hip): the wiring of ``Engine.prefill_segments``,
``dops.prefill_attention_paged`` and the shared blocks.  The per-element truth of the kernel is
tests/test_prefill_paged_gpu.py; here last-row logits are compared with ``prefill_batch`` on a fresh engine
of the same weights by per-row cosine (> 0.99, the criterion of tests/test_kv8_gpu.py), the two GPU routes
with each other, and the exact block accounting of tests/test_prefix_cache.py is repeated on the device.
"""
import pytest
import torch

from mxllm.models import Llama, get_config
from mxllm.serve.engine import Engine, SamplingParams

pytestmark = pytest.mark.gpu

MAX_SEQ, POOL, NEW = 1024, 4096, 6


def toks(n, seed, vocab=512):
    return torch.randint(3, vocab - 3, (n,), generator=torch.Generator().manual_seed(seed)).tolist()


SHORT, LONG = toks(57, 2), toks(600, 4)
TAILED = LONG[:512] + toks(40, 9)


@pytest.fixture(scope="module")
def setup(gpu):
    model = Llama(get_config("tiny-d128"), device=gpu, seed=9).eval()
    ref = Engine(model, max_batch=2, max_seq=MAX_SEQ, kv_pool_tokens=POOL, use_graphs=False)
    ref.reserve(0, 700)
    ref.reserve(1, 100)
    want = ref.prefill_batch([0, 1], [LONG, SHORT])  # [2, V]: last-row logits of the 600- and the 57-token prompt
    ref.reserve(0, 700)
    want_tailed = ref.prefill_batch([0], [TAILED])[0]
    return model, want, want_tailed


def engine(model, use_graphs=False, **kw):
    return Engine(model, max_batch=2, max_seq=MAX_SEQ, kv_pool_tokens=POOL, use_graphs=use_graphs, eos_ids=(-1,), **kw)


def cos_rows(a, b):
    return torch.nn.functional.cosine_similarity(a.float(), b.float(), dim=-1)


def chunked_logits(eng, chunk):
    """LONG in slot 0 and SHORT in slot 1 through prefill_segments in passes of ``chunk`` tokens per prompt."""
    eng.reserve(0, 700)
    eng.reserve(1, 100)
    last = {}
    for st in range(0, len(LONG), chunk):
        slots, chunks, starts = [0], [LONG[st:st + chunk]], [st]
        if st < len(SHORT):
            slots, chunks, starts = slots + [1], chunks + [SHORT[st:st + chunk]], starts + [st]
        lg = eng.prefill_segments(slots, chunks, starts)
        for s_, row in zip(slots, lg):
            last[s_] = row
    assert eng.lens[0] == len(LONG) and eng.lens[1] == len(SHORT)
    return torch.stack([last[0], last[1]])


@pytest.mark.parametrize("chunk", [256, 100])
def test_chunked_prefill_logits_match_prefill_batch(setup, chunk):
    model, want, _ = setup
    cos = cos_rows(chunked_logits(engine(model, prefill_chunk=chunk), chunk), want)
    assert float(cos.min()) > 0.99, cos


def test_routes_hip_and_gather_agree(setup, monkeypatch):
    model, want, _ = setup
    got = {}
    for route in ("hip", "gather"):
        monkeypatch.setenv("MXLLM_PREFILL_PAGED", route)
        got[route] = chunked_logits(engine(model, prefill_chunk=100), 100)
        assert float(cos_rows(got[route], want).min()) > 0.99, route
    assert float(cos_rows(got["hip"], got["gather"]).min()) > 0.99


@pytest.mark.parametrize("use_graphs", [False, True], ids=["eager", "graphed"])
def test_prefix_hit_logits_and_accounting(setup, use_graphs):
    model, want, want_tailed = setup
    eng = engine(model, use_graphs=use_graphs, prefix_cache=True)
    kv = eng.kv
    sp = lambda: SamplingParams(max_new_tokens=NEW)
    r1 = eng.generate([LONG], max_new_tokens=NEW, return_requests=True)[0]
    assert r1.cached_tokens == 0 and len(r1.output) == NEW
    first = kv.match_prefix(LONG)
    assert len(first) == 2 and kv.evictable_blocks == 2
    snap = [(k[first].clone(), v[first].clone()) for k, v in zip(kv.k, kv.v)]

    # logits after a 512-token hit: the remainder through prefill_segments over the shared blocks
    shared = kv.match_prefix(TAILED)
    assert shared == first
    kv.reserve(1, 700, shared=shared)
    lg = eng.prefill_segments([1], [TAILED[512:]], [512])[0]
    assert float(cos_rows(lg, want_tailed)) > 0.99
    kv.release(1)

    r2 = eng.submit(LONG, sp())
    eng.step()
    assert r2.cached_tokens == 512 and kv.owned[r2.slot][:2] == first and [kv.ref[b] for b in first] == [1, 1]
    assert kv.bt[r2.slot, :2].tolist() == first
    r3 = eng.submit(TAILED, sp())
    eng.step()
    assert r3.cached_tokens == 512 and kv.owned[r3.slot][:2] == first and [kv.ref[b] for b in first] == [2, 2]
    assert kv.bt[r3.slot, :2].tolist() == first
    while not (r2.done.is_set() and r3.done.is_set()):
        eng.step()
    assert r2.error is None and r3.error is None and len(r2.output) == NEW and len(r3.output) == NEW
    st = eng.stats()
    assert st["prefix_cache_hit_tokens"] == 1024 and st["prefix_cache_query_tokens"] == 600 + 600 + 552
    for (k0, v0), k, v in zip(snap, kv.k, kv.v):  # shared blocks are never written
        assert torch.equal(k[first].view(torch.int16), k0.view(torch.int16))
        assert torch.equal(v[first].view(torch.int16), v0.view(torch.int16))
    assert not any(kv.ref) and set(kv.owned) <= {eng.scratch_slot}
    assert kv.free_blocks + kv.evictable_blocks == POOL // 256


@pytest.mark.parametrize("use_graphs", [False, True], ids=["eager", "graphed"])
def test_generate_with_both_options_on(setup, use_graphs):
    model, _, _ = setup
    eng = engine(model, use_graphs=use_graphs, prefix_cache=True, prefill_chunk=128)
    prompts = [LONG, SHORT, TAILED, toks(300, 5), LONG[:256] + toks(9, 6), toks(3, 7)]  # 6 prompts, 2 slots
    rs = eng.generate(prompts, max_new_tokens=NEW, return_requests=True)
    assert [len(r.output) for r in rs] == [NEW] * 6 and all(r.error is None for r in rs)
    assert rs[2].cached_tokens == 512 and rs[4].cached_tokens == 256  # LONG finished before they were admitted
    assert not any(eng.kv.ref) and eng.kv.free_blocks + eng.kv.evictable_blocks == POOL // 256
    assert eng.stats()["prefill_chunks"] >= 5 + 1 + 1 + 3 + 1 + 1
