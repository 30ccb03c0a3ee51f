"""Speculative decoding of the serving engine on the GPU (``tiny-d128``, eager and graphed, bf16 and fp8 KV
cache): ``Engine(speculate=3, drafter=...)`` on the HIP verify-attention and accept kernels.

The verify attention is bit for bit the plain kernel's (tests/test_verify_attn_gpu.py), but the GEMMs of a
step with 12 rows and of a step with 3 rows round differently, and the bf16 logits of this random model tie
often (the smallest top-2 margin of the plain engine's decode steps is 0 on most seeds), so token equality
with the plain engine is not the criterion here.  Instead a plain engine teacher-forces the speculative
engine's prompt + output through ``prefill_batch``, and every emitted token must lie within DELTA of that
position's largest logit.

DELTA: on the parent commit, the largest |decode logit - prefill logit| over the output positions of the
same sequences through the two paths that exist there (the plain decode step and ``prefill_batch``; these
prompt lengths, 12 new tokens, six prompt seeds, eager and graphed gave the same figures) is 0.015625 with the
bf16 cache and 0.0546875 with the fp8 cache (prefill attends over the fresh bf16 K/V, decode over the
quantised rows).  The speculative step and the reference can each be off by that much: DELTA is twice it.
(profiles/speculative/README.md has the measurement.)

Drafters: ``oracle`` proposes a recorded continuation; the record starts as the plain engine's output and,
where a tie falls the other way in the speculative engine, is replaced by that run's own output until a run
reproduces its record -- the kernels are deterministic, so this ends after a run or two -- and then every
draft is accepted.  ``wrong`` proposes the recorded token + 1: nothing is accepted.  ``half``: two recorded
tokens, then a wrong one.
"""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

NEW, K = 12, 3
MEASURED = {"bf16": 0.015625, "fp8": 0.0546875}  # max |decode logit - prefill logit| on the parent commit
DELTA = {kv: 2 * v for kv, v in MEASURED.items()}
MODES = [(False, "bf16"), (True, "bf16"), (False, "fp8"), (True, "fp8")]
MODE_IDS = ["eager-bf16", "graphed-bf16", "eager-fp8", "graphed-fp8"]


def toks(n, seed, vocab=512):
    return torch.randint(3, vocab - 3, (n,), generator=torch.Generator().manual_seed(seed)).tolist()


PROMPTS = [toks(5, 114), toks(41, 115), toks(250, 116)]  # the last one crosses a 256-token block while decoding


@functools.lru_cache(maxsize=None)
def _model():
    from mxllm.models import Llama, get_config

    cfg = get_config("tiny-d128")
    return cfg, Llama(cfg, device="cpu", seed=9).eval().to(torch.device("cuda", 0))


def _engine(graphs, kv, **kw):
    from mxllm.serve.engine import Engine

    kw.setdefault("kv_pool_tokens", 2048)
    return Engine(_model()[1], max_batch=4, max_seq=512, use_graphs=graphs, kv_dtype=kv, **kw)


@functools.lru_cache(maxsize=None)
def _plain_outputs(graphs, kv):
    return _engine(graphs, kv).generate(PROMPTS, max_new_tokens=NEW)


@functools.lru_cache(maxsize=None)
def _ref_engine(kv):
    from mxllm.serve.engine import Engine

    return Engine(_model()[1], max_batch=NEW, max_seq=512, use_graphs=False, kv_dtype=kv)


def check_within_delta(outputs, kv, what):
    """Every emitted token's logit in the plain engine's prefill of the same prefix is within DELTA of the
    row's largest; prints the largest shortfall."""
    ref, worst = _ref_engine(kv), 0.0
    for p, out in zip(PROMPTS, outputs):
        assert len(out) == NEW
        seq = p + out
        lg = ref.prefill_batch(list(range(NEW)), [seq[:len(p) + t] for t in range(NEW)]).float().cpu()  # [NEW, V]
        for s in range(NEW):
            ref.kv.release(s)
        short = lg.max(-1).values - lg[torch.arange(NEW), torch.tensor(out)]
        worst = max(worst, float(short.max()))
        assert float(short.max()) <= DELTA[kv], (what, kv, short.tolist())
    print(f"{what}, {kv}: largest shortfall of an emitted token below its row's maximum {worst:.6g}, DELTA {DELTA[kv]}")


def make_drafter(kind, record, vocab):
    def draft(tokens, k):
        for p, out in zip(PROMPTS, record):
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


def run(graphs, kv, kind, record):
    cfg = _model()[0]
    eng = _engine(graphs, kv, speculate=K, drafter=make_drafter(kind, record, cfg.vocab_size))
    reqs = eng.generate(PROMPTS, max_new_tokens=NEW, return_requests=True)
    assert all(r.error is None and r.finish_reason == "length" for r in reqs), [r.error for r in reqs]
    return eng, [r.output for r in reqs]


@pytest.mark.parametrize("graphs,kv", MODES, ids=MODE_IDS)
def test_oracle_drafts_are_all_accepted(gpu, graphs, kv):
    record = _plain_outputs(graphs, kv)
    for _ in range(4):
        eng, out = run(graphs, kv, "oracle", record)
        if out == record:
            break
        record = out  # a tie fell the other way somewhere: the run's own output is the next record
    assert out == record, "no run reproduced its record"
    st = eng.stats()
    assert st["spec_accepted_tokens"] == st["spec_draft_tokens"] > 0
    # the first token comes from the prefill, the other NEW - 1 in runs of K + 1 (= ceil(NEW / (K + 1)) here)
    assert st["decode_steps"] == st["spec_steps"] == math.ceil((NEW - 1) / (K + 1)) == math.ceil(NEW / (K + 1))
    assert st["tokens_generated"] == len(PROMPTS) * NEW
    if graphs:
        assert {k[0] for k in eng._graphs} == {"verify"} and all(k[3] == K + 1 for k in eng._graphs)
    check_within_delta(out, kv, "oracle drafter")


@pytest.mark.parametrize("graphs,kv", MODES, ids=MODE_IDS)
def test_wrong_drafts_are_all_rejected(gpu, graphs, kv):
    eng, out = run(graphs, kv, "wrong", _plain_outputs(graphs, kv))
    st = eng.stats()
    # one token per step: the prefill's, then NEW - 1 decode steps; the last of them has no room for a draft
    assert st["spec_accepted_tokens"] == 0 and st["decode_steps"] == NEW - 1 and st["spec_steps"] == NEW - 2
    assert st["spec_draft_tokens"] > 0
    check_within_delta(out, kv, "wrong drafter")


@pytest.mark.parametrize("kv", ["bf16", "fp8"])
def test_graphed_and_eager_emit_the_same_tokens(gpu, kv):
    record = _plain_outputs(True, kv)
    outs = {}
    for graphs in (False, True):
        eng, outs[graphs] = run(graphs, kv, "half", record)
        assert eng.stats()["spec_draft_tokens"] > 0
    assert outs[False] == outs[True]
    check_within_delta(outs[True], kv, "half drafter")


def test_prefix_cache_chunked_prefill_and_speculation_together(gpu):
    """6 prompts on 2 slots with ``prefix_cache=True, prefill_chunk=128, speculate=3`` and the prompt-lookup
    drafter: every request finishes, and every block returns to the pool."""
    from mxllm.serve.engine import Engine

    shared = toks(256, 31) + (toks(7, 32) * 9)[:60]
    prompts = [shared + toks(3, 40 + i) for i in range(4)] + [(toks(5, 50) * 20)[:90], toks(33, 51)]
    eng = Engine(_model()[1], max_batch=2, max_seq=1024, kv_pool_tokens=4096, prefix_cache=True, prefill_chunk=128,
                 speculate=K)
    reqs = eng.generate(prompts, max_new_tokens=24, return_requests=True)
    assert all(r.error is None and r.finish_reason in ("length", "stop") for r in reqs), [r.error for r in reqs]
    assert all(0 < len(r.output) <= 24 for r in reqs)
    st = eng.stats()
    assert st["requests_finished"] == 6 and st["spec_steps"] > 0 and st["prefix_cache_hit_tokens"] > 0
    kv = eng.kv
    assert len(kv.free) + len(kv.lru) == kv.n_blocks - 1 and not any(kv.ref)  # (one block is the spare slot's)
    assert sorted(eng.free_slots) == [0, 1] and not eng.active and not eng.prefilling
