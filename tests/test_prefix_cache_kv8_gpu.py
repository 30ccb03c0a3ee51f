"""tests/test_prefix_cache_gpu.py on an engine with ``kv_dtype="fp8"`` (prompts and helpers imported): every prefill
chunk runs csrc/kernels/prefill_paged_kv8.hip.  The kernel route against the gather-and-dequantise route of the same
engine (both read the same quantised cache: row cosine > 0.99, the criterion of ``test_routes_hip_and_gather_agree``),
and the accounting of a prefix hit with the shared blocks' codes AND scales bitwise unchanged.
"""
import pytest
import torch

from mxllm.models import Llama, get_config
from mxllm.serve.engine import SamplingParams
from tests.test_prefix_cache_gpu import LONG, NEW, POOL, TAILED, chunked_logits, cos_rows, engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model(gpu):
    return Llama(get_config("tiny-d128"), device=gpu, seed=9).eval()


@pytest.mark.parametrize("chunk", [256, 100])
def test_chunked_prefill_kernel_and_gather_routes_agree(model, monkeypatch, chunk):
    got = {}
    for route in ("hip", "gather"):
        monkeypatch.setenv("MXLLM_PREFILL_PAGED", route)
        got[route] = chunked_logits(engine(model, prefill_chunk=chunk, kv_dtype="fp8"), chunk)
    cos = cos_rows(got["hip"], got["gather"])
    assert float(cos.min()) > 0.99, cos


@pytest.mark.parametrize("use_graphs", [False, True], ids=["eager", "graphed"])
def test_prefix_hit_accounting_and_shared_blocks_untouched(model, use_graphs):
    eng = engine(model, use_graphs=use_graphs, prefix_cache=True, kv_dtype="fp8")
    kv = eng.kv
    sp = lambda: SamplingParams(max_new_tokens=NEW)
    r1 = eng.generate([LONG], max_new_tokens=NEW, return_requests=True)[0]
    assert r1.cached_tokens == 0 and len(r1.output) == NEW
    first = kv.match_prefix(LONG)
    assert len(first) == 2 and kv.evictable_blocks == 2
    pools = [*kv.k, *kv.v, *kv.k_scale, *kv.v_scale]
    snap = [p[first].clone() for p in pools]

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
    assert eng.stats()["prefix_cache_hit_tokens"] == 1024
    for p0, p in zip(snap, pools):  # shared blocks are never written: codes and scales
        assert torch.equal(p[first].view(torch.uint8), p0.view(torch.uint8))
    assert not any(kv.ref) and set(kv.owned) <= {eng.scratch_slot}
    assert kv.free_blocks + kv.evictable_blocks == POOL // 256
