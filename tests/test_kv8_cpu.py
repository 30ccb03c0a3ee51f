"""CPU tests of the fp8 (kv8) KV cache: the codec (mxllm/serve/quant.py), KVCache and Engine in fp8
mode on their CPU paths, the server's option, and the input conditions of tests/test_kv8_gpu.py."""
import math

import pytest
import torch

from mxllm.serve.quant import kv8_dequantize, kv8_quantize
from tests import _kv8 as K

BF16, F32, U8 = K.BF16, K.F32, K.U8


def _row(vals):
    x = torch.zeros(1, 128, dtype=BF16)
    x[0, :len(vals)] = torch.tensor(vals, dtype=F32).to(BF16)
    return x


# =========================================================================== codec
def test_every_code_decodes_as_float8_e4m3fn():
    v = K.e4m3_values()
    codes = torch.arange(256, dtype=torch.int16).to(U8).view(2, 128)
    for e in (0, -100, 17, 120):
        s = torch.full((2,), 2.0 ** e)
        got, want = kv8_dequantize(codes, s).float().view(-1), v * 2.0 ** e
        fin = torch.isfinite(v)
        assert fin.sum() == 254 and got[~fin].isnan().all()
        assert torch.equal(got[fin], want[fin]), e  # bf16 holds every finite code times the scale exactly
    # the format's own table: sign, 4 exponent bits (bias 7), 3 mantissa bits, subnormals below 2^-6
    c = torch.arange(128)
    e, m = (c >> 3) & 0xF, (c & 7).double()
    tab = torch.where(e == 0, m / 8 * 2.0 ** -6, (1 + m / 8) * torch.exp2(e.double() - 7))
    assert torch.equal(v[:127].double(), tab[:127]) and torch.equal(v[128:255].double(), -tab[:127])


def test_scale_rule():
    x = K.random_rows(torch.Generator().manual_seed(1), 4096, -60, 60)
    codes, scale = kv8_quantize(x)
    assert codes.dtype == U8 and scale.dtype == F32 and tuple(scale.shape) == (4096,)
    amax = x.float().abs().amax(-1)
    nz = amax > 0
    ratio = amax[nz].double() / scale[nz].double()
    assert (ratio > 224).all() and (ratio <= 448).all(), (ratio.min(), ratio.max())
    assert ((scale.view(torch.int32) & 0x7FFFFF) == 0).all() and (scale > 0).all()  # powers of two
    assert (kv8_quantize(x[0:1])[1] == 2.0 ** -8).all()   # amax 1 -> 256 in code units
    assert (kv8_quantize(x[2:3])[1] == 2.0 ** -8).all()   # amax 1.75 -> 448, still the smaller scale
    assert (kv8_quantize(x[3:4])[1] == 2.0 ** -7).all()   # the next bf16 above 1.75
    assert scale[1] == 1.0 and not codes[1].any()           # a zero row: scale 1, codes 0
    assert not ((codes & 0x7F) == 0x7F).any()               # the NaN codes are never produced
    tiny = _row([2.0 ** -120, -2.0 ** -126])
    assert kv8_quantize(tiny)[1].item() == 2.0 ** -100      # the exponent clamp


def test_rounding_and_subnormals():
    # amax 256 -> scale 1: the values are code units
    codes, scale = kv8_quantize(_row([256, 17, 19, 2 ** -10, 3 * 2 ** -10, -17, 2 ** -9, 0.0, -2 ** -10]))
    assert scale.item() == 1.0
    got = kv8_dequantize(codes, scale).float()[0, :9].tolist()
    assert got == [256, 16, 20, 0, 2 ** -8, -16, 2 ** -9, 0, 0], got  # ties to even; subnormals and zero kept
    assert codes[0, 6].item() == 0x01 and codes[0, 7].item() == 0x00


def test_dequantised_rows_are_bf16_rows():
    x = K.random_rows(torch.Generator().manual_seed(2), 512)
    codes, scale = kv8_quantize(x)
    f32 = codes.view(torch.float8_e4m3fn).float() * scale[:, None]
    dq = kv8_dequantize(codes, scale)
    assert torch.equal(dq.float(), f32)  # no rounding in the bf16 conversion
    assert torch.equal(dq.float().to(BF16), dq)
    # half an ulp of the top binade (32 code units) bounds the rounding error of a row
    assert ((dq.float() - x.float()).abs().amax(-1) <= 16 * scale).all()
    with pytest.raises(ValueError):
        kv8_quantize(x[:, :64])
    with pytest.raises(ValueError):
        kv8_quantize(x.float())


def test_onehot_keys_quantise_exactly():
    """The input conditions of the GPU one-hot test, asserted inside the builder."""
    c = K.onehot_kv8((128, 6, 2, True, True))
    dead = c["ks"].isnan()
    assert dead.any() and (c["kq"][dead] == K.NAN_CODE).all() and (c["vq"][dead] == K.NAN_CODE).all()
    assert c["vs"][dead].isnan().all() and not c["vs"][~dead].isnan().any()


def test_fp32_model_error_at_quantised_inputs_within_measured_bound():
    from tests.test_kv8_gpu import check_measure

    check_measure()


# =========================================================================== ops on the CPU
def test_decode_attention_kv8_cpu_reference():
    """decode_attention with scale pools: appends the codec's rows and attends over the dequantised
    cache (the existing fp32 expression), contiguous and paged."""
    from mxllm.ops import decode as dops
    from mxllm.ops import reference as ref

    g = torch.Generator().manual_seed(5)
    Hq, Hkv, D, B = 8, 2, 128, 2
    cos, sin = ref.rope_tables(512, D, 500000.0, None)
    for bt in (None, torch.tensor([[3, 1], [0, 2]], dtype=torch.int32)):
        n0, rows = (4, 256) if bt is not None else (2, 512)
        k16, v16 = (torch.randn(n0, Hkv, rows, D, generator=g).to(BF16) for _ in range(2))
        (kq, ks), (vq, vs) = kv8_quantize(k16), kv8_quantize(v16)
        kdq, vdq = kv8_dequantize(kq, ks), kv8_dequantize(vq, vs)
        qkv = torch.randn(B, (Hq + 2 * Hkv) * D, generator=g).to(BF16)
        pos, slots = torch.tensor([300, 7], dtype=torch.int32), torch.tensor([1, 0], dtype=torch.int32)
        out8 = dops.decode_attention(qkv, cos, sin, kq, vq, pos, slots, Hq, Hkv, D, 512, bt, k_scale=ks, v_scale=vs)
        out16 = dops.decode_attention(qkv, cos, sin, kdq, vdq, pos, slots, Hq, Hkv, D, 512, bt)
        # the appended rows: the codec of what the bf16 path stored
        assert torch.equal(kv8_dequantize(kq, ks), kv8_dequantize(*kv8_quantize(kdq)))
        assert torch.equal(kv8_dequantize(vq, vs), kv8_dequantize(*kv8_quantize(vdq)))
        assert torch.nn.functional.cosine_similarity(out8.float(), out16.float(), dim=1).min() > 0.999
    with pytest.raises(ValueError):
        dops.decode_attention(qkv, cos, sin, kq, vq, pos, slots, Hq, Hkv, D, 512, None, k_scale=ks)
    with pytest.raises(ValueError):
        dops.decode_attention(qkv, cos, sin, kq, vq, pos, slots, 16, 4, 64, 512, None, k_scale=ks, v_scale=vs)


# =========================================================================== KVCache
@pytest.mark.parametrize("paged", [False, True])
def test_kvcache_fp8_write_gather(paged):
    from mxllm.serve.kvcache import KVCache

    g = torch.Generator().manual_seed(7)
    kv = KVCache(2, 2, 128, BF16, torch.device("cpu"), 3, 1024, pool_tokens=2048 if paged else None, kv_dtype="fp8")
    ref = KVCache(2, 2, 128, BF16, torch.device("cpu"), 3, 1024, pool_tokens=2048 if paged else None)
    assert kv.k[0].dtype == U8 and kv.k[0].shape == ref.k[0].shape and kv.k_scale[0].shape == ref.k[0].shape[:3]
    assert kv.nbytes() * 256 == ref.nbytes() * 132 and kv.n_blocks == ref.n_blocks
    if paged:  # non-consecutive blocks for slot 1: slot 0 takes and returns blocks in between
        for c in (kv, ref):
            c.reserve(0, 256)
            c.reserve(1, 256)
            c.release(0)
            c.free.sort(reverse=True)
            c.reserve(1, 700)
            assert c.owned[1] != list(range(c.owned[1][0], c.owned[1][0] + 3))
    S = 700  # two full blocks and a partial one
    k, v = (torch.randn(2, S, 128, generator=g).to(BF16) for _ in range(2))
    kv.write(1, 1, k, v)
    kq, ks, vq, vs = kv.gather_raw(1, 1, S)
    for got, want in ((kq, kv8_quantize(k)[0]), (ks, kv8_quantize(k)[1]), (vq, kv8_quantize(v)[0]), (vs, kv8_quantize(v)[1])):
        assert torch.equal(got, want)
    gk, gv = kv.gather(1, 1, S)
    assert gk.dtype == BF16 and torch.equal(gk, kv8_dequantize(*kv8_quantize(k))) and torch.equal(gv, kv8_dequantize(*kv8_quantize(v)))
    assert not kv.k[0].any() and (kv.k_scale[0] == 1).all()  # the other layer untouched
    with pytest.raises(ValueError):
        KVCache(1, 2, 64, BF16, torch.device("cpu"), 2, 256, kv_dtype="fp8")
    with pytest.raises(ValueError):
        KVCache(1, 2, 128, BF16, torch.device("cpu"), 2, 256, kv_dtype="int8")


# =========================================================================== Engine
def test_engine_fp8_kv_cache_cpu(monkeypatch):
    """Prefill plus 3 decode steps for two slots: after prefill the fp8 engine's cache is the codec of the
    bf16 engine's rows in every layer (prefill attends over the fresh bf16 K/V), and decoding runs."""
    from mxllm.models import Llama, get_config
    from mxllm.serve.engine import Engine

    cfg = get_config("tiny-d128")
    mk = lambda **kw: Engine(Llama(cfg, seed=3, dtype=BF16).eval(), max_batch=2, max_seq=512, kv_pool_tokens=1024, **kw)  # noqa: E731
    ref, eng = mk(), mk(kv_dtype="fp8")
    assert ref.kv_dtype == "bf16" and not ref.kv.fp8 and eng.kv.fp8
    prompts = [list(range(3, 60)), [7, 8, 9] * 90]
    l_ref, l_8 = ref.prefill_batch([0, 1], prompts), eng.prefill_batch([0, 1], prompts)
    assert torch.equal(l_ref, l_8)
    for layer in range(cfg.n_layers):
        for slot, p in enumerate(prompts):
            k, v = ref.kv.gather(layer, slot, len(p))
            kq, ks, vq, vs = eng.kv.gather_raw(layer, slot, len(p))
            assert torch.equal(kq, kv8_quantize(k)[0]) and torch.equal(ks, kv8_quantize(k)[1])
            assert torch.equal(vq, kv8_quantize(v)[0]) and torch.equal(vs, kv8_quantize(v)[1])
    tok = torch.tensor([5, 9])
    for step in range(3):
        d_ref, d_8 = ref.decode([0, 1], tok), eng.decode([0, 1], tok)
        assert torch.nn.functional.cosine_similarity(d_8.float(), d_ref.float(), dim=1).min() > 0.99
        tok = d_ref.float().argmax(-1)
    assert eng.lens[:2] == [60, 273]
    k, _ = ref.kv.gather(0, 0, 58)  # layer 0's first appended row: the same qkv in both engines
    assert torch.equal(eng.kv.gather_raw(0, 0, 58)[0][:, 57], kv8_quantize(k[:, 57])[0])
    st = eng.stats()
    assert st["kv_cache_dtype"] == "fp8" and st["kv_cache_bytes"] == eng.kv.nbytes()
    # the environment default and the refusals
    monkeypatch.setenv("MXLLM_KV_CACHE", "fp8")
    assert mk().kv.fp8 and not mk(kv_dtype="bf16").kv.fp8
    monkeypatch.setenv("MXLLM_KV_CACHE", "int4")
    with pytest.raises(ValueError, match="MXLLM_KV_CACHE"):
        mk()
    monkeypatch.delenv("MXLLM_KV_CACHE")
    with pytest.raises(ValueError, match="head_dim 128"):
        Engine(Llama(get_config("tiny"), seed=0).eval(), max_batch=2, max_seq=256, kv_dtype="fp8")


# =========================================================================== server option
def test_server_kv_cache_option(monkeypatch):
    from mxllm.serve import server

    monkeypatch.delenv("MXLLM_KV_CACHE", raising=False)
    assert server.parse_args([]).kv_cache == "bf16"
    assert server.parse_args(["--kv-cache", "fp8"]).kv_cache == "fp8"
    monkeypatch.setenv("MXLLM_KV_CACHE", "fp8")
    assert server.parse_args([]).kv_cache == "fp8"
    assert server.parse_args(["--kv-cache", "bf16"]).kv_cache == "bf16"
    with pytest.raises(SystemExit):
        server.parse_args(["--kv-cache", "int4"])


def test_local_engine_kv_cache_keyword(monkeypatch):
    from mxllm.serve import client, local

    monkeypatch.setattr(client, "_LOCAL", {})
    eng = local.ensure_local_engine("kv8-test", "cpu", engine_model="tiny-d128", max_batch=2, max_seq=512,
                                    kv_cache="fp8")[0]
    assert eng.kv.fp8 and math.isclose(eng.kv.nbytes() / eng.kv.k[0].numel() / 2 / len(eng.kv.k), 132 / 128)
