"""GPU tests of the fp8 (kv8) KV cache: csrc/kernels/decode.hip kv8_quant_rows, rope_append_kv8 and
decode_attn_kv8, and the engine's fp8 cache mode.

The row format (mxllm/serve/quant.py) has power-of-two scales, so the dequantised cache is a bf16
cache and the exact tests of tests/test_decode_exact_gpu.py carry over: codes and scales equal the CPU
codec bit for bit, one-hot attention returns the dequantised V row bit for bit, and the Gaussian
parity bound is the bf16 kernel's (``P.DECODE_O_MFMA``), against fp64 on the dequantised cache.
Dead rows hold the NaN code 0x7F and NaN scales: one of them read anywhere poisons the output.

``python -m tests.test_kv8_gpu`` (no GPU) prints the error of the fp32 model of the documented
algorithm against fp64 at the quantised Gaussian inputs and asserts that it stays within
``P.DECODE_O_MFMA_MEASURED``, the measurement that ``P.DECODE_O_MFMA`` doubles.
"""
import math

import pytest
import torch

from mxllm.serve.quant import kv8_dequantize, kv8_quantize
from tests import _kv8 as K
from tests import _parity as P
from tests import test_decode_exact_gpu as X
from tests._parity import assert_exact, assert_parity

pytestmark = pytest.mark.gpu

BF16, F32, F64, I32, U8 = K.BF16, K.F32, K.F64, K.I32, K.U8
bits = X.bits


def _ops():
    from mxllm.ops import native

    return native()


# =========================================================================== 1. kv8_quant_rows
@pytest.mark.parametrize("R", [1, 3, 64, 257])
def test_kv8_quant_rows_equals_codec(gpu, R):
    x = K.random_rows(X._gen(3100 + R), R)
    codes, scale = kv8_quantize(x)
    wide = torch.zeros(R, 136, dtype=BF16)
    wide[:, :128] = x
    for name, inp in (("contiguous", x.to(gpu)), ("strided", wide.to(gpu)[:, :128])):
        q, s = _ops().kv8_quant_rows(inp)
        assert q.dtype == U8 and s.dtype == F32 and tuple(s.shape) == (R,)
        assert_exact(bits(s.cpu()), bits(scale), f"R{R} {name}: scales")
        assert_exact(q.cpu(), codes, f"R{R} {name}: codes")


# =========================================================================== 2. rope_append_kv8
APPEND_CASES = [(hq, hkv, B, paged) for hq, hkv in X.GROUPS_128 for B in (1, 5) for paged in (False, True)]


def append_id(c):
    return f"Hq{c[0]}-Hkv{c[1]}-B{c[2]}-{'paged' if c[3] else 'contig'}"


@pytest.mark.parametrize("case", APPEND_CASES, ids=append_id)
def test_rope_append_kv8_whole_pools(gpu, case):
    """Every row of the four pools: the appended rows hold the codec of what rope_append stores (K; at
    position 0 and for V the codec of the input itself), every other row keeps its fill pattern; q is
    rope_append's q."""
    Hq, Hkv, B, paged = case
    D, S = 128, 300
    g = X._gen(3300 + 16 * Hq + Hkv + 2 * B + paged)
    c = X.append_layout(g, B, Hkv, D, S, paged, True)
    qkv = torch.randn(B, (Hq + 2 * Hkv) * D, generator=g).to(BF16)
    qkv.view(B, -1, D)[:, :, 0] *= torch.exp2(torch.randint(-20, 20, (B, Hq + 2 * Hkv), generator=g).float()).to(BF16)
    n0, _, rows, _ = c["kc"].shape
    fill_q = [torch.randint(0, 256, (n0, Hkv, rows, D), generator=g, dtype=torch.int16).to(U8) for _ in range(2)]
    fill_s = [torch.randint(-2 ** 31, 2 ** 31, (n0, Hkv, rows), generator=g, dtype=torch.int64).to(I32).view(F32)
              for _ in range(2)]
    dv = {k: X._dev(c[k], gpu) for k in ("cos", "sin", "pos", "slots", "bt")}
    ops = _ops()
    kc, vc = c["kc"].to(gpu, copy=True), c["vc"].to(gpu, copy=True)
    q_ref = ops.rope_append(qkv.to(gpu), dv["cos"], dv["sin"], dv["pos"], dv["slots"], kc, vc, Hq, Hkv, D, dv["bt"])
    kc = kc.cpu()
    kq, ks, vq, vs = (t.to(gpu, copy=True) for t in (fill_q[0], fill_s[0], fill_q[1], fill_s[1]))
    q = ops.rope_append_kv8(qkv.to(gpu), dv["cos"], dv["sin"], dv["pos"], dv["slots"], kq, ks, vq, vs, Hq, Hkv,
                            dv["bt"])
    assert_exact(bits(q.cpu()), bits(q_ref.cpu()), "q")
    want = [t.clone() for t in (fill_q[0], fill_s[0], fill_q[1], fill_s[1])]
    x = qkv.view(B, Hq + 2 * Hkv, D)
    for b in range(B):
        i0, r = X.kv_place(c["bt"], rows, int(c["slots"][b]), int(c["pos"][b]))
        k_row = kc[i0, :, r]  # what rope_append stores
        if int(c["pos"][b]) == 0:
            assert_exact(bits(k_row), bits(x[b, Hq:Hq + Hkv]), "rope_append at position 0 stores the input")
        want[0][i0, :, r], want[1][i0, :, r] = kv8_quantize(k_row)
        want[2][i0, :, r], want[3][i0, :, r] = kv8_quantize(x[b, Hq + Hkv:])
    for name, out, w in zip(("k_codes", "k_scale", "v_codes", "v_scale"), (kq, ks, vq, vs), want):
        o = out.cpu()
        assert_exact(bits(o) if o.dtype == F32 else o, bits(w) if w.dtype == F32 else w,
                     f"{append_id(case)}: {name} (appended rows and every other row)")


# =========================================================================== 3. one-hot exactness
ONEHOT_CASES = [c for c in X.ONEHOT_CASES if c[0] == 128]


@pytest.mark.parametrize("case", ONEHOT_CASES, ids=X.onehot_id)
def test_decode_attn_kv8_onehot_exact(gpu, case):
    c = K.onehot_kv8(case)
    X.assert_onehot_conditions(c)
    out = K.run_attn_kv8(_ops(), c, gpu)
    assert_exact(out.cpu(), c["want"], X.onehot_id(case))


# =========================================================================== 4. empty lengths, refusals
@pytest.mark.parametrize("lens", X.EMPTY_LENS, ids=lambda l: "lens" + "_".join(map(str, l)))
def test_decode_attn_kv8_empty_rows(gpu, lens):
    c = K.onehot_kv8((128, 8, 2, False, False), tuple(lens))
    out = K.run_attn_kv8(_ops(), c, gpu).cpu()
    assert_exact(out, c["want"], f"lens {lens}")
    for b, L in enumerate(lens):
        if L == 0:
            assert not bits(out[b]).any(), f"row {b} (no keys) is not all zero"


def _pools(g, n0, Hkv, rows, D, dev):
    kq = torch.randint(0, 127, (n0, Hkv, rows, D), generator=g, dtype=torch.int16).to(U8).to(dev)
    ks = torch.exp2(torch.randint(-8, 8, (n0, Hkv, rows), generator=g).float()).to(dev)
    return kq, ks


def test_decode_attn_kv8_refusals(gpu):
    ops, g = _ops(), X._gen(6)
    lens = torch.tensor([5, 300], dtype=I32, device=gpu)

    def refused(q, kq, ks, vq, vs, max_len, bt=None):
        before = [t.clone() for t in (kq, ks, vq, vs)]
        with pytest.raises(RuntimeError):
            ops.decode_attn_kv8(q, kq, ks, vq, vs, lens, None, max_len, 1.0, 0, bt)
        for t, b in zip((kq, ks, vq, vs), before):
            assert torch.equal(t.view(torch.uint8), b.view(torch.uint8)), "a refused call wrote to a pool"

    for Hq, Hkv in X.REFUSED_HEADS:  # group size 17; Hq % Hkv != 0
        q = torch.randn(2, Hq, 128, generator=g).to(BF16).to(gpu)
        kq, ks = _pools(g, 2, Hkv, 300, 128, gpu)
        refused(q, kq, ks, kq, ks, 300)
    q = torch.randn(2, 8, 128, generator=g).to(BF16).to(gpu)
    for blk in (128, 320):  # a paged cache whose block size is no multiple of the 256-key split
        kq, ks = _pools(g, 8, 2, blk, 128, gpu)
        refused(q, kq, ks, kq, ks, 4 * blk, torch.arange(8, dtype=I32).view(2, 4).to(gpu))
    kq64, ks64 = _pools(g, 2, 2, 300, 64, gpu)  # head_dim 64
    refused(torch.randn(2, 8, 64, generator=g).to(BF16).to(gpu), kq64, ks64, kq64, ks64, 300)
    refused(q, kq64, ks64, kq64, ks64, 300)
    kq, ks = _pools(g, 2, 2, 300, 128, gpu)
    ops.decode_attn_kv8(q, kq, ks, kq, ks, lens, None, 300, 1.0, 0, None)  # the accepted form of the calls below
    refused(q, kq.to(BF16), ks, kq, ks, 300)          # bf16 pools given as codes
    refused(q, kq, ks, kq.view(torch.int8), ks, 300)  # int8 codes
    refused(q, kq, ks.to(BF16), kq, ks, 300)          # bf16 scales
    refused(q, kq, ks, kq, ks.double(), 300)          # f64 scales
    refused(q.float(), kq, ks, kq, ks, 300)           # f32 q
    refused(q, kq, ks[:, :, :299], kq, ks, 300)       # scale pool of another shape
    # rope_append_kv8: the same pool checks, and nothing written on a refusal
    qkv = torch.randn(2, 12 * 128, generator=g).to(BF16).to(gpu)
    cos, sin = (t.to(gpu) for t in X.ref.rope_tables(300, 128, X.ROPE_THETA, None))
    pos = torch.tensor([0, 7], dtype=I32, device=gpu)
    for bad in ((kq.to(BF16), ks, kq, ks), (kq, ks.to(BF16), kq, ks), (kq64, ks64, kq64, ks64)):
        before = [t.clone() for t in bad]
        with pytest.raises(RuntimeError):
            ops.rope_append_kv8(qkv, cos, sin, pos, None, *bad, 8, 2, None)
        for t, b in zip(bad, before):
            assert torch.equal(t.view(torch.uint8), b.view(torch.uint8))


# =========================================================================== 5. Gaussian parity
GAUSS_CASES = [c for c in X.GAUSS_CASES if c[0] == 128]


@pytest.mark.parametrize("case", GAUSS_CASES, ids=X.gauss_id)
def test_decode_attn_kv8_gaussian_parity(gpu, case):
    """Against fp64 on the dequantised cache, under the bf16 kernel's bound; the bf16 kernel on the
    dequantised cache is held to the same bound, so a difference between the two kernels shows."""
    D = 128
    c = K.gauss_kv8(case)
    r64 = X.gauss_reference(c, F64, D)
    scale, max_len = 1.0 / math.sqrt(D), max(X.GAUSS_LENS)
    out8 = K.run_attn_kv8(_ops(), c, gpu, scale=scale, max_len=max_len).cpu()
    out16 = X.run_attn(_ops(), c, gpu, scale=scale, max_len=max_len).cpu()
    d = (out8.double() - out16.double()).abs().max().item()
    print(f"{X.gauss_id(case)}: max |decode_attn_kv8 - decode_attn on the dequantised cache| = {d:.3g}")
    assert_parity(out8.view(-1, D), r64.view(-1, D), P.DECODE_O_MFMA, name=f"decode_attn_kv8 {X.gauss_id(case)}")
    assert_parity(out16.view(-1, D), r64.view(-1, D), P.DECODE_O_MFMA,
                  name=f"decode_attn on the dequantised cache {X.gauss_id(case)}")


# =========================================================================== 6. engine
def _engines(gpu, monkeypatch, use_graphs):
    from mxllm.models import Llama, get_config
    from mxllm.serve import engine as E

    monkeypatch.setattr(E, "_NORM_FUSED", False)
    monkeypatch.setattr(E, "_ROPE_FUSED", False)
    cfg = get_config("tiny-d128")
    assert cfg.n_layers == 2
    mk = lambda kv: E.Engine(Llama(cfg, device=gpu, seed=9).eval(), max_batch=2, max_seq=512, use_graphs=use_graphs,
                             kv_pool_tokens=1024, kv_dtype=kv)  # noqa: E731
    return cfg, mk("bf16"), mk("fp8")


@pytest.mark.parametrize("use_graphs", [False, True], ids=["eager", "graphed"])
def test_engine_fp8_kv_cache(gpu, monkeypatch, use_graphs):
    cfg, ref, eng = _engines(gpu, monkeypatch, use_graphs)
    assert eng.kv.fp8 and eng.kv.k[0].dtype == U8 and eng.stats()["kv_cache_dtype"] == "fp8"
    assert eng.kv.nbytes() * 256 == ref.kv.nbytes() * 132
    g = X._gen(41)
    prompts = [torch.randint(3, cfg.vocab_size, (n,), generator=g).tolist() for n in (57, 300)]
    l_ref, l_8 = ref.prefill_batch([0, 1], prompts), eng.prefill_batch([0, 1], prompts)
    assert torch.equal(l_ref, l_8)  # prefill attends over the fresh bf16 K/V: only the cache write differs

    def check_rows(layer, slot, a, b):
        k, v = ref.kv.gather(layer, slot, b)
        kq, ks, vq, vs = (t.cpu() for t in eng.kv.gather_raw(layer, slot, b))
        for name, x, cd, sc in (("K", k, kq, ks), ("V", v, vq, vs)):
            wq, ws = kv8_quantize(x[:, a:b].cpu())
            assert_exact(cd[:, a:b], wq, f"layer {layer} slot {slot} rows {a}..{b}: {name} codes")
            assert_exact(bits(sc[:, a:b]), bits(ws), f"layer {layer} slot {slot} rows {a}..{b}: {name} scales")

    for layer in range(cfg.n_layers):
        for slot, p in enumerate(prompts):
            check_rows(layer, slot, 0, len(p))
    tok = torch.tensor([5, 9])
    d_ref, d_8 = ref.decode([0, 1], tok), eng.decode([0, 1], tok)
    for slot, p in enumerate(prompts):
        check_rows(0, slot, len(p), len(p) + 1)  # layer 0's appended row: the same qkv in both engines
    cos = torch.nn.functional.cosine_similarity(d_8.float(), d_ref.float(), dim=1)
    assert (cos > 0.99).all(), cos.tolist()
    for s in (0, 1):
        eng.kv.release(s)
        eng.lens[s] = 0
    out = eng.generate(prompts, max_new_tokens=8)
    assert all(len(o) == 8 for o in out)


def test_engine_fp8_kv_cache_with_fp8_weights(gpu):
    from mxllm.models import Llama, get_config
    from mxllm.serve.engine import Engine
    from mxllm.serve.quant import quantize_model_fp8_

    m8 = Llama(get_config("tiny-d128"), device=gpu, seed=9).eval()
    assert quantize_model_fp8_(m8) > 0
    eng = Engine(m8, max_batch=2, max_seq=512, kv_pool_tokens=1024, kv_dtype="fp8")
    out = eng.generate([list(range(3, 60)), [1, 2, 3]], max_new_tokens=8)
    assert all(len(o) == 8 for o in out)


# =========================================================================== yardstick
def measure():
    """Error of the fp32 model of the documented algorithm (X.attn_model) against fp64 at the quantised
    Gaussian inputs above: ``DECODE_O_MFMA`` carries over when it stays within ``DECODE_O_MFMA_MEASURED``."""
    acc = {}
    for case in GAUSS_CASES:
        c = K.gauss_kv8(case)
        y32, r64 = X.gauss_reference(c, F32, 128), X.gauss_reference(c, F64, 128)
        X._meas(acc, "DECODE_O_MFMA", y32.view(-1, 128), r64.view(-1, 128))
    return acc["DECODE_O_MFMA"]


def check_measure():
    rel, ab = measure()
    print(f"kv8 DECODE_O_MFMA_MEASURED = ({rel:.3g}, {ab:.3g}); bf16 cache: {P.DECODE_O_MFMA_MEASURED}")
    # the constants are written with three significant digits
    assert float(f"{rel:.3g}") <= P.DECODE_O_MFMA_MEASURED[0] and float(f"{ab:.3g}") <= P.DECODE_O_MFMA_MEASURED[1]


if __name__ == "__main__":
    check_measure()
