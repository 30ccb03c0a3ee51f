"""Helpers of the MXFP4 weight tests: tests/test_mxfp4_cpu.py and tests/test_mxfp4_gpu.py.

The CPU codec (mxllm/serve/quant.py quantize_mxfp4 / dequantize_mxfp4) is the reference of every
expectation.  Each check is a function ``check_*(run, dev)``: the GPU test calls it with the HIP op,
the CPU test with the Python reference -- which proves without a GPU that the inputs are valid and
that the reference itself passes.  The bounds are arguments: the constants live in
tests/test_mxfp4_gpu.py.
"""
import functools
import math

import torch

from mxllm.serve.quant import MXFP4_GRID, W4Linear, dequantize_mxfp4, quantize_mxfp4, quantize_model_mxfp4_
from tests import test_skinny_exact_gpu as SK
from tests._parity import assert_exact, assert_parity

BF16, F32, F64, U8 = torch.bfloat16, torch.float32, torch.float64, torch.uint8
EXACT_LIMIT = 2 ** 24
bits, strided = SK.bits, SK.strided


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def pack(code):
    """e2m1 codes [N, K] (0..15) -> bytes [N, K/2], the even k in the low nibble."""
    code = code.to(U8)
    return (code[:, 0::2] | (code[:, 1::2] << 4)).contiguous()


# =========================================================================== every code x every scale
def every_code_case():
    """codes [254, 32], scales [254, 2]: channel n carries scale bytes n + 1 (block 0) and 254 - n
    (block 1); in either block every one of the 16 codes stands once in a low and once in a high nibble."""
    i = torch.arange(16)
    b0 = i | ((15 - i) << 4)
    b1 = ((i + 5) % 16) | (((3 * i + 1) % 16) << 4)
    for b in (b0, b1):
        assert sorted((b & 15).tolist()) == sorted((b >> 4).tolist()) == list(range(16))
    codes = torch.cat([b0, b1]).to(U8).repeat(254, 1)
    n = torch.arange(254)
    scales = torch.stack([n + 1, 254 - n], 1).to(U8)
    assert int(scales.min()) == 1 and int(scales.max()) == 254
    return codes, scales


def check_every_code(dequant, dev):
    """``dequant(codes, scales) -> bf16 [N, K]``, bitwise the reference (which is its own bf16 rounding
    wherever it is finite; 2 * 2^127 and above are inf in f32 and bf16 alike)."""
    codes, scales = every_code_case()
    ref = dequantize_mxfp4(codes, scales)
    want = ref.to(BF16)
    fin = torch.isfinite(ref)
    assert torch.equal(want.float()[fin], ref[fin]) and int((~fin).sum()) > 0
    got = dequant(codes.to(dev), scales.to(dev)).cpu()
    if not torch.equal(bits(got), bits(want)):
        bad = (bits(got) != bits(want)).nonzero()
        rows = sorted({int(r) for r in bad[:, 0]})
        first = [(int(r), int(c), hex(int(bits(got)[r, c]) & 0xFFFF), hex(int(bits(want)[r, c]) & 0xFFFF))
                 for r, c in bad[:12]]
        print(f"every-code mismatches: {len(bad)} elements; scale bytes of block 0 in rows "
              f"{[r + 1 for r in rows][:40]}; first (row, column, got, expected) {first}")
    assert_exact(bits(got), bits(want), "w4_dequant: 16 codes x scale bytes 1..254 x both nibbles")


# =========================================================================== w4_linear operands
@functools.lru_cache(maxsize=4)
def int_weight(N, K):
    """Magnitude codes 1..4 (0.5, 1, 1.5, 2) with random signs; scale bytes 125..129 drawn per (channel,
    block), so every output is tied to its own scales.  Every weight is an integer multiple of 2^-3."""
    g = _gen(4100 + N + K)
    code = torch.randint(1, 5, (N, K), generator=g) | (torch.randint(0, 2, (N, K), generator=g) << 3)
    scales = torch.randint(125, 130, (N, K // 32), generator=g).to(U8)
    return pack(code), scales


@functools.lru_cache(maxsize=4)
def gauss_weight(N, K):
    """The quantiser's output on Gaussian weights, a few rows scaled far up and down."""
    w = torch.randn(N, K, generator=_gen(4200 + N + K)) * 0.05
    w[1::7] *= 2.0 ** 9
    w[3::11] *= 2.0 ** -11
    return quantize_mxfp4(w)


@functools.lru_cache(maxsize=4)
def dense(kind, N, K):
    """The reference-decoded weight (f32; exactly a bf16 matrix)."""
    codes, scales = int_weight(N, K) if kind == "int" else gauss_weight(N, K)
    wd = dequantize_mxfp4(codes, scales)
    assert torch.equal(wd, wd.to(BF16).float())
    return wd


def linear_case(kind, M, N, K):
    """(x, codes, scales, fp64 product with the reference-decoded weights)."""
    codes, scales = int_weight(N, K) if kind == "int" else gauss_weight(N, K)
    wd = dense(kind, N, K)
    if kind == "int":
        x = SK.int_x(M, K, 4301 + M, lim=3)
        assert 4 * 4 * 3 * K < EXACT_LIMIT
        # in units of 2^-3 (the smallest weight, 0.5 * 2^-2) every partial sum is an integer below 2^24
        assert float((x.abs().double() @ wd.abs().double().t()).max()) * 8 < EXACT_LIMIT
        assert torch.equal(wd * 8, (wd * 8).round())
    else:
        x = SK.gauss_x(M, K, 4401 + M)
    return x, codes, scales, x.double() @ wd.double().t()


def check_linear(kind, M, N, K, run, dev, bound=None, xpad=24):
    """``run(x, codes, scales) -> y``; x row-strided with NaN pads and NaN rows past M."""
    name = f"w4 {kind} M{M} N{N} K{K}"
    x, codes, scales, r64 = linear_case(kind, M, N, K)
    y = run(strided(x, xpad, 3, dev), codes.to(dev), scales.to(dev)).cpu()
    if kind == "int":
        assert_exact(bits(y), bits(r64.to(F32).to(BF16)), name)
    else:
        assert_parity(y, r64, bound, name=name)
    return y


def check_fallback(M, N, K, run, dequant, dev, bound):
    """Calls the decode kernel does not take (more rows than stream_m, K % 512): w4_dequant bitwise, then
    the bf16 GEMM of those (exactly bf16) weights per element."""
    x, codes, scales, r64 = linear_case("gauss", M, N, K)
    got = dequant(codes.to(dev), scales.to(dev)).cpu()
    assert_exact(bits(got), bits(dense("gauss", N, K).to(BF16)), f"w4_dequant N{N} K{K}")
    y = run(strided(x, 24, 3, dev), codes.to(dev), scales.to(dev)).cpu()
    assert_parity(y, r64, bound, name=f"w4 fallback M{M} N{N} K{K}")
    return y


def reference_linear(x, codes, scales, stream_m=None):
    """The CPU path of W4Linear: the bf16 matmul with the reference-decoded weights."""
    return torch.matmul(x, dequantize_mxfp4(codes, scales).to(x.dtype).t())


def reference_dequant(codes, scales):
    return dequantize_mxfp4(codes, scales).to(BF16)


# =========================================================================== models
def quantized_pair(cfg, dev, seed=21, lora_r=0):
    """(m4, m16): a Llama with W4Linear projections, and the same model with each projection weight
    replaced by the bf16 dequantised one."""
    from mxllm.models import Llama

    m4 = Llama(cfg, device=dev, seed=seed, lora_r=lora_r).eval()
    m16 = Llama(cfg, device=dev, seed=seed, lora_r=lora_r).eval()
    assert quantize_model_mxfp4_(m4) > 0
    from mxllm.serve.engine import merge_lora_

    merge_lora_(m16)
    with torch.no_grad():
        for l4, l16 in zip(m4.layers, m16.layers):
            for name in ("wqkv", "wo", "wgu", "wd"):
                q = getattr(l4, name)
                assert isinstance(q, W4Linear), name
                getattr(l16, name).weight.copy_(dequantize_mxfp4(q.codes, q.scales).to(BF16))
    return m4, m16


@torch.no_grad()
def forward_f32(model, tokens) -> torch.Tensor:
    """Logits [S, V] of a bf16-weight Llama over one sequence, computed in fp32 on the CPU."""
    c = model.cfg
    S, D, Hq, Hkv = len(tokens), c.head_dim, c.n_heads, c.n_kv_heads
    f = lambda t: t.detach().cpu().float()  # noqa: E731
    cos, sin = f(model.rope_cos[:S]), f(model.rope_sin[:S])

    def norm(x, w):
        return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + c.norm_eps) * f(w)

    def rope(t):  # [S, H, D], rotate-half
        t1, t2 = t[..., :D // 2], t[..., D // 2:]
        cc, ss = cos[:, None, :], sin[:, None, :]
        return torch.cat([t1 * cc - t2 * ss, t2 * cc + t1 * ss], -1)

    h = f(model.tok_emb)[torch.tensor(tokens)]
    mask = torch.ones(S, S, dtype=torch.bool).tril()
    for layer in model.layers:
        qkv = norm(h, layer.attn_norm) @ f(layer.wqkv.weight).t()
        q = rope(qkv[:, :c.q_dim].view(S, Hq, D))
        k = rope(qkv[:, c.q_dim:c.q_dim + c.kv_dim].view(S, Hkv, D)).repeat_interleave(Hq // Hkv, 1)
        v = qkv[:, c.q_dim + c.kv_dim:].view(S, Hkv, D).repeat_interleave(Hq // Hkv, 1)
        sc = torch.einsum("shd,thd->hst", q, k) / math.sqrt(D)
        p = torch.softmax(sc.masked_fill(~mask, float("-inf")), -1)
        o = torch.einsum("hst,thd->shd", p, v).reshape(S, Hq * D)
        h = h + o @ f(layer.wo.weight).t()
        gu = norm(h, layer.mlp_norm) @ f(layer.wgu.weight).t()
        h = h + (torch.nn.functional.silu(gu[:, :c.ffn]) * gu[:, c.ffn:]) @ f(layer.wd.weight).t()
    return norm(h, model.final_norm) @ f(model.head_weight).t()


def check_engine(dev, expect_graphs):
    """Prefill of a 57-token prompt, then decode at batch 2 and at the 16-row bucket, of the mxfp4 engine
    and of the bf16 engine over the dequantised weights, per row against the fp32 CPU reference of that
    dequantised model.  The mxfp4 engine may be off by twice what the bf16 engine is (max abs over a
    row's logits): a different but valid summation order moves the result about as much as the baseline
    is off (tests/_parity.py).  Returns the (mxfp4, bf16) error pairs."""
    from mxllm.models import get_config
    from mxllm.serve.engine import Engine

    cfg = get_config("tiny-d128").replace(n_layers=4)
    m4, m16 = quantized_pair(cfg, dev)
    g = _gen(4500)
    pairs = []

    def compare(what, l4, l16, ref):
        e4, e16 = (l4.float().cpu() - ref).abs().max().item(), (l16.float().cpu() - ref).abs().max().item()
        print(f"{what}: mxfp4 engine {e4:.4g}, bf16 engine over the dequantised weights {e16:.4g} "
              f"(max |logit - fp32 reference|, reference max {ref.abs().max().item():.4g})")
        pairs.append((what, e4, e16))

    prompt = torch.randint(3, cfg.vocab_size, (57,), generator=g).tolist()
    engs = [Engine(m, max_batch=16, max_seq=128) for m in (m4, m16)]
    if expect_graphs:
        assert all(e.use_graphs for e in engs)
    compare("prefill 57", *(e.prefill(0, prompt) for e in engs), forward_f32(m16, prompt)[-1])
    for B in (2, 16):
        prompts = [torch.randint(3, cfg.vocab_size, (20 + i,), generator=g).tolist() for i in range(B)]
        tok = torch.randint(3, cfg.vocab_size, (B,), generator=g)
        out = []
        for e in engs:
            for i, p in enumerate(prompts):
                e.prefill(i, p)
            out.append(e.decode(list(range(B)), tok.to(dev))[:B])
        for i in range(B):
            ref = forward_f32(m16, prompts[i] + [int(tok[i])])[-1]
            compare(f"decode B{B} row {i}", out[0][i], out[1][i], ref)
    bad = [(w, e4, e16) for w, e4, e16 in pairs if not e4 <= 2 * e16]
    assert not bad, bad
    eng8 = Engine(m4, max_batch=2, max_seq=128, kv_dtype="fp8")
    outs = eng8.generate([prompt, [1, 2, 3]], max_new_tokens=6)
    assert [len(o) for o in outs] == [6, 6]
    return pairs
