"""CPU checks of op semantics: fused LoRA linear autograd vs a plain-PyTorch
formulation, Llama-3.1 RoPE frequencies vs the transformers implementation,
reference attention vs torch SDPA, AdamW reference vs torch.optim.AdamW."""
import math

import pytest
import torch

from mxllm.ops import reference as ref
from mxllm.ops.linear import lora_linear


def test_lora_linear_matches_plain_autograd():
    torch.manual_seed(0)
    T, K, splits, r, s = 7, 24, [16, 8, 8], 4, 2.0
    x = torch.randn(T, K, dtype=torch.float64, requires_grad=True)
    w = torch.randn(sum(splits), K, dtype=torch.float64)
    a = torch.randn(len(splits) * r, K, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(sum(splits), len(splits) * r, dtype=torch.float64)
    off = 0
    for i, n in enumerate(splits):
        b[off:off + n, i * r:(i + 1) * r] = torch.randn(n, r, dtype=torch.float64)
        off += n
    b.requires_grad_(True)
    y = lora_linear(x, w, a, b, splits, s)
    gy = torch.randn_like(y)
    y.backward(gy)
    gx, ga, gb = x.grad.clone(), a.grad.clone(), b.grad.clone()
    x.grad = a.grad = b.grad = None
    # plain: separate adapter per split
    outs, off = [], 0
    for i, n in enumerate(splits):
        bi = b[off:off + n, i * r:(i + 1) * r]
        ai = a[i * r:(i + 1) * r]
        outs.append(x @ w[off:off + n].t() + s * (x @ ai.t()) @ bi.t())
        off += n
    yr = torch.cat(outs, -1)
    yr.backward(gy)
    assert torch.allclose(y, yr, atol=1e-10)
    assert torch.allclose(gx, x.grad, atol=1e-10) and torch.allclose(ga, a.grad, atol=1e-10)
    mask = b.detach() != 0
    assert torch.allclose(gb[mask], b.grad[mask], atol=1e-10)
    assert (gb[~mask] == 0).all(), "off-diagonal blocks of B must get exactly zero gradient"


def test_llama3_rope_matches_transformers():
    tr = pytest.importorskip("transformers.modeling_rope_utils")
    from transformers import LlamaConfig

    cfg = LlamaConfig(rope_theta=500000.0, head_dim=128, hidden_size=8192, num_attention_heads=64,
                      max_position_embeddings=131072,
                      rope_scaling={"rope_type": "llama3", "factor": 8.0, "low_freq_factor": 1.0,
                                    "high_freq_factor": 4.0, "original_max_position_embeddings": 8192})
    fn = tr.ROPE_INIT_FUNCTIONS["llama3"]
    inv_hf, _ = fn(cfg, "cpu")
    mine = ref.llama3_inv_freq(128, 500000.0, {"factor": 8.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0,
                                               "original_max_position_embeddings": 8192})
    assert torch.allclose(inv_hf.double(), mine, rtol=1e-5, atol=0)


@pytest.mark.parametrize("S,Sk,causal", [(17, 17, True), (5, 23, True), (9, 9, False)])
def test_reference_attention_vs_sdpa(S, Sk, causal):
    torch.manual_seed(1)
    q = torch.randn(2, S, 4, 16)
    k = torch.randn(2, Sk, 2, 16)
    v = torch.randn(2, Sk, 2, 16)
    o = ref.attention(q, k, v, causal=causal)
    kk, vv = k.repeat_interleave(2, 2), v.repeat_interleave(2, 2)
    mask = None
    if causal:
        i = torch.arange(S).view(S, 1)
        j = torch.arange(Sk).view(1, Sk)
        mask = j <= i + (Sk - S)
    o2 = torch.nn.functional.scaled_dot_product_attention(q.transpose(1, 2), kk.transpose(1, 2), vv.transpose(1, 2),
                                                          attn_mask=mask).transpose(1, 2)
    assert torch.allclose(o, o2, atol=1e-5)


def test_adamw_reference_matches_torch():
    torch.manual_seed(2)
    p0 = torch.randn(50)
    grads = [torch.randn(50) for _ in range(4)]
    p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([p], lr=1e-2, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.1)
    mine, m, v = p0.clone(), torch.zeros(50), torch.zeros(50)
    for i, g in enumerate(grads):
        p.grad = g.clone()
        opt.step()
        ref.adamw_(mine, g, m, v, lr=1e-2, beta1=0.9, beta2=0.95, eps=1e-8, weight_decay=0.1, step=i + 1)
    assert torch.allclose(mine, p.detach(), atol=1e-6)


def test_flops_model():
    from mxllm.models import get_config

    c = get_config("llama3.1-70b")
    assert abs(c.n_params() / 1e9 - 70.55) < 0.05
    assert abs(get_config("llama3.1-8b").n_params() / 1e9 - 8.03) < 0.01
    assert math.isclose(c.train_flops_per_token(2048) / 1e9, 431.4, rel_tol=0.02)


def test_lora_augmented_gemm_matches_two_gemm_form():
    """One augmented GEMM per direction == the two-GEMM LoRA (forward, dx, dA, dB)."""
    from mxllm.models.llama import FusedLinear
    from mxllm.ops.linear import lora_linear

    torch.manual_seed(0)
    lin = FusedLinear(48, [40, 24], dtype=torch.float32, device="cpu", lora_r=4, lora_alpha=8.0, train_base=False)
    lin.reset_parameters(0.05, None)
    with torch.no_grad():
        for blk in lin.lora_b_blocks():
            blk.normal_(0, 0.1)
    lin.sync_adapter_()
    assert lin.augmented() and lin.pad == 64
    x = torch.randn(10, 48, requires_grad=True)
    dy = torch.randn(10, 64)
    y = lin(x)
    y.backward(dy)
    got = (y.detach(), x.grad.clone(), lin.lora_a.grad.clone(), lin.lora_b.grad.clone())
    x.grad = None
    lin.lora_a.grad = lin.lora_b.grad = None
    y2 = lora_linear(x, lin.weight, lin.lora_a, lin.lora_b, lin.splits, lin.scaling)
    y2.backward(dy)
    want = (y2.detach(), x.grad, lin.lora_a.grad, lin.lora_b.grad)
    for g, w in zip(got, want):
        torch.testing.assert_close(g, w, rtol=1e-5, atol=1e-5)
    # off-diagonal blocks of B get exactly zero gradient
    assert float(lin.lora_b.grad[:40, 4:].abs().max()) == 0.0


def test_lora_producer_written_tails_are_used():
    """``x_tail`` / ``dy_tail`` (the fused SwiGLU writes the LoRA tails): a padded x / dy whose
    pad columns already hold s x A^T / s dy B gives the same output and gradients as the
    recomputed tails; a wrong tail changes them (so it really is read, not recomputed); an
    unpadded tensor falls back to recomputing."""
    from mxllm.models.llama import FusedLinear

    torch.manual_seed(1)
    lin = FusedLinear(48, [40, 24], dtype=torch.float32, device="cpu", lora_r=4, lora_alpha=8.0, train_base=False)
    lin.reset_parameters(0.05, None)
    with torch.no_grad():
        for blk in lin.lora_b_blocks():
            blk.normal_(0, 0.1)
    lin.sync_adapter_()
    (amat, R, s), (bt, _, _) = lin.tail_operands()
    pad, K, N = lin.pad, 48, 64
    x0 = torch.randn(10, K)
    dy0 = torch.randn(10, N)

    class Produce(torch.autograd.Function):
        """identity whose output / gradient live in padded buffers with producer-written tails"""
        @staticmethod
        def forward(ctx, x, bad):
            ctx.bad = bad
            buf = torch.empty(x.shape[0], K + pad)
            buf[:, :K] = x
            buf[:, K:] = s * x @ amat.t() + (1.0 if bad == "x" else 0.0)
            return buf[:, :K]

        @staticmethod
        def backward(ctx, g):
            return g, None

    class GradPad(torch.autograd.Function):
        @staticmethod
        def forward(ctx, y, bad):
            ctx.bad = bad
            return y.view_as(y)

        @staticmethod
        def backward(ctx, g):
            buf = torch.empty(g.shape[0], N + pad)
            buf[:, :N] = g
            buf[:, N:] = s * g @ bt.t() + (1.0 if ctx.bad == "dy" else 0.0)
            return buf[:, :N], None

    def run(bad=None, fused=True):
        lin.lora_a.grad = lin.lora_b.grad = None
        x = x0.clone().requires_grad_(True)
        xin = Produce.apply(x, bad) if fused else x
        y = lin(xin, x_tail=fused, dy_tail=fused)
        y = GradPad.apply(y, bad) if fused else y
        y.backward(dy0)
        return y.detach(), x.grad, lin.lora_a.grad.clone(), lin.lora_b.grad.clone()

    want = run(fused=False)
    for g, w in zip(run(), want):
        torch.testing.assert_close(g, w, rtol=1e-5, atol=1e-5)
    assert not torch.allclose(run("x")[0], want[0])
    assert not torch.allclose(run("dy")[2], want[2])
    # flags set but the tensors arrive unpadded: tails recomputed, same result
    x = x0.clone().requires_grad_(True)
    lin.lora_a.grad = lin.lora_b.grad = None
    y = lin(x, x_tail=True, dy_tail=True)
    y.backward(dy0)
    torch.testing.assert_close(y.detach(), want[0], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(lin.lora_a.grad, want[2], rtol=1e-5, atol=1e-5)


def test_attention_bwd_chunking_assembles_head_ranges(monkeypatch):
    """The long-context bound on the attention backward (mxllm/ops/attention.py attn_bwd): with a
    budget below one call's dS^T image the backward runs per (sequence, KV-group chunk) and writes
    each chunk's dQ and per-q-head dK / dV partials into its head range.  A CPU stand-in for the
    native op (fp32 autograd, per-q-head partials, the out= arguments honoured) checks the slicing
    and the assembly against one unchunked call."""
    from mxllm.ops import attention as A
    from mxllm.ops import reference as R

    class Fake:
        calls = 0

        def attn_bwd(self, do, q, k, v, o, lse, causal, scale, mode, dq_out=None, dk_out=None, dv_out=None):
            Fake.calls += 1
            B, Hq, S, D = q.shape
            Hkv = k.shape[1]
            G = Hq // Hkv
            qf = q.detach().float().clone().requires_grad_(True)
            kr = k.detach().float().repeat_interleave(G, dim=1).requires_grad_(True)  # per-q-head copies -> partials
            vr = v.detach().float().repeat_interleave(G, dim=1).requires_grad_(True)
            out = R.attention(qf.transpose(1, 2), kr.transpose(1, 2), vr.transpose(1, 2), causal, scale)
            out.backward(do.reshape(B, S, Hq, D).float())
            res = (qf.grad, kr.grad, vr.grad)
            if dq_out is None:
                return res
            for dst, src in zip((dq_out, dk_out, dv_out), res):
                dst.copy_(src)
            return dq_out, dk_out, dv_out

    torch.manual_seed(0)
    B, Hq, Hkv, S, D = 2, 8, 2, 64, 16
    q = torch.randn(B, Hq, S, D)
    k = torch.randn(B, Hkv, S, D)
    v = torch.randn(B, Hkv, S, D)
    o = torch.randn(B, S, Hq * D)
    lse = torch.zeros(B, Hq, S)
    do = torch.randn(B * S, Hq * D)
    monkeypatch.setattr(A, "native", lambda: Fake())
    want = Fake().attn_bwd(do, q, k, v, o, lse, True, 0.25, 3)
    per_head = 128 * 64 * 2
    monkeypatch.setattr(A, "_DS_BUDGET", 4 * per_head)  # one KV group (4 heads) per chunk
    Fake.calls = 0
    got = A.attn_bwd(do, q, k, v, o, lse, True, 0.25, 3)
    assert Fake.calls == B * (Hq // 4)
    for g, w in zip(got, want):
        torch.testing.assert_close(g, w, rtol=1e-5, atol=1e-6)


def test_fp8_weight_quantization_roundtrip():
    """Serving-time e4m3 weight quantisation (mxllm/serve/quant.py): per-channel
    scales, no zero / subnormal codes (the HIP decoder relies on it), the
    reference decoder agrees with torch's float8_e4m3fn, and the round-trip
    error is what 3 mantissa bits give."""
    from mxllm.serve.quant import dequantize_e4m3, quantize_e4m3

    torch.manual_seed(0)
    w = torch.randn(96, 512) * 0.02
    w[3, :5] = 0.0  # exact zeros -> smallest normal code
    q, s = quantize_e4m3(w)
    assert q.dtype == torch.uint8 and s.shape == (96,)
    assert int(((q & 0x78) == 0).sum()) == 0
    ref = q.view(torch.float8_e4m3fn).float() * s[:, None]
    assert torch.equal(dequantize_e4m3(q, s), ref)
    err = (dequantize_e4m3(q, s) - w).norm() / w.norm()
    assert err < 0.04, err
    assert (dequantize_e4m3(q, s)[3, :5].abs() <= s[3] * 2 ** -6 + 1e-12).all()


def test_lora_dx_image_matches_augmented_buffer():
    """FusedLinear's transposed [W; A] image (dX in the reduction-contiguous
    GEMM form) gives the same input gradient as the augmented buffer, also
    after an adapter update is synced."""
    import torch

    from mxllm.models.llama import FusedLinear

    torch.manual_seed(0)
    kw = dict(dtype=torch.float32, device="cpu", lora_r=4, lora_alpha=8.0, train_base=False)
    a = FusedLinear(64, [32, 16, 16], dx_image=True, **kw)
    b = FusedLinear(64, [32, 16, 16], dx_image=False, **kw)
    gen = torch.Generator().manual_seed(1)
    a.reset_parameters(0.02, gen)
    b.load_state_dict(a.state_dict(), strict=False)
    with torch.no_grad():
        b.wbuf.copy_(a.wbuf)
        for m in (a, b):
            m.lora_b.normal_(0, 0.1, generator=torch.Generator().manual_seed(2))
            m.sync_adapter_()
    assert a.wxt is not None and not hasattr(b, "wxt")
    for step in range(2):
        x = torch.randn(8, 64, generator=torch.Generator().manual_seed(3 + step))
        xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        dy = torch.randn(8, 64, generator=torch.Generator().manual_seed(9))
        a(xa).backward(dy)
        b(xb).backward(dy)
        assert torch.allclose(xa.grad, xb.grad, atol=1e-5)
        with torch.no_grad():  # adapter update, then the owner's sync
            for m in (a, b):
                m.lora_a.add_(0.05)
                m.sync_adapter_()


def test_split_master_roundtrip_exact():
    """SplitMaster (mxllm/ops/optim.py): fp32 -> (bf16 hi, int16 lo) -> fp32 is the
    identity on the bits; hi is the value rounded half-up on its bit pattern (= RNE
    except at exact ties); AdamW through a split master equals AdamW on fp32."""
    from mxllm.ops import SplitMaster, adamw_step_

    g = torch.Generator().manual_seed(0)
    x = torch.cat([torch.randn(10000, generator=g) * s for s in (1e-30, 1e-3, 1.0, 1e4, 1e30)])
    x = torch.cat([x, -x, torch.tensor([0.0, -0.0, 1.0 + 2 ** -8, -(1.0 + 2 ** -8), 3.0 + 2 ** -7])])
    sm = SplitMaster(torch.empty(x.numel(), dtype=torch.bfloat16))
    sm.copy_(x)
    assert torch.equal(sm.float().view(torch.int32), x.view(torch.int32))
    bits = x.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    want_hi = ((bits + 0x8000) >> 16) & 0xFFFF
    assert torch.equal(sm.hi.view(torch.int16).to(torch.int64) & 0xFFFF, want_hi)
    ne = (bits & 0xFFFF) != 0x8000  # not a tie: same as round-to-nearest-even
    assert torch.equal(sm.hi[ne], x[ne].bfloat16())
    # slices are views of both halves
    sm[5:10].copy_(torch.full((5,), 2.5))
    assert torch.equal(sm.float()[5:10], torch.full((5,), 2.5))
    # AdamW: split master == fp32 master, bit for bit
    n = 4096
    p32 = torch.randn(n, generator=g)
    grad = torch.randn(n, generator=g).bfloat16()
    m1, v1, m2, v2 = (torch.zeros(n) for _ in range(4))
    sp = SplitMaster(torch.empty(n, dtype=torch.bfloat16))
    sp.copy_(p32)
    for step in range(1, 4):
        kw = dict(lr=1e-3, beta1=0.9, beta2=0.95, eps=1e-8, weight_decay=0.01, step=step, grad_scale=0.5)
        adamw_step_(p32, grad, m1, v1, None, **kw)
        adamw_step_(sp, grad, m2, v2, None, **kw)
    assert torch.equal(sp.float(), p32) and torch.equal(m1, m2) and torch.equal(v1, v2)


def test_chunked_linear_cross_entropy_matches_reference():
    """LM head + CE walked over T in chunks (global valid-token count, dh / dW formed in the
    forward, scaled by the upstream gradient in the backward) == autograd of the plain form."""
    import torch.nn.functional as F

    from mxllm.ops.loss import ce_chunk_tokens, linear_cross_entropy

    torch.manual_seed(0)
    T, H, V = 37, 16, 50
    h = torch.randn(T, H, dtype=torch.float64, requires_grad=True)
    w = torch.randn(V, H, dtype=torch.float64, requires_grad=True)
    lab = torch.randint(0, V, (T,))
    lab[3] = lab[20] = -100
    for chunk in (8, 36, 37):
        l1 = linear_cross_entropy(h, w, lab, chunk=chunk)
        (l1 * 0.5).backward()
        g1h, g1w = h.grad.clone(), w.grad.clone()
        h.grad = w.grad = None
        l2 = F.cross_entropy(h @ w.t(), lab, ignore_index=-100)
        (l2 * 0.5).backward()
        assert abs(float(l1) - float(l2)) < 1e-6
        assert torch.allclose(g1h, h.grad, atol=1e-7) and torch.allclose(g1w, w.grad, atol=1e-7)
        h.grad = w.grad = None
    assert ce_chunk_tokens(4096, 128256) == 4096  # 1 GB of logits: one piece
    assert ce_chunk_tokens(32768, 128256) == 4096  # 8.4 GB: chunked
    # under no_grad the chunked path forms no gradients (same loss) ...
    from unittest import mock

    import mxllm.ops.loss as L

    with torch.no_grad(), mock.patch.object(L, "weight_grad_", side_effect=AssertionError("dW formed")):
        l3 = linear_cross_entropy(h, w, lab, chunk=8)
    assert abs(float(l3) - float(l2)) < 1e-6
    # ... and a second backward through the consumed accumulator is refused, not applied twice
    l4 = linear_cross_entropy(h, w, lab, chunk=8)
    l4.backward(retain_graph=True)
    import pytest

    with pytest.raises(RuntimeError, match="only once|inplace"):  # autograd version check or ours
        l4.backward()


def test_swiglu_linear_recompute_matches_saved_activation(monkeypatch):
    """Full fine-tuning with selective checkpointing: the un-checkpointed layers recompute the MLP
    activation m = swiglu(gu) (mxllm/ops/linear.py _SwiGLULinearFn) and the normed qkv / gate-up
    inputs (_NormedLinearFn) in the backward instead of saving them; loss and every gradient equal
    the saving path, also with 0 layers checkpointed."""
    import mxllm.models.llama as L
    from mxllm.models import get_config

    cfg = get_config("tiny").replace(n_layers=3)
    ids = torch.randint(0, cfg.vocab_size, (2, 32), generator=torch.Generator().manual_seed(0))

    def run(policy, norm="auto", ck=1):
        monkeypatch.setattr(L, "RECOMPUTE_SWIGLU", policy)
        monkeypatch.setattr(L, "RECOMPUTE_NORM", norm)
        m = L.Llama(cfg, device="cpu", dtype=torch.float32, seed=4, activation_checkpointing=ck)
        calls, ncalls = [], []
        real, nreal = L.ops.swiglu_linear, L.ops.normed_linear
        monkeypatch.setattr(L.ops, "swiglu_linear", lambda gu, w: calls.append(1) or real(gu, w))
        monkeypatch.setattr(L.ops, "normed_linear", lambda *a: ncalls.append(1) or nreal(*a))
        loss = m(ids, ids)
        loss.backward()
        return float(loss), {n: p.grad.clone() for n, p in m.named_parameters()}, len(calls), len(ncalls)

    l0, g0, n0, k0 = run("0")
    for args, (n_m, n_x) in ((("auto",), (2, 4)), (("auto", "0"), (2, 0)), (("auto", "auto", 0), (3, 6))):
        l1, g1, n1, k1 = run(*args)
        assert (n0, k0) == (0, 0) and (n1, k1) == (n_m, n_x), args  # ck 1: layers 1 and 2 recompute
        assert abs(l0 - l1) < 1e-6
        for k in g0:
            torch.testing.assert_close(g1[k], g0[k], rtol=1e-5, atol=1e-6)


def test_fused_epilogue_predicates_match_native_limits():
    """the fused-epilogue predicates check what mx_gemm8_epi declines (strides,
    alignment, the 2^31-byte operand spans), so a predicate that says yes is never met by a
    declined launch; a 405B-class gate-up weight stays on the unfused path."""
    from mxllm.ops.gemm import g8_swiglu_takes

    x = torch.empty(4096, 8192, dtype=torch.bfloat16, device="meta")
    assert g8_swiglu_takes(x, torch.empty(57344, 8192, dtype=torch.bfloat16, device="meta"))  # 70B gate-up
    assert not g8_swiglu_takes(torch.empty(4096, 16384, dtype=torch.bfloat16, device="meta"),
                               torch.empty(106496, 16384, dtype=torch.bfloat16, device="meta"))
    assert not g8_swiglu_takes(torch.empty(4096, 8196, dtype=torch.bfloat16, device="meta")[:, :8192],
                               torch.empty(57344, 8192, dtype=torch.bfloat16, device="meta"))  # lda % 8


def test_counted_wait_isa_check_fails_closed():
    """an assembly with no counted wait left is NOT a pass."""
    from mxllm._build import _attn_bwd_counted_wait_ok

    asm = "_ZN2mx16attn_bwd8_kernelILi1EEEvv:\n s_waitcnt vmcnt(0)\n s_barrier\n.Lfunc_end0:\n"
    ok, detail = _attn_bwd_counted_wait_ok(asm)
    assert not ok and "nothing verified" in detail
