"""HIP kernel numerics vs plain-PyTorch fp32 references.

Random (never zero) data, odd shapes where the kernel supports them.
"""
import math

import pytest
import torch

from mxllm.ops import reference as ref

pytestmark = pytest.mark.gpu


def _ops():
    from mxllm.ops import native

    return native()


def rel_err(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


@pytest.mark.parametrize("T,H", [(1, 64), (37, 512), (512, 4096), (64, 8192), (3, 16384)])
def test_rmsnorm_fwd_bwd(gpu, T, H):
    torch.manual_seed(0)
    x = torch.randn(T, H, device=gpu, dtype=torch.bfloat16)
    w = (1 + 0.1 * torch.randn(H, device=gpu)).to(torch.bfloat16)
    y, rstd, _ = _ops().rmsnorm_fwd(x, None, w, 1e-5)
    xf = x.float().requires_grad_(True)
    wf = w.float().requires_grad_(True)
    yr = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-5) * wf
    assert rel_err(y, yr) < 1e-2
    dy = torch.randn_like(x)
    yr.backward(dy.float())
    dres = torch.randn_like(x)
    dx, dw = _ops().rmsnorm_bwd(dy, x, w, rstd, dres, True)
    assert rel_err(dx, xf.grad + dres.float()) < 1e-2
    assert rel_err(dw, wf.grad) < 1e-3


def test_add_rmsnorm(gpu):
    torch.manual_seed(1)
    x = torch.randn(300, 1024, device=gpu, dtype=torch.bfloat16)
    r = torch.randn_like(x)
    w = torch.randn(1024, device=gpu, dtype=torch.bfloat16)
    y, rstd, h = _ops().rmsnorm_fwd(x, r, w, 1e-5)
    href = (x.float() + r.float()).to(torch.bfloat16)
    assert torch.equal(h, href)
    assert rel_err(y, ref.rms_norm(href, w, 1e-5).float()) < 1e-2


@pytest.mark.parametrize("T,F", [(1, 8), (129, 1024), (1024, 14336)])
def test_swiglu(gpu, T, F):
    torch.manual_seed(2)
    gu = torch.randn(T, 2 * F, device=gpu, dtype=torch.bfloat16)
    m = _ops().swiglu_fwd(gu)
    guf = gu.float().requires_grad_(True)
    mr = torch.nn.functional.silu(guf[:, :F]) * guf[:, F:]
    assert rel_err(m, mr) < 1e-2
    dm = torch.randn_like(m)
    mr.backward(dm.float())
    dgu = _ops().swiglu_bwd(dm, gu)
    assert rel_err(dgu, guf.grad) < 1e-2
    # the recompute backward: same dgu and bitwise the forward's m from one pass over gu
    dgu2, m2 = _ops().swiglu_bwd_m(dm, gu)
    assert torch.equal(dgu2, dgu) and torch.equal(m2, m)


# The large shapes under one norm ratio.  The exact and per-element checks of this kernel -- every template
# instantiation with several trips per workgroup and uneven splits, one-hot routing, the operand refusals --
# are tests/test_lora_strict_gpu.py ``test_swiglu_lora_strict`` / ``test_swiglu_lora_refusals``.
@pytest.mark.parametrize("rbw", ["1", "2", "4"])
@pytest.mark.parametrize("bwd", [False, True])
@pytest.mark.parametrize("T,F,R", [(16, 128, 16), (48, 384, 32), (1024, 1536, 48), (256, 256, 64), (4096, 28672, 16)])
def test_swiglu_lora_tail(gpu, T, F, R, bwd, rbw, monkeypatch):
    """SwiGLU fused with the neighbour's LoRA tail (csrc/kernels/lora.hip swiglu_lora_kernel):
    the SwiGLU output is bitwise the plain kernel's, the tail is s out V[:R]^T against fp32,
    zeros past R (V rows past R deliberately non-zero), bit-reproducible."""
    from mxllm.ops.linear import _padded_rows

    monkeypatch.setenv("MXLLM_SWIGLU_LORA_RBW", rbw)  # 16-row blocks per workgroup (clamped to T)
    torch.manual_seed(4)
    pad, s = 64, 2.0
    gu = torch.randn(T, 2 * F, device=gpu, dtype=torch.bfloat16)
    W = 2 * F if bwd else F
    V = torch.randn(pad, W + 24, device=gpu, dtype=torch.bfloat16)[:, :W]  # padded row stride
    dm = torch.randn(T, F, device=gpu, dtype=torch.bfloat16) if bwd else None
    out = _ops().swiglu_lora(dm, gu, pad, V, R // 16, s)
    plain = _ops().swiglu_bwd(dm, gu) if bwd else _ops().swiglu_fwd(gu)
    assert torch.equal(out, plain)
    full = _padded_rows(out, pad)
    assert full is not None
    tail = full[:, W:]
    ref_tail = s * (out.float() @ V[:R].float().t())
    assert rel_err(tail[:, :R], ref_tail) < 1e-2
    assert not tail[:, R:].any()
    again = _padded_rows(_ops().swiglu_lora(dm, gu, pad, V, R // 16, s), pad)
    assert torch.equal(again[:, W:], tail)


def test_attention_bwd_bounded_ds_image(gpu, monkeypatch):
    """Long-context memory bound: with the split-mode dS^T image over budget, the backward runs per
    (sequence, KV-group chunk) and gives the one-call dQ, and per-KV-head dK / dV (partials summed),
    to fp32 rounding."""
    from mxllm.ops import attention as A

    torch.manual_seed(11)
    B, Hq, Hkv, S, D = 2, 8, 2, 512, 128
    q = torch.randn(B, Hq, S, D, device=gpu, dtype=torch.bfloat16)
    k = torch.randn(B, Hkv, S, D, device=gpu, dtype=torch.bfloat16)
    v = torch.randn(B, Hkv, S, D, device=gpu, dtype=torch.bfloat16)
    sc = 1 / math.sqrt(D)
    o, lse = _ops().attn_fwd(q, k, v, True, sc)
    do = torch.randn(B * S, Hq * D, device=gpu, dtype=torch.bfloat16)
    ref_dq, ref_dk, ref_dv = _ops().attn_bwd(do, q, k, v, o, lse, True, sc, 3)
    monkeypatch.setattr(A, "_DS_BUDGET", 1.5 * 2**20)  # < one KV group's image: 4 chunks of 4 heads
    dq, dk, dv = A.attn_bwd(do, q, k, v, o, lse, True, sc, 3)
    assert dq.shape == ref_dq.shape
    assert rel_err(dq, ref_dq) < 1e-5

    def per_kv(t):
        return t.view(B, Hkv, -1, S, D).sum(2)

    assert rel_err(per_kv(dk), per_kv(ref_dk)) < 1e-5
    assert rel_err(per_kv(dv), per_kv(ref_dv)) < 1e-5


@pytest.mark.parametrize("T,V", [(5, 1000), (256, 128256)])
def test_cross_entropy(gpu, T, V):
    torch.manual_seed(3)
    logits = (3 * torch.randn(T, V, device=gpu)).to(torch.bfloat16)
    labels = torch.randint(0, V, (T,), device=gpu)
    labels[1] = -100
    lf = logits.float().requires_grad_(True)
    lr_ = torch.nn.functional.cross_entropy(lf, labels, ignore_index=-100)
    lr_.backward()
    work = logits.clone()
    loss, _ = _ops().ce_fwd_bwd(work, labels, -100)
    assert abs(loss.item() - lr_.item()) < 1e-3 * max(1.0, abs(lr_.item()))
    assert rel_err(work, lf.grad) < 1e-2
    assert work[1].abs().max().item() == 0.0


@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16])
def test_adamw(gpu, gdt):
    torch.manual_seed(4)
    n = 10000 * 4
    p = torch.randn(n, device=gpu)
    g = torch.randn(n, device=gpu).to(gdt)
    m = torch.randn(n, device=gpu).abs() * 0.1
    v = torch.randn(n, device=gpu).abs() * 0.1
    pr, mr, vr = p.clone(), m.clone(), v.clone()
    lowp = torch.empty(n, device=gpu, dtype=torch.bfloat16)
    kw = dict(lr=1e-3, beta1=0.9, beta2=0.95, eps=1e-8, weight_decay=0.1, step=3)
    ref.adamw_(pr, g, mr, vr, grad_scale=0.5, **kw)
    from mxllm.ops import adamw_step_

    g0 = g.clone()
    adamw_step_(p, g, m, v, lowp, grad_scale=torch.tensor([0.5], device=gpu), **kw)
    assert rel_err(p, pr) < 1e-6 and rel_err(m, mr) < 1e-6 and rel_err(v, vr) < 1e-6
    assert torch.equal(lowp, p.to(torch.bfloat16))
    assert torch.equal(g, g0)  # untouched without zero_grad
    # fused gradient clearing: same update, gradient zeroed in the same pass
    p2, m2, v2 = p.clone(), m.clone(), v.clone()
    p3, m3, v3 = p.clone(), m.clone(), v.clone()
    adamw_step_(p2, g, m2, v2, None, grad_scale=0.5, **kw)
    adamw_step_(p3, g, m3, v3, None, grad_scale=0.5, zero_grad=True, **kw)
    assert torch.equal(p2, p3) and torch.equal(m2, m3) and torch.equal(v2, v3)
    assert g.abs().max().item() == 0.0


def test_embedding(gpu):
    torch.manual_seed(5)
    V, H, T = 1000, 512, 333
    w = torch.randn(V, H, device=gpu, dtype=torch.bfloat16)
    ids = torch.randint(0, V, (T,), device=gpu)
    out = _ops().embedding_fwd(ids, w)
    assert torch.equal(out, w[ids])
    dy = torch.randn(T, H, device=gpu, dtype=torch.bfloat16)
    dw = _ops().embedding_bwd(dy, ids, V)
    dref = torch.zeros(V, H, device=gpu).index_add_(0, ids, dy.float())
    assert rel_err(dw, dref) < 1e-5


@pytest.mark.parametrize("D", [32, 64, 128])
def test_rope_split_merge(gpu, D):
    torch.manual_seed(6)
    B, S, Hq, Hkv = 2, 70, 8, 2
    cos, sin = ref.rope_tables(256, D, 500000.0, {"factor": 8.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0,
                                                    "original_max_position_embeddings": 8192}, gpu)
    qkv = torch.randn(B * S, (Hq + 2 * Hkv) * D, device=gpu, dtype=torch.bfloat16)
    q, k, v = _ops().rope_split(qkv, cos, sin, B, S, Hq, Hkv, D)
    x = qkv.view(B, S, Hq + 2 * Hkv, D)
    qr = ref.apply_rope(x[:, :, :Hq], cos, sin).transpose(1, 2)
    kr = ref.apply_rope(x[:, :, Hq:Hq + Hkv], cos, sin).transpose(1, 2)
    assert rel_err(q, qr) < 1e-2 and rel_err(k, kr) < 1e-2
    assert torch.equal(v, x[:, :, Hq + Hkv:].transpose(1, 2).contiguous())
    # backward: merge(dq, dk partials per q head, dv partials) == autograd of split+rope+GQA-repeat
    xf = qkv.float().view(B, S, Hq + 2 * Hkv, D).requires_grad_(True)
    qf = ref.apply_rope(xf[:, :, :Hq], cos, sin).transpose(1, 2)
    kf = ref.apply_rope(xf[:, :, Hq:Hq + Hkv], cos, sin).transpose(1, 2).repeat_interleave(Hq // Hkv, 1)
    vf = xf[:, :, Hq + Hkv:].transpose(1, 2).repeat_interleave(Hq // Hkv, 1)
    dq = torch.randn(B, Hq, S, D, device=gpu)
    dkp = torch.randn(B, Hq, S, D, device=gpu)
    dvp = torch.randn(B, Hq, S, D, device=gpu)
    (qf * dq + kf * dkp + vf * dvp).sum().backward()
    dqkv = _ops().rope_merge_bwd(dq, dkp, dvp, cos, sin, B, S, Hq, Hkv, D)
    assert rel_err(dqkv, xf.grad.view(B * S, -1)) < 1e-2


ATTN_SHAPES = [
    (1, 4, 1, 128, 128, 128, True),
    (2, 8, 2, 200, 200, 128, True),
    (1, 8, 8, 256, 256, 64, False),
    (1, 4, 2, 77, 77, 32, True),
    (2, 16, 2, 512, 512, 128, True),
    (1, 8, 2, 64, 320, 128, True),   # prefill with a cached prefix (bottom-right causal)
    (1, 4, 2, 100, 300, 128, False),  # non-causal, key tail past the last full 64-key tile
    (1, 4, 1, 700, 700, 128, True),   # several 256-row query blocks, partial last block
]


@pytest.mark.parametrize("B,Hq,Hkv,S,Sk,D,causal", ATTN_SHAPES)
def test_attention_fwd_bwd(gpu, B, Hq, Hkv, S, Sk, D, causal):
    torch.manual_seed(7)
    q = torch.randn(B, Hq, S, D, device=gpu, dtype=torch.bfloat16)
    k = torch.randn(B, Hkv, Sk, D, device=gpu, dtype=torch.bfloat16)
    v = torch.randn(B, Hkv, Sk, D, device=gpu, dtype=torch.bfloat16)
    scale = 1.0 / math.sqrt(D)
    o, lse = _ops().attn_fwd(q, k, v, causal, scale)
    qf, kf, vf = [t.float().requires_grad_(True) for t in (q, k, v)]
    orf = ref.attention(qf.transpose(1, 2), kf.transpose(1, 2), vf.transpose(1, 2), causal=causal)  # [B,S,Hq,D]
    assert rel_err(o.view(B, S, Hq, D), orf) < 2e-2
    # lse (log2 domain) vs reference
    s = torch.matmul(qf, kf.repeat_interleave(Hq // Hkv, 1).transpose(-1, -2)) * scale
    if causal:
        i = torch.arange(S, device=gpu).view(S, 1)
        j = torch.arange(Sk, device=gpu).view(1, Sk)
        s = s.masked_fill(j > i + (Sk - S), float("-inf"))
    lse_ref = torch.logsumexp(s, -1) / math.log(2)
    assert (lse - lse_ref).abs().max().item() < 2e-2
    do = torch.randn(B, S, Hq, D, device=gpu, dtype=torch.bfloat16)
    orf.backward(do.float())
    dq, dkp, dvp = _ops().attn_bwd(do.view(B, S, Hq * D), q, k, v, o, lse, causal, scale)
    rep = Hq // Hkv
    dk = dkp.view(B, Hkv, -1, Sk, D).sum(2)  # partials: per q-head or per q-head group
    dv = dvp.view(B, Hkv, -1, Sk, D).sum(2)
    assert rel_err(dq, qf.grad) < 3e-2
    assert rel_err(dk, kf.grad) < 3e-2
    assert rel_err(dv, vf.grad) < 3e-2


@pytest.mark.parametrize("causal", [True, False])
def test_attention_fwd_growing_max(gpu, causal):
    """Exercise the forward's deferred-rescale branch (rescale only when a row's
    tile max exceeds its running max by > 2^8): scores grow with the key index,
    steeply for some rows (a rescale on nearly every 64-key tile, max jumps of
    tens of log2 units) and gently for others (growth below the threshold, so
    probabilities > 1 are carried), mixed inside every wave."""
    torch.manual_seed(3)
    B, Hq, Hkv, S, D = 1, 4, 1, 640, 128
    keypos = torch.arange(S, device=gpu, dtype=torch.float32) / S
    k = torch.randn(B, Hkv, S, D, device=gpu) * 0.3
    k[..., 0] = keypos * 8.0  # a key feature that grows along the sequence
    q = torch.randn(B, Hq, S, D, device=gpu) * 0.3
    # per row: steep (~20 log2 units of max growth per tile: rescale every tile),
    # medium (~4 per tile: deferred max lags by up to 8) and flat rows
    slope = torch.tensor([200.0, 40.0, 3.0], device=gpu)[torch.arange(S, device=gpu) % 3]
    q[..., 0] = slope
    q, k = q.to(torch.bfloat16), k.to(torch.bfloat16)
    v = torch.randn(B, Hkv, S, D, device=gpu, dtype=torch.bfloat16)
    scale = 1.0 / math.sqrt(D)
    o, lse = _ops().attn_fwd(q, k, v, causal, scale)
    qf, kf, vf = q.float(), k.float(), v.float()
    orf = ref.attention(qf.transpose(1, 2), kf.transpose(1, 2), vf.transpose(1, 2), causal=causal)
    assert rel_err(o.view(B, S, Hq, D), orf) < 2e-2
    s = torch.matmul(qf, kf.repeat_interleave(Hq // Hkv, 1).transpose(-1, -2)) * scale
    if causal:
        i = torch.arange(S, device=gpu).view(S, 1)
        j = torch.arange(S, device=gpu).view(1, S)
        s = s.masked_fill(j > i, float("-inf"))
    lse_ref = torch.logsumexp(s, -1) / math.log(2)
    assert (lse - lse_ref).abs().max().item() < 2e-2


@pytest.mark.parametrize("causal,S", [(True, 2048), (True, 200), (False, 333)])
def test_attention_bwd_deterministic(gpu, causal, S):
    """Deterministic dQ modes (2: per-key-block partials + ordered reduction,
    3: dS^T through HBM + dQ kernel): bitwise identical across runs, equal to
    the atomic path up to f32 summation order."""
    torch.manual_seed(21)
    B, Hq, Hkv, D = 1, 8, 2, 128
    q = torch.randn(B, Hq, S, D, device=gpu, dtype=torch.bfloat16)
    k = torch.randn(B, Hkv, S, D, device=gpu, dtype=torch.bfloat16)
    v = torch.randn(B, Hkv, S, D, device=gpu, dtype=torch.bfloat16)
    sc = 1 / math.sqrt(D)
    o, lse = _ops().attn_fwd(q, k, v, causal, sc)
    do = torch.randn(B, S, Hq * D, device=gpu, dtype=torch.bfloat16)
    ra = _ops().attn_bwd(do, q, k, v, o, lse, causal, sc, 1)  # f32 atomics
    for mode in (2, 3):
        r1 = _ops().attn_bwd(do, q, k, v, o, lse, causal, sc, mode)
        r2 = _ops().attn_bwd(do, q, k, v, o, lse, causal, sc, mode)
        for a, b in zip(r1, r2):
            assert torch.equal(a, b), mode
        # mode 3 rounds dS to bf16 before the dQ GEMM (as the atomic path does in LDS)
        torch.testing.assert_close(r1[0], ra[0], rtol=1e-3, atol=1e-3)
        if mode == 2:  # same key-block kernel: dK / dV summed in the same order
            assert torch.equal(r1[1], ra[1]) and torch.equal(r1[2], ra[2])
        else:  # D=128 split mode: the 8-wave kernel sums its q halves (and q-heads) in its own order
            def g(t):
                return t.view(B, Hkv, -1, S, D).sum(2)
            torch.testing.assert_close(g(r1[1]), g(ra[1]), rtol=1e-4, atol=1e-4)
            torch.testing.assert_close(g(r1[2]), g(ra[2]), rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("mode", [3, 1])
def test_attention_training_shape_vs_fp32(gpu, mode):
    """The exact Llama-3.1-70B training attention shape (S=2048, Hq=64, Hkv=8,
    D=128, causal; one sequence) against an fp32 PyTorch reference: forward
    output and every gradient, through the default split backward (3) and the
    f32-atomic dQ path (1)."""
    torch.manual_seed(5)
    B, Hq, Hkv, S, D = 1, 64, 8, 2048, 128
    q = torch.randn(B, Hq, S, D, device=gpu, dtype=torch.bfloat16)
    k = torch.randn(B, Hkv, S, D, device=gpu, dtype=torch.bfloat16)
    v = torch.randn(B, Hkv, S, D, device=gpu, dtype=torch.bfloat16)
    sc = 1.0 / math.sqrt(D)
    o, lse = _ops().attn_fwd(q, k, v, True, sc)
    do = torch.randn(B, S, Hq, D, device=gpu, dtype=torch.bfloat16)
    dq, dkp, dvp = _ops().attn_bwd(do.view(B, S, Hq * D), q, k, v, o, lse, True, sc, mode)
    rep = Hq // Hkv
    dk = dkp.view(B, Hkv, -1, S, D).sum(2)
    dv = dvp.view(B, Hkv, -1, S, D).sum(2)
    qf, kf, vf = [t.float().requires_grad_(True) for t in (q, k, v)]
    orf = ref.attention(qf.transpose(1, 2), kf.transpose(1, 2), vf.transpose(1, 2), causal=True)
    assert rel_err(o.view(B, S, Hq, D), orf) < 2e-2
    orf.backward(do.float())
    assert rel_err(dq, qf.grad) < 3e-2
    assert rel_err(dk, kf.grad) < 3e-2
    assert rel_err(dv, vf.grad) < 3e-2


@pytest.mark.parametrize("hpw", [2, 4, 8])
def test_attention_bwd_heads_per_workgroup(gpu, hpw, monkeypatch):
    """The 8-wave backward with `hpw` q-heads of one KV group per workgroup (dK / dV summed over
    them in registers): [B, Hq / hpw, Sk, D] partials whose per-KV-head sums equal the one-head-
    per-workgroup result, and the same dQ (it does not depend on the grouping)."""
    torch.manual_seed(9)
    B, Hq, Hkv, S, D = 1, 16, 2, 640, 128
    q = torch.randn(B, Hq, S, D, device=gpu, dtype=torch.bfloat16)
    k = torch.randn(B, Hkv, S, D, device=gpu, dtype=torch.bfloat16)
    v = torch.randn(B, Hkv, S, D, device=gpu, dtype=torch.bfloat16)
    sc = 1.0 / math.sqrt(D)
    o, lse = _ops().attn_fwd(q, k, v, True, sc)
    do = torch.randn(B, S, Hq * D, device=gpu, dtype=torch.bfloat16)
    monkeypatch.setenv("MXLLM_ATTN_BWD8_HPW", "1")
    dq1, dk1, dv1 = _ops().attn_bwd(do, q, k, v, o, lse, True, sc, 3)
    monkeypatch.setenv("MXLLM_ATTN_BWD8_HPW", str(hpw))
    dq, dkp, dvp = _ops().attn_bwd(do, q, k, v, o, lse, True, sc, 3)
    assert dkp.shape == (B, Hq // hpw, S, D) and dk1.shape == (B, Hq, S, D)
    assert torch.equal(dq, dq1)

    def g(t):
        return t.view(B, Hkv, -1, S, D).sum(2)
    torch.testing.assert_close(g(dkp), g(dk1), rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(g(dvp), g(dv1), rtol=1e-4, atol=1e-4)


def test_attention_block_autograd(gpu):
    """Full split+rope+attention autograd node vs the reference path."""
    from mxllm.ops.attention import attention_block

    torch.manual_seed(8)
    B, S, Hq, Hkv, D = 2, 192, 8, 2, 128
    cos, sin = ref.rope_tables(S, D, 500000.0, None, gpu)
    qkv = torch.randn(B * S, (Hq + 2 * Hkv) * D, device=gpu, dtype=torch.bfloat16, requires_grad=True)
    o = attention_block(qkv, cos, sin, B, S, Hq, Hkv, D)
    go = torch.randn_like(o)
    o.backward(go)
    x = qkv.detach().float().requires_grad_(True)
    from mxllm.ops.attention import split_heads_ref

    qq, kk, vv = split_heads_ref(x, B, S, Hq, Hkv, D)
    orf = ref.attention(ref.apply_rope(qq, cos, sin), ref.apply_rope(kk, cos, sin), vv).reshape(B * S, -1)
    orf.backward(go.float())
    assert rel_err(o, orf) < 2e-2
    assert rel_err(qkv.grad, x.grad) < 3e-2


def test_segmented_mean(gpu):
    texts = ["test", "hello world", "é漢字", "x" * 5000]
    codes = torch.tensor([ord(c) for t in texts for c in t], dtype=torch.int32, device=gpu)
    offs = torch.tensor([0] + list(torch.tensor([len(t) for t in texts]).cumsum(0)), dtype=torch.int64, device=gpu)
    out = _ops().segmented_mean(codes, offs).cpu()
    for i, t in enumerate(texts):
        assert abs(out[i].item() - torch.tensor([ord(c) for c in t], dtype=torch.float32).mean().item()) < 1e-3


@pytest.mark.parametrize("dtype,n", [(torch.float32, 1_000_003), (torch.bfloat16, 3_000_001), (torch.bfloat16, 7)])
def test_sq_norm_deterministic(gpu, dtype, n):
    """sum(x^2) for f32 and bf16 (one read, fixed-order reduction): matches fp64,
    and is bitwise identical across calls (DDP replicas must agree on the clip)."""
    from mxllm.ops import sq_norm

    x = torch.randn(n, device=gpu).to(dtype)
    a, b = sq_norm(x), sq_norm(x)
    assert torch.equal(a, b)
    ref = x.double().pow(2).sum().item()
    assert abs(a.item() - ref) / ref < 1e-5


@pytest.mark.parametrize("M,K", [(1, 1024), (5, 1024), (16, 1536), (17, 1024), (32, 2048), (33, 1024),
                                 (64, 1024), (100, 1024), (5, 768)])
def test_w8_linear(gpu, M, K):
    """FP8-weight GEMM (decode kernel for M <= 32 and K % 512 == 0, dequantise +
    hipBLASLt otherwise) vs an fp32 matmul with the reference-decoded weights."""
    from mxllm.serve.quant import dequantize_e4m3, quantize_e4m3

    torch.manual_seed(11)
    N = 96
    w = torch.randn(N, K, device=gpu) * 0.02
    q, s = quantize_e4m3(w)
    x = torch.randn(M, K + 64, device=gpu, dtype=torch.bfloat16)[:, :K]  # strided rows (padded producer buffers)
    y = _ops().w8_linear(x, q, s)
    yr = x.float() @ dequantize_e4m3(q, s).t()
    assert y.shape == (M, N) and rel_err(y, yr) < 1e-2
    assert rel_err(_ops().w8_dequant(q, s), dequantize_e4m3(q, s)) < 5e-3


@pytest.mark.parametrize("nc", ["", "4"])
@pytest.mark.parametrize("M,K", [(1, 1536), (4, 1536), (8, 1536), (16, 1536), (8, 8192), (16, 8192),
                                 (8, 4608), (4, 16384), (5, 16384)])
def test_w8_linear_wide(gpu, M, K, nc, monkeypatch):
    """FP8-weight decode GEMM at a projection-sized N (>= 8192: the two-channel-group
    variant for 6..16 tokens, and for 4..5 at K >= 16384; MXLLM_W8_NC=4 the four-group one)
    vs an fp32 matmul with the reference-decoded weights.
    K = 8192 / 4608 give every wave enough k-chunks for the unrolled batch loop
    (and, at 4608, a remainder for its tail loop)."""
    monkeypatch.setenv("MXLLM_W8_NC", nc)
    from mxllm.serve.quant import dequantize_e4m3, quantize_e4m3

    torch.manual_seed(12)
    N = 8192
    w = torch.randn(N, K, device=gpu) * 0.02
    q, s = quantize_e4m3(w)
    x = torch.randn(M, K + 64, device=gpu, dtype=torch.bfloat16)[:, :K]
    y = _ops().w8_linear(x, q, s)
    yr = x.float() @ dequantize_e4m3(q, s).t()
    assert y.shape == (M, N) and rel_err(y, yr) < 1e-2


def test_quant_rows_e4m3(gpu):
    """Per-token activation quantisation kernel == torch's e4m3fn conversion of
    x / (amax / 448), and its decode reproduces x to e4m3 precision."""
    torch.manual_seed(12)
    x = (torch.randn(37, 1024 + 64, device=gpu) * 3).to(torch.bfloat16)[:, :1024]
    q, s = _ops().quant_rows_e4m3(x)
    xf = x.float()
    s_ref = xf.abs().amax(1, keepdim=True) / 448.0
    assert torch.allclose(s, s_ref, rtol=1e-6)
    ref = (xf / s).to(torch.float8_e4m3fn)
    mism = (q.view(torch.float8_e4m3fn).float() != ref.float()).float().mean().item()
    assert mism < 1e-3, mism  # RNE on both sides; only 1/s rounding can flip a tie
    assert rel_err(q.view(torch.float8_e4m3fn).float() * s, xf) < 0.04


@pytest.mark.parametrize("rows", [16, 32, 48, 64])
@pytest.mark.parametrize("T,K", [(16, 128), (48, 384), (96, 1024), (4096, 8192), (4096, 28672), (4096, 10240)])
def test_lora_xwt_tile(gpu, T, K, rows, monkeypatch):
    """Row-tiled lora_xwt (MXLLM_LORA_XWT=tile): only the first `rows` rows of V are the adapter ->
    out[:, :rows] = alpha x V[:rows]^T, zeros in the rest of the 64-column pad (V's padding rows
    are deliberately non-zero here), columns past the pad untouched, bit-reproducible; row counts
    that select 1, 2 and 4 row blocks per workgroup."""
    monkeypatch.setenv("MXLLM_LORA_XWT", "tile")
    torch.manual_seed(5)
    pad = 64
    buf = torch.randn(T, K + pad + 8, device=gpu, dtype=torch.bfloat16)
    x = buf[:, :K]
    v = torch.randn(pad, K + 16, device=gpu, dtype=torch.bfloat16)[:, :K]
    sentinel = buf[:, K + pad:].clone()
    _ops().lora_xwt(x, v, buf[:, K:K + pad], 2.0, rows)
    want = 2.0 * x.float() @ v[:rows].float().t()
    assert rel_err(buf[:, K:K + rows], want) < 1e-2
    assert not buf[:, K + rows:K + pad].any()
    assert torch.equal(buf[:, K + pad:], sentinel)
    first = buf[:, K:K + pad].clone()
    _ops().lora_xwt(x, v, buf[:, K:K + pad], 2.0, rows)
    assert torch.equal(buf[:, K:K + pad], first)


@pytest.mark.parametrize("kern", ["lds", "reg"])
@pytest.mark.parametrize("T,K,vrows", [(256, 512, 64), (256, 4096, 64), (4096, 1024, 128), (64, 192, 64),
                                       (4096, 8192, 64)])
def test_lora_xwt(gpu, T, K, vrows, kern, monkeypatch):
    """out[:, :vrows] = alpha x V^T into the tail of a padded buffer (S = 1 and the
    ordered split reduction), columns past the tail untouched; both kernels: the
    LDS-DMA-staged one (default) and the register-fragment one (MXLLM_LORA_XWT=reg)."""
    monkeypatch.setenv("MXLLM_LORA_XWT", kern)
    torch.manual_seed(3)
    buf = torch.randn(T, K + vrows + 8, device=gpu, dtype=torch.bfloat16)
    x = buf[:, :K]
    vb = torch.randn(vrows, K + 8, device=gpu, dtype=torch.bfloat16)
    v = vb[:, :K]
    sentinel = buf[:, K + vrows:].clone()
    _ops().lora_xwt(x, v, buf[:, K:K + vrows], 2.0)
    want = 2.0 * x.float() @ v.float().t()
    assert rel_err(buf[:, K:K + vrows], want) < 1e-2
    assert torch.equal(buf[:, K + vrows:], sentinel)
    first = buf[:, K:K + vrows].clone()
    _ops().lora_xwt(x, v, buf[:, K:K + vrows], 2.0)
    assert torch.equal(buf[:, K:K + vrows], first)  # bit-reproducible
    if kern == "lds":  # split partials merged in-launch (sc1 hand-off): same bits, counters reset
        monkeypatch.setenv("MXLLM_LORA_FUSED_RED", "1")
        for _ in range(2):
            buf[:, K:K + vrows] = 0
            _ops().lora_xwt(x, v, buf[:, K:K + vrows], 2.0)
            assert torch.equal(buf[:, K:K + vrows], first)


@pytest.mark.parametrize("T,K,splits,r,acc", [(256, 512, [512, 128, 128], 16, False),
                                              (4096, 1024, [1024, 256, 256], 16, True),
                                              (512, 256, [1024, 1024], 16, True),
                                              (256, 320, [192], 16, False),
                                              (256, 512, [512, 256, 256], 32, True)])
def test_lora_grads(gpu, T, K, splits, r, acc, monkeypatch):
    """dA = g^T x and the diagonal blocks dB_i = dy_i^T st_i in one launch,
    accumulated into bf16 grads or written fresh; off-diagonal blocks untouched;
    the in-launch split merge (MXLLM_LORA_FUSED_RED=1) gives the same bits."""
    torch.manual_seed(4)
    n, N = len(splits), sum(splits)
    R = n * r
    pad = (R + 63) // 64 * 64
    xa = torch.randn(T, K + pad, device=gpu, dtype=torch.bfloat16)
    dya = torch.randn(T, N + pad, device=gpu, dtype=torch.bfloat16)
    ga = torch.randn(R, K, device=gpu, dtype=torch.bfloat16) if acc else torch.zeros(R, K, device=gpu,
                                                                                       dtype=torch.bfloat16)
    gb = torch.randn(N, R, device=gpu, dtype=torch.bfloat16) if acc else torch.zeros(N, R, device=gpu,
                                                                                       dtype=torch.bfloat16)
    ga0, gb0 = ga.clone(), gb.clone()
    x2, dy2, g, st = xa[:, :K], dya[:, :N], dya[:, N:], xa[:, K:]
    _ops().lora_grads(x2, dy2, g, st, ga, gb, splits, r, acc)
    want_a = g[:, :R].float().t() @ x2.float() + (ga0.float() if acc else 0)
    assert rel_err(ga, want_a) < 1e-2
    want_b = gb0.float().clone()
    off = 0
    for i, ni in enumerate(splits):
        blk = dy2[:, off:off + ni].float().t() @ st[:, i * r:(i + 1) * r].float()
        want_b[off:off + ni, i * r:(i + 1) * r] = blk + (want_b[off:off + ni, i * r:(i + 1) * r] if acc else 0)
        off += ni
    assert rel_err(gb, want_b) < 1e-2
    mask = torch.ones_like(gb, dtype=torch.bool)
    off = 0
    for i, ni in enumerate(splits):
        mask[off:off + ni, i * r:(i + 1) * r] = False
        off += ni
    assert torch.equal(gb[mask], gb0[mask])  # off-diagonal blocks untouched
    ga1, gb1 = ga0.clone(), gb0.clone()
    _ops().lora_grads(x2, dy2, g, st, ga1, gb1, splits, r, acc)
    assert torch.equal(ga1, ga) and torch.equal(gb1, gb)  # bit-reproducible
    monkeypatch.setenv("MXLLM_LORA_FUSED_RED", "1")
    monkeypatch.setenv("MXLLM_LORA_XTG_WT", "0")
    for _ in range(2):
        ga1, gb1 = ga0.clone(), gb0.clone()
        _ops().lora_grads(x2, dy2, g, st, ga1, gb1, splits, r, acc)
        assert torch.equal(ga1, ga) and torch.equal(gb1, gb)
    # one 64-col tile per wave over all rows (MXLLM_LORA_XTG_WT=1; the tile threshold lowered so
    # these shapes qualify): same products to fp32 rounding, off-diagonal blocks untouched, reproducible
    monkeypatch.setenv("MXLLM_LORA_XTG_WT", "1")
    monkeypatch.setenv("MXLLM_LORA_XTG_WT_MIN", "16")
    outs = []
    for _ in range(2):
        ga1, gb1 = ga0.clone(), gb0.clone()
        _ops().lora_grads(x2, dy2, g, st, ga1, gb1, splits, r, acc)
        assert rel_err(ga1, want_a) < 1e-2 and rel_err(gb1, want_b) < 1e-2
        assert torch.equal(gb1[mask], gb0[mask])
        outs.append((ga1, gb1))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("R,C,ld", [(4096, 8192, None), (64, 64, None), (37, 130, None), (130, 4096, 4160),
                                    (4096, 1, None)])
def test_transpose2d(gpu, R, C, ld):
    """LDS-tiled 16-bit transpose (full fine-tuning dW operand images): exact,
    row-strided inputs and ragged edge tiles included."""
    torch.manual_seed(0)
    base = torch.randn(R, ld or C, device=gpu, dtype=torch.bfloat16)
    x = base[:, :C]
    y = _ops().transpose2d(x)
    assert y.shape == (C, R) and y.is_contiguous()
    assert torch.equal(y, x.t())
    # with a device-scalar scale (the CE upstream gradient folded into dlogits' image)
    sc = torch.tensor([0.3], device=gpu)
    ys = _ops().transpose2d(x, sc)
    assert torch.equal(ys, (x.float() * 0.3).bfloat16().t())


@pytest.mark.parametrize("T,N,K", [(4096, 1024, 512), (300, 130, 72)])
def test_weight_grad_tn(gpu, T, N, K):
    """Full fine-tuning dW through transposed token-contiguous images equals
    dy^T x (fp32 reference), with and without beta=1 accumulation."""
    from mxllm.ops.linear import weight_grad_

    torch.manual_seed(0)
    dy = torch.randn(T, N, device=gpu, dtype=torch.bfloat16)
    x = torch.randn(T, K, device=gpu, dtype=torch.bfloat16)
    want = dy.float().t() @ x.float()
    assert rel_err(weight_grad_(None, dy, x), want) < 1e-2
    acc = torch.randn(N, K, device=gpu, dtype=torch.bfloat16)
    want2 = acc.float() + want
    weight_grad_(acc, dy, x)
    assert rel_err(acc, want2) < 1e-2


@pytest.mark.parametrize("M,N,K", [(1, 6144, 4096), (5, 4096, 14336), (16, 1040, 512), (17, 2048, 1024),
                                   (32, 96, 4608)])
def test_skinny_linear_vs_fp32(gpu, M, N, K):
    """Decode GEMM (csrc/kernels/skinny_gemm.hip) against fp32 torch, incl. a row-strided x
    (the view a producer leaves) and both token-block variants (<= 16 and 17..32 rows)."""
    torch.manual_seed(M + N)
    xb = torch.randn(M, K + 64, device=gpu, dtype=torch.bfloat16)
    x = xb[:, :K]
    w = torch.randn(N, K, device=gpu, dtype=torch.bfloat16) * 0.05
    y = _ops().skinny_linear(x, w)
    ref = x.float() @ w.float().t()
    assert y.shape == (M, N) and rel_err(y, ref) < 1e-2


@pytest.mark.gpu
@pytest.mark.parametrize("M,F,K", [(1, 14336, 4096), (5, 520, 512), (8, 1024, 1536), (17, 256, 1024),
                                   (32, 512, 2048)])
def test_skinny_linear_swiglu(gpu, M, F, K):
    """Decode gate|up projection with SwiGLU in the epilogue: bit-identical to the decode
    GEMM + SwiGLU kernel, and close to fp32 silu(x Wg^T) * (x Wu^T).  x is row-strided."""
    import sys

    from mxllm import ops

    torch.manual_seed(M * 7 + K)
    xb = torch.randn(M, K + 64, device=gpu, dtype=torch.bfloat16)
    x = xb[:, :K]
    w = torch.randn(2 * F, K, device=gpu, dtype=torch.bfloat16) * 0.05
    y = _ops().skinny_linear_swiglu(x, w)
    two = ops.swiglu(_ops().skinny_linear(x, w))
    assert y.shape == (M, F) and torch.equal(y, two)
    gu = x.float() @ w.float().t()
    ref = torch.nn.functional.silu(gu[:, :F]) * gu[:, F:]
    assert rel_err(y, ref) < 1e-2
    if M <= sys.modules["mxllm.ops.linear"].SKINNY_M:  # the routed entry point takes it
        assert torch.equal(ops.linear_swiglu(x, w), y)


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K,resid,swiglu", [(1, 6144, 4096, False, False), (1, 1024, 4096, True, False),
                                                (3, 512, 8192, True, False), (4, 2048, 4096, True, True),
                                                (1, 28672 // 8, 8192, True, True), (2, 1040, 1536, False, True)])
def test_skinny_norm_linear(gpu, M, N, K, resid, swiglu):
    """Decode projection with the (residual-add +) RMSNorm in the GEMM prologue: bit-identical to
    the RMSNorm kernel followed by the decode GEMM (or the SwiGLU-epilogue GEMM), same new
    residual, and close to the fp32 reference."""
    from mxllm import ops

    torch.manual_seed(M + N + K)
    h = torch.randn(M, K, device=gpu, dtype=torch.bfloat16)
    d = torch.randn(M, K, device=gpu, dtype=torch.bfloat16) if resid else None
    gamma = (1.0 + 0.1 * torch.randn(K, device=gpu)).to(torch.bfloat16)
    w = torch.randn(N, K, device=gpu, dtype=torch.bfloat16) * 0.05
    y, h2 = _ops().skinny_norm_linear(h, d, gamma, 1e-5, w, swiglu)
    if resid:
        xn, hn = ops.add_rms_norm(d, h, gamma, 1e-5)
        assert torch.equal(h2, hn)
    else:
        xn, hn = ops.rms_norm(h, gamma, 1e-5), h
        assert h2.data_ptr() == h.data_ptr()
    two = _ops().skinny_linear_swiglu(xn, w) if swiglu else _ops().skinny_linear(xn, w)
    assert torch.equal(y, two)
    hf = hn.float()
    xr = hf * torch.rsqrt(hf.pow(2).mean(-1, keepdim=True) + 1e-5) * gamma.float()
    gu = xr @ w.float().t()
    ref = torch.nn.functional.silu(gu[:, :N // 2]) * gu[:, N // 2:] if swiglu else gu
    assert rel_err(y, ref) < 2e-2
    import sys

    if M <= sys.modules["mxllm.ops.linear"].NORM_M:  # the routed entry point takes it
        got = ops.norm_linear(d, h, gamma, 1e-5, w, swiglu)
        assert got is not None and torch.equal(got[0], y)


@pytest.mark.gpu
@pytest.mark.parametrize("M,Hq,Hkv,K,norm,resid", [(1, 32, 8, 4096, True, True), (2, 8, 2, 1024, True, False),
                                                   (2, 64, 8, 8192, True, True), (5, 16, 4, 2048, False, False)])
def test_skinny_qkv_rope(gpu, M, Hq, Hkv, K, norm, resid):
    """Decode QKV projection with RoPE + KV-cache append in the GEMM epilogue (and the RMSNorm
    in its prologue): the same q, cache rows and residual as RMSNorm + decode GEMM + rope_append."""
    from mxllm import ops

    torch.manual_seed(M * 3 + Hq)
    D, max_seq, nslots = 128, 300, M + 2
    N = (Hq + 2 * Hkv) * D
    h = torch.randn(M, K, device=gpu, dtype=torch.bfloat16)
    d = torch.randn(M, K, device=gpu, dtype=torch.bfloat16) if resid else None
    gamma = (1.0 + 0.1 * torch.randn(K, device=gpu)).to(torch.bfloat16) if norm else None
    w = torch.randn(N, K, device=gpu, dtype=torch.bfloat16) * 0.05
    cos, sin = ref.rope_tables(1024, D, 500000.0, None, gpu)
    pos = torch.tensor([17, 299, 0, 5, 123][:M], dtype=torch.int32, device=gpu)
    slots = torch.tensor([3, 0, 2, 1, 4][:M], dtype=torch.int32, device=gpu) % nslots
    kc = torch.randn(nslots, Hkv, max_seq, D, device=gpu, dtype=torch.bfloat16)
    vc = torch.randn_like(kc)
    kc2, vc2 = kc.clone(), vc.clone()
    q, h2 = _ops().skinny_qkv_rope(h, d, gamma, 1e-5, w, cos, sin, pos, slots, kc, vc, Hq, Hkv)
    if norm:
        if resid:
            xn, hn = ops.add_rms_norm(d, h, gamma, 1e-5)
        else:
            xn, hn = ops.rms_norm(h, gamma, 1e-5), h
        assert torch.equal(h2, hn)
    else:
        xn = h
    qkv = _ops().skinny_linear(xn, w)
    q_ref = _ops().rope_append(qkv, cos, sin, pos, slots, kc2, vc2, Hq, Hkv, D)
    assert torch.equal(q.view(M, -1), q_ref.reshape(M, -1))
    assert torch.equal(kc, kc2) and torch.equal(vc, vc2)


@pytest.mark.parametrize("target", ["bf16", "fp32"])
@pytest.mark.parametrize("fresh", [True, False])
def test_embedding_sparse_backward(gpu, target, fresh):
    """Embedding backward into the owner's gradient buffer (sorted ids, one workgroup per
    distinct id, touched rows only) vs an fp32 index_add reference: repeated ids, first
    write of the step (fresh: stale buffer contents ignored) or accumulation."""
    from mxllm.ops.embedding import embedding

    torch.manual_seed(7)
    V, H = 3000, 512
    w = torch.nn.Parameter(torch.randn(V, H, device=gpu).bfloat16())
    ids = torch.randint(0, 40, (1200,), device=gpu)  # heavy repetition
    ids[:5] = 2999
    dy = torch.randn(1200, H, device=gpu).bfloat16()
    init = torch.randn(V, H, device=gpu)
    if target == "fp32":
        w._mx_grad32 = init.clone()
    else:
        w.grad = init.bfloat16().clone()
    w._mx_grad_fresh = fresh
    embedding(ids, w).backward(dy)
    ref = torch.zeros(V, H, device=gpu).index_add_(0, ids.reshape(-1), dy.reshape(-1, H).float())
    base = 0 if fresh else (init if target == "fp32" else init.bfloat16().float())
    got = w._mx_grad32 if target == "fp32" else w.grad.float()
    tol = 1e-5 if target == "fp32" else 1e-2
    assert ((got - (base + ref)).abs().max() / (base + ref).abs().max()).item() < tol
    # deterministic: the same call again gives the same bits
    first = got.clone()
    if target == "fp32":
        w._mx_grad32.copy_(init)
    else:
        w.grad.copy_(init.bfloat16())
    w._mx_grad_fresh = fresh
    embedding(ids, w).backward(dy)
    again = w._mx_grad32 if target == "fp32" else w.grad.float()
    assert torch.equal(again, first)


def test_embedding_backward_tied_is_deterministic(gpu):
    """No owner buffer (tied embeddings: autograd sums the embedding and head gradients): the
    embedding gradient comes from the same sorted, fixed-order kernel into a zeroed fp32 [V, H]
    -- equal to an fp32 index_add reference and bitwise the same on every call (the atomic
    accumulator it replaces made tied-embedding training differ run to run)."""
    from mxllm.ops.embedding import embedding

    torch.manual_seed(3)
    V, H = 5000, 512
    ids = torch.randint(0, 64, (2048,), device=gpu)  # flat token ids (as the model passes them), heavy repetition
    dy = torch.randn(2048, H, device=gpu).bfloat16()
    grads = []
    for _ in range(3):
        w = torch.nn.Parameter(torch.zeros(V, H, device=gpu).bfloat16())
        w._mx_no_direct = True
        embedding(ids, w).backward(dy)
        grads.append(w.grad.float().clone())
    ref = torch.zeros(V, H, device=gpu).index_add_(0, ids.reshape(-1), dy.reshape(-1, H).float())
    assert rel_err(grads[0], ref) < 1e-2
    assert torch.equal(grads[0], grads[1]) and torch.equal(grads[0], grads[2])


def test_chunked_lm_head_ce_matches_unchunked_gpu(gpu):
    """Long-sequence LM head + CE walked in token chunks (ce_inv_count + ce_chunk_f32 kernels: the
    loss from fp32 logits, dh / dW formed per chunk) vs the one-piece fused path (bf16 logits) and an
    fp32 PyTorch reference: loss and gradients."""
    import torch.nn.functional as F

    from mxllm.ops.loss import linear_cross_entropy

    torch.manual_seed(11)
    T, H, V = 1000, 256, 4096
    h = (torch.randn(T, H, device=gpu) * 0.5).to(torch.bfloat16).requires_grad_(True)
    w = (torch.randn(V, H, device=gpu) * 0.05).to(torch.bfloat16).requires_grad_(True)
    lab = torch.randint(0, V, (T,), device=gpu)
    lab[::17] = -100
    res = []
    for chunk in (None, 256):
        loss = linear_cross_entropy(h, w, lab) if chunk is None else linear_cross_entropy(h, w, lab, chunk=chunk)
        (loss * 0.5).backward()
        res.append((float(loss.detach()), h.grad.float().clone(), w.grad.float().clone()))
        h.grad = w.grad = None
    hf, wf = h.detach().float().requires_grad_(True), w.detach().float().requires_grad_(True)
    lr = F.cross_entropy(hf @ wf.t(), lab, ignore_index=-100)
    (lr * 0.5).backward()
    (l0, gh0, gw0), (l1, gh1, gw1) = res
    assert abs(l1 - float(lr)) < 2e-6 * abs(float(lr))  # fp32 logits: the loss of the fp32 reference
    assert abs(l0 - float(lr)) < 2e-3 * abs(float(lr))  # bf16 logits
    for g, r in ((gh0, hf.grad), (gh1, hf.grad), (gw0, wf.grad), (gw1, wf.grad)):
        assert rel_err(g, r) < 2e-2


@pytest.mark.parametrize("S", [8192])
def test_attention_long_context_vs_fp32(gpu, S):
    """Long context: causal GQA attention at S=8192 through the training
    kernels (forward + the default split backward) against an fp32 PyTorch reference —
    output, dQ, dK, dV."""
    torch.manual_seed(9)
    B, Hq, Hkv, D = 1, 8, 2, 128
    q = torch.randn(B, Hq, S, D, device=gpu, dtype=torch.bfloat16)
    k = torch.randn(B, Hkv, S, D, device=gpu, dtype=torch.bfloat16)
    v = torch.randn(B, Hkv, S, D, device=gpu, dtype=torch.bfloat16)
    sc = 1.0 / math.sqrt(D)
    o, lse = _ops().attn_fwd(q, k, v, True, sc)
    do = torch.randn(B, S, Hq, D, device=gpu, dtype=torch.bfloat16)
    dq, dkp, dvp = _ops().attn_bwd(do.view(B, S, Hq * D), q, k, v, o, lse, True, sc, 3)
    dk = dkp.view(B, Hkv, -1, S, D).sum(2)
    dv = dvp.view(B, Hkv, -1, S, D).sum(2)
    qf, kf, vf = [t.float().requires_grad_(True) for t in (q, k, v)]
    orf = ref.attention(qf.transpose(1, 2), kf.transpose(1, 2), vf.transpose(1, 2), causal=True)
    assert rel_err(o.view(B, S, Hq, D), orf) < 2e-2
    orf.backward(do.float())
    assert rel_err(dq, qf.grad) < 3e-2
    assert rel_err(dk, kf.grad) < 3e-2
    assert rel_err(dv, vf.grad) < 3e-2


@pytest.mark.parametrize("f32", [True, False])
def test_embedding_bwd_sorted_dominant_id(gpu, f32):
    """Sorted, chunked embedding backward: a dominant id (here 80 % of 5,000 tokens, as
    pad / EOS in packed batches) is split over 64-row chunks whose partials are combined in chunk
    order -- the sums match an fp64 reference and repeat bitwise."""
    torch.manual_seed(13)
    T, H, V = 5000, 512, 300
    ids = torch.randint(0, V, (T,), device=gpu)
    ids[torch.rand(T, device=gpu) < 0.8] = 7
    dy = torch.randn(T, H, device=gpu, dtype=torch.bfloat16)
    sid, perm = torch.sort(ids, stable=True)
    outs = []
    for _ in range(2):
        out = torch.zeros(V, H, device=gpu, dtype=torch.float32 if f32 else torch.bfloat16)
        _ops().embedding_bwd_sorted(dy, sid, perm, out)
        outs.append(out)
    ref = torch.zeros(V, H, device=gpu, dtype=torch.float64).index_add_(0, ids, dy.double())
    assert rel_err(outs[0], ref) < (1e-5 if f32 else 5e-3)
    assert torch.equal(outs[0], outs[1])
