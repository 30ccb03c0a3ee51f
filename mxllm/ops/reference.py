"""Pure-PyTorch reference implementations of every mxllm op.

They define the semantics the HIP kernels must match, run the CPU path (gloo
plumbing runs / CPU tests), and serve as fp32 numerics oracles in the kernel
parity tests.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F


def rms_norm(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    xf = x.float()
    y = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps) * w.float()
    return y.to(x.dtype)


def llama3_inv_freq(head_dim: int, theta: float, scaling: dict | None) -> torch.Tensor:
    """Llama-3.1 RoPE frequencies (theta 500000, factor 8, low/high 1/4,
    original context 8192), computed in float64 on the host."""
    inv = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.float64) / head_dim))
    if not scaling:
        return inv
    factor = scaling.get("factor", 8.0)
    lf = scaling.get("low_freq_factor", 1.0)
    hf = scaling.get("high_freq_factor", 4.0)
    old = scaling.get("original_max_position_embeddings", 8192)
    low_wl, high_wl = old / lf, old / hf
    wl = 2 * math.pi / inv
    out = torch.where(wl > low_wl, inv / factor, inv)
    smooth = (old / wl - lf) / (hf - lf)
    mid = (1 - smooth) * out / factor + smooth * out
    is_mid = (wl >= high_wl) & (wl <= low_wl)
    return torch.where(is_mid, mid, out)


def rope_tables(seq_len: int, head_dim: int, theta: float, scaling: dict | None, device=None):
    """cos/sin tables [S, D/2] float32 (host-precomputed, guide App. B)."""
    inv = llama3_inv_freq(head_dim, theta, scaling)
    t = torch.arange(seq_len, dtype=torch.float64)
    ang = torch.outer(t, inv)
    return ang.cos().float().to(device), ang.sin().float().to(device)


def apply_rope(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """x [B, S, H, D] with the "rotate-half" (HF Llama) pairing (i, i + D/2)."""
    S, D = x.shape[1], x.shape[-1]
    c = cos[:S].view(1, S, 1, D // 2).float()
    s = sin[:S].view(1, S, 1, D // 2).float()
    xf = x.float()
    x1, x2 = xf[..., : D // 2], xf[..., D // 2:]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1).to(x.dtype)


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, causal: bool = True,
              scale: float | None = None, doc_start: torch.Tensor | None = None) -> torch.Tensor:
    """q [B, S, Hq, D], k/v [B, Sk, Hkv, D] -> o [B, S, Hq, D]  (GQA, fp32 math).
    Causal alignment is bottom-right (query i sees keys <= i + Sk - S).  ``doc_start`` [B, S] (packed
    documents, ``ops.doc_bounds``): query i also sees no key before ``doc_start[b, i]``."""
    B, S, Hq, D = q.shape
    Sk, Hkv = k.shape[1], k.shape[2]
    rep = Hq // Hkv
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    qf = q.float().transpose(1, 2)
    kf = k.float().transpose(1, 2).repeat_interleave(rep, dim=1)
    vf = v.float().transpose(1, 2).repeat_interleave(rep, dim=1)
    s = torch.matmul(qf, kf.transpose(-1, -2)) * scale
    if causal:
        i = torch.arange(S, device=q.device).view(S, 1)
        j = torch.arange(Sk, device=q.device).view(1, Sk)
        s = s.masked_fill(j > i + (Sk - S), float("-inf"))
    if doc_start is not None:
        j = torch.arange(Sk, device=q.device).view(1, 1, 1, Sk)
        s = s.masked_fill(j < doc_start.view(B, 1, S, 1), float("-inf"))
    p = torch.softmax(s, dim=-1)
    o = torch.matmul(p, vf)
    return o.transpose(1, 2).to(q.dtype)


def swiglu(gate_up: torch.Tensor) -> torch.Tensor:
    """gate_up [..., 2F] laid out [gate | up] -> silu(gate) * up  [..., F]."""
    F_ = gate_up.shape[-1] // 2
    g, u = gate_up[..., :F_].float(), gate_up[..., F_:].float()
    return (F.silu(g) * u).to(gate_up.dtype)


def cross_entropy(logits: torch.Tensor, labels: torch.Tensor, ignore_index: int = -100) -> torch.Tensor:
    """Mean over the valid tokens; no valid token: loss 0 and a zero gradient (the kernels' and the chunked
    path's clamped count), not the 0 / 0 of ``reduction="mean"``."""
    n = (labels != ignore_index).sum().clamp(min=1)
    return F.cross_entropy(logits.float(), labels, ignore_index=ignore_index, reduction="sum") / n


def adamw_(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, *, lr: float, beta1: float,
           beta2: float, eps: float, weight_decay: float, step: int, grad_scale: float = 1.0,
           p_lowp: torch.Tensor | None = None) -> None:
    """Decoupled-weight-decay Adam on fp32 master ``p`` (in place)."""
    gf = g.float() * grad_scale
    m.mul_(beta1).add_(gf, alpha=1 - beta1)
    v.mul_(beta2).addcmul_(gf, gf, value=1 - beta2)
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    p.mul_(1 - lr * weight_decay)
    denom = (v / bc2).sqrt_().add_(eps)
    p.addcdiv_(m, denom, value=-lr / bc1)
    if p_lowp is not None:
        p_lowp.copy_(p)


# ----------------------------------------------------------------- fp8 AdamW moments (mxllm/ops/optim.py QuantMoment)
# A block is Q8_BLOCK consecutive elements of the flat buffer: OCP e4m3 codes (1 sign, 4 exponent bits of bias 7,
# 3 mantissa bits; largest 448, smallest subnormal 2^-9) times 2^e with one int8 ``e`` per block.
Q8_BLOCK = 64
Q8_MAX = 448.0
Q8_MIN_EXP = -100
_M32 = 0xFFFFFFFF


def q8_exps(x: torch.Tensor) -> torch.Tensor:
    """x fp32 [nb, 64] -> int8 [nb]: the smallest e with amax / 2^e <= 448 (amax = f 2^E, 1 <= f < 2: E - 8 if
    f <= 1.75, else E - 7), at least Q8_MIN_EXP; 0 for an all-zero block (the rule of csrc/kernels/kv8.h kv8_exp)."""
    bits = x.abs().amax(1).contiguous().view(torch.int32)
    e = (bits >> 23) - 135 + ((bits & 0x7FFFFF) > 0x600000).to(torch.int32)
    e = torch.where(bits == 0, torch.zeros_like(e), e.clamp(min=Q8_MIN_EXP))
    return e.to(torch.int8)


def _pow2(k: torch.Tensor, dtype=torch.float64) -> torch.Tensor:  # 2^k from the exponent field (exact on any device)
    if dtype == torch.float32:
        return ((k.to(torch.int32) + 127) << 23).view(torch.float32)
    return ((k.to(torch.int64) + 1023) << 52).view(torch.float64)


def q8_decode(codes: torch.Tensor, exps: torch.Tensor) -> torch.Tensor:
    """codes uint8 [n], exps int8 [n / 64] -> fp32 [n] (exact)."""
    c = codes.to(torch.int32)
    ef, mf = (c >> 3) & 15, (c & 7).float()
    mag = torch.where(ef == 0, mf * 2.0 ** -9, (8.0 + mf) * _pow2(ef - 10, torch.float32))
    val = torch.where(c >= 128, -mag, mag).view(-1, Q8_BLOCK)
    return (val * _pow2(exps, torch.float32)[:, None]).reshape(-1)


def _fmix32(h: torch.Tensor) -> torch.Tensor:  # murmur3's 32-bit finalizer on int64 lanes holding uint32 values
    h = ((h ^ (h >> 16)) * 0x85EBCA6B) & _M32
    h = ((h ^ (h >> 13)) * 0xC2B2AE35) & _M32
    return h ^ (h >> 16)


def q8_key(seed: int, step: int) -> int:
    return (seed * 0x9E3779B1 + step * 0x85EBCA77) & _M32


def q8_rand20(key: int, moment: int, base: int, n: int, device=None) -> torch.Tensor:
    """20 random bits per element from a counter hash of (seed and step in ``key``, moment 0 = m / 1 = sqrt(v),
    global element index base + i): the same bits whatever the grid, the chunking or the rank."""
    idx = torch.arange(base, base + n, dtype=torch.int64, device=device)
    a = (_fmix32((idx & _M32) ^ key) + (idx >> 32) * 0x9E3779B1) & _M32
    return _fmix32((a + (0x3C6EF372, 0xDAA66D2B)[moment]) & _M32) >> 12


def q8_encode_(codes: torch.Tensor, exps: torch.Tensor, x: torch.Tensor, rand20: torch.Tensor | None = None,
               floor_min: torch.Tensor | None = None) -> None:
    """Quantise fp32 ``x`` [n] into ``codes`` / ``exps`` in place.  Per block e = q8_exps; y = |x| / 2^e lies between
    two adjacent e4m3 values lo <= y <= hi (spacing 2^(max(floor(log2 y), -6) - 3)).  ``rand20`` given (stochastic):
    y goes to hi when (y - lo) / (hi - lo) + r / 2^20 >= 1, i.e. with probability (y - lo) / (hi - lo) in steps of
    2^-20; a representable y stays.  None: round to nearest, ties to even.  ``floor_min`` (bool [n]): such an element
    is stored no smaller than the smallest subnormal (a positive sqrt(v) never flushes to a zero denominator)."""
    xb = x.float().view(-1, Q8_BLOCK)
    e = q8_exps(xb)
    y = (xb.double() * _pow2(-e.to(torch.int64))[:, None]).abs().reshape(-1)
    ex = (((y.view(torch.int64) >> 52) & 0x7FF) - 1023).clamp(min=-6)  # floor(log2 y); y = 0: -6
    t = y * _pow2(3 - ex)  # y in units of its spacing: [8, 16), or [0, 8) for subnormals
    k = torch.floor(t + rand20.double() * 2.0 ** -20) if rand20 is not None else torch.round(t)
    mag = ((ex + 6) * 8 + k.to(torch.int32)).clamp(max=126)
    if floor_min is not None:
        mag = torch.where(floor_min & (mag == 0), torch.ones_like(mag), mag)
    neg = torch.signbit(x.float().reshape(-1))
    codes.copy_((mag + torch.where(neg, 128, 0)).to(torch.uint8))
    exps.copy_(e)


def adamw8_(p: torch.Tensor, g: torch.Tensor, m_codes: torch.Tensor, m_exps: torch.Tensor, s_codes: torch.Tensor,
            s_exps: torch.Tensor, *, lr: float, beta1: float, beta2: float, eps: float, weight_decay: float, step: int,
            grad_scale: float = 1.0, p_lowp: torch.Tensor | None = None, seed: int = 0, base: int = 0) -> None:
    """AdamW with fp8 moments: decode m and s = sqrt(v), run ``adamw_`` (today's fp32 arithmetic; ``p`` comes from
    the fp32 m_new and v_new), then store m_new and sqrt(v_new) with stochastic rounding."""
    m = q8_decode(m_codes, m_exps)
    s = q8_decode(s_codes, s_exps)
    v = s * s
    adamw_(p, g, m, v, lr=lr, beta1=beta1, beta2=beta2, eps=eps, weight_decay=weight_decay, step=step,
           grad_scale=grad_scale, p_lowp=p_lowp)
    n, key = p.numel(), q8_key(seed, step)
    q8_encode_(m_codes, m_exps, m, q8_rand20(key, 0, base, n, p.device))
    q8_encode_(s_codes, s_exps, v.sqrt(), q8_rand20(key, 1, base, n, p.device), floor_min=v > 0)
