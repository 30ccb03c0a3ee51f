"""Inference ops: prefill attention into a KV cache, decode attention, sampling.

GPU: csrc/kernels/decode.hip (rope_append, split-K decode attention, their kv8
forms over an fp8 KV cache, the multi-row verify attention of speculative decoding,
greedy / Gumbel-max sampler), sampling.hip (batched top-k / top-p / temperature, draft acceptance),
logits_proc.hip (sampling penalties, logit_bias, log-probabilities),
attn_fwd.hip for prefill and prefill_paged.hip for prefill chunks over the paged cache.
CPU: reference implementations.
"""
from __future__ import annotations

import math
import os

import torch

from . import reference as ref
from ._ext import native, use_native


def prefill_attention(qkv: torch.Tensor, cos, sin, write_kv, S: int, Hq: int, Hkv: int, D: int) -> torch.Tensor:
    """One sequence (positions 0..S-1): RoPE, hand the rotated K and V [Hkv, S, D] to
    ``write_kv(k, v)`` (the engine's KV cache), causal attention.
    qkv [S, NH*D] -> o [S, Hq*D]."""
    if use_native(qkv):
        ops = native()
        q, k, v = ops.rope_split(qkv.contiguous(), cos, sin, 1, S, Hq, Hkv, D, None)
        write_kv(k[0], v[0])
        o, _ = ops.attn_fwd(q, k, v, True, 1.0 / math.sqrt(D))
        return o.view(S, Hq * D)
    x = qkv.view(1, S, Hq + 2 * Hkv, D)
    q = ref.apply_rope(x[:, :, :Hq], cos, sin)
    k = ref.apply_rope(x[:, :, Hq:Hq + Hkv], cos, sin)
    v = x[:, :, Hq + Hkv:]
    write_kv(k[0].transpose(0, 1), v[0].transpose(0, 1))
    return ref.attention(q, k, v, causal=True).reshape(S, Hq * D)


def _kv_at(cache: torch.Tensor, bt, slot: int, p0: int, p1: int) -> torch.Tensor:
    """Rows [p0, p1) of ``slot`` as [Hkv, p1 - p0, D] (contiguous or paged cache; a view
    when they lie in one block)."""
    if bt is None:
        return cache[slot, :, p0:p1]
    blk = cache.shape[2]
    if p0 // blk == (p1 - 1) // blk:
        b = int(bt[slot, p0 // blk])
        return cache[b, :, p0 % blk:p0 % blk + (p1 - p0)]
    parts, a = [], p0
    while a < p1:
        e = min(p1, (a // blk + 1) * blk)
        parts.append(_kv_at(cache, bt, slot, a, e))
        a = e
    return torch.cat(parts, 1)


# ---------------------------------------------------------------- prefill chunks over the paged cache
class PrefillPlan:
    """The segments of one prefill pass, prepared once and reused by every layer: ``segs`` a list of
    ``(row0, n, slot, p0)`` -- rows [row0, row0 + n) of the pass are positions [p0, p0 + n) of cache
    slot ``slot`` -- over ``T`` rows.  Holds the per-row position / slot tensors ``rope_append``
    reads, the int32 [nseg, 4] host table the attention kernel's binding checks, and (gather route)
    a host copy of the block table."""

    def __init__(self, segs, T: int, device, block_table: torch.Tensor | None = None):
        self.segs = [tuple(int(x) for x in s) for s in segs]
        self.T = int(T)
        for row0, n, slot, p0 in self.segs:
            if n <= 0 or row0 < 0 or row0 + n > self.T or p0 < 0 or slot < 0:
                raise ValueError(f"bad prefill segment {(row0, n, slot, p0)} over {self.T} rows")
        order = sorted(self.segs)
        if any(b[0] < a[0] + a[1] for a, b in zip(order, order[1:])):
            raise ValueError("prefill segments overlap")
        self.table = torch.tensor(self.segs, dtype=torch.int32).reshape(-1, 4)
        # all rows covered in order: one rope_append launch over the pass
        self.dense = sum(s[1] for s in self.segs) == self.T
        pos = torch.zeros(self.T, dtype=torch.int32)
        slots = torch.zeros(self.T, dtype=torch.int32)
        for row0, n, slot, p0 in self.segs:
            pos[row0:row0 + n] = torch.arange(p0, p0 + n, dtype=torch.int32)
            slots[row0:row0 + n] = slot
        device = torch.device(device)
        if device.type == "cuda":
            pos, slots = pos.pin_memory().to(device, non_blocking=True), slots.pin_memory().to(device, non_blocking=True)
        self.pos, self.slots = pos, slots
        self.bt_host = block_table.cpu() if block_table is not None else None


def prefill_paged_route(D: int, Hq: int, Hkv: int, blk: int, dtype) -> str:
    """GPU route of ``prefill_attention_paged``: "hip" (csrc/kernels/prefill_paged.hip) where the
    kernel takes the launch -- bf16, head_dim 128, whole GQA groups of at most 16, a block size
    that is a multiple of 256 -- else "gather".  ``MXLLM_PREFILL_PAGED=hip|gather`` forces one;
    a forced "hip" that the kernel does not take is an error, not a fall-back."""
    env = os.environ.get("MXLLM_PREFILL_PAGED", "")
    if env:
        if env not in ("hip", "gather"):
            raise ValueError(f"MXLLM_PREFILL_PAGED must be hip or gather, got {env!r}")
        return env
    takes = dtype == torch.bfloat16 and D == 128 and Hkv > 0 and Hq % Hkv == 0 and Hq // Hkv <= 16 and blk % 256 == 0
    return "hip" if takes else "gather"


def paged_attention_gather(q: torch.Tensor, k_cache, v_cache, bt_host, segs, scale: float,
                           out: torch.Tensor) -> torch.Tensor:
    """The gather route of ``prefill_attention_paged`` (GPU, any head dim ``attn_fwd`` takes): per
    segment ``(row0, n, slot, p0)`` the rows [0, p0 + n) of the slot are made contiguous (``_kv_at``
    through the HOST block table) and fed to ``attn_fwd`` with Sk = p0 + n > S = n, whose causal
    offset Sk - S is p0.  q [T, Hq, D] (rope_append's output) -> rows of ``out`` [T, Hq * D]."""
    ops = native()
    Hq, D = q.shape[1], q.shape[2]
    for row0, n, slot, p0 in segs:
        kk = _kv_at(k_cache, bt_host, slot, 0, p0 + n).contiguous().unsqueeze(0)
        vv = _kv_at(v_cache, bt_host, slot, 0, p0 + n).contiguous().unsqueeze(0)
        qs = q[row0:row0 + n].transpose(0, 1).contiguous().unsqueeze(0)  # [1, Hq, n, D]
        o, _ = ops.attn_fwd(qs, kk, vv, True, scale)
        out[row0:row0 + n] = o.view(n, Hq * D)
    return out


def prefill_attention_paged(qkv: torch.Tensor, cos, sin, k_cache, v_cache, block_table, segs, Hq: int, Hkv: int,
                            D: int, out: torch.Tensor | None = None) -> torch.Tensor:
    """Prefill chunks over the paged KV cache.  qkv [T, NH*D]; ``segs`` a host list of
    ``(row0, n, slot, p0)`` (or a ``PrefillPlan`` of it, built once per pass): rows
    [row0, row0 + n) are positions [p0, p0 + n) of cache slot ``slot``.  RoPE and the cache append
    of every segment row (``rope_append``, pos = p0 + t), then causal attention of each segment
    over rows [0, p0 + n) of its slot, which now hold the chunk's own K/V: row t sees keys
    0 .. p0 + t.  -> o [T, Hq*D]; rows outside every segment are not written (``out`` keeps them).

    GPU routes (``prefill_paged_route``): "hip" -- one launch of the paged flash-attention kernel
    for all segments; "gather" -- per segment, rows [0, p0 + n) made contiguous (``_kv_at``) and
    ``attn_fwd`` with Sk > S (its causal offset Sk - S is p0).  CPU: the fp32 softmax expression."""
    T = qkv.shape[0]
    plan = segs if isinstance(segs, PrefillPlan) else PrefillPlan(segs, T, qkv.device)
    if plan.T != T:
        raise ValueError(f"the plan covers {plan.T} rows, qkv has {T}")
    scale = 1.0 / math.sqrt(D)
    if out is None:
        out = torch.empty(T, Hq * D, dtype=qkv.dtype, device=qkv.device)
    if not plan.segs:
        return out
    if use_native(qkv):
        ops = native()
        route = prefill_paged_route(D, Hq, Hkv, k_cache.shape[2], qkv.dtype)
        qkv = qkv.contiguous()
        if plan.dense:
            q = ops.rope_append(qkv, cos, sin, plan.pos, plan.slots, k_cache, v_cache, Hq, Hkv, D, block_table)
        else:  # rows in no segment are neither rotated nor appended
            q = torch.empty(T, Hq, D, dtype=qkv.dtype, device=qkv.device)
            for row0, n, _, _ in plan.segs:
                q[row0:row0 + n] = ops.rope_append(qkv[row0:row0 + n], cos, sin, plan.pos[row0:row0 + n].contiguous(),
                                                   plan.slots[row0:row0 + n].contiguous(), k_cache, v_cache, Hq, Hkv,
                                                   D, block_table)
        if route == "hip":
            return ops.prefill_attn_paged(q, k_cache, v_cache, block_table, plan.table, scale, out)
        if plan.bt_host is None:
            plan.bt_host = block_table.cpu()
        return paged_attention_gather(q, k_cache, v_cache, plan.bt_host, plan.segs, scale, out)
    bt = block_table.cpu() if block_table is not None else None
    x = qkv.view(T, Hq + 2 * Hkv, D).float()
    for row0, n, slot, p0 in plan.segs:
        c = cos[p0:p0 + n].view(n, 1, D // 2).float()
        sn = sin[p0:p0 + n].view(n, 1, D // 2).float()

        def rot(t):
            t1, t2 = t[..., : D // 2], t[..., D // 2:]
            return torch.cat([t1 * c - t2 * sn, t2 * c + t1 * sn], -1)

        xs = x[row0:row0 + n]
        qi = rot(xs[:, :Hq]).to(qkv.dtype).float()  # [n, Hq, D], rounded as rope_append stores it
        ki = rot(xs[:, Hq:Hq + Hkv]).to(k_cache.dtype)
        vi = qkv.view(T, Hq + 2 * Hkv, D)[row0:row0 + n, Hq + Hkv:].to(v_cache.dtype)
        blk = k_cache.shape[2] if bt is not None else None
        a = 0
        while a < n:  # the chunk's own rows, block by block
            e = n if blk is None else min(n, ((p0 + a) // blk + 1) * blk - p0)
            _kv_at(k_cache, bt, slot, p0 + a, p0 + e).copy_(ki[a:e].transpose(0, 1))
            _kv_at(v_cache, bt, slot, p0 + a, p0 + e).copy_(vi[a:e].transpose(0, 1))
            a = e
        kk = _kv_at(k_cache, bt, slot, 0, p0 + n).float().repeat_interleave(Hq // Hkv, 0)  # [Hq, L, D]
        vv = _kv_at(v_cache, bt, slot, 0, p0 + n).float().repeat_interleave(Hq // Hkv, 0)
        sc = torch.einsum("nhd,hld->hnl", qi, kk) * scale
        key = torch.arange(p0 + n).view(1, 1, -1)
        row = torch.arange(n).view(1, -1, 1)
        sc = sc.masked_fill(key > row + p0, float("-inf"))
        out[row0:row0 + n] = torch.einsum("hnl,hld->nhd", sc.softmax(-1), vv).reshape(n, Hq * D).to(out.dtype)
    return out


# ---------------------------------------------------------------- kv8: the fp8 (e4m3) KV cache
# Row format and CPU codec: mxllm/serve/quant.py (kv8_quantize / kv8_dequantize).  Pools of one
# layer: codes uint8 [rows, Hkv, SEQ, 128] and scales f32 [rows, Hkv, SEQ], for K and for V.
def _kv8_codec():
    from ..serve.quant import kv8_dequantize, kv8_quantize

    return kv8_quantize, kv8_dequantize


def kv8_quant_rows(x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """bf16 rows [R, 128] (row stride a multiple of 8) -> (codes uint8 [R, 128], scale f32 [R])."""
    if use_native(x):
        return native().kv8_quant_rows(x)
    return _kv8_codec()[0](x)


def _pool_rows(cache, bt, slots, pos):
    """Index tensors (first index [B], row [B]) of position pos[b] of slots[b] (None: b)."""
    B = pos.shape[0]
    p = pos.long().cpu()
    s = slots.long().cpu() if slots is not None else torch.arange(B)
    if bt is None:
        return s, p
    blk = cache.shape[2]
    return bt.cpu().long()[s, p // blk], p % blk


def rope_append_kv8(qkv: torch.Tensor, cos, sin, pos, slots, k_codes, k_scale, v_codes, v_scale, Hq: int, Hkv: int,
                    block_table: torch.Tensor | None = None) -> torch.Tensor:
    """``rope_append`` into a kv8 cache: the K row rotated and rounded to bf16 as ``rope_append``
    stores it, then K and V rows quantised (``kv8_quantize``) into the four pools at ``pos``.
    Returns the rotated q [B, Hq, 128] bf16.  head_dim 128."""
    if use_native(qkv):
        return native().rope_append_kv8(qkv.contiguous(), cos, sin, pos, slots, k_codes, k_scale, v_codes, v_scale,
                                        Hq, Hkv, block_table)
    D = 128
    if qkv.shape[1] != (Hq + 2 * Hkv) * D or k_codes.shape[-1] != D:
        raise ValueError("rope_append_kv8: the fp8 KV cache supports head_dim 128 only")
    quant = _kv8_codec()[0]
    B = qkv.shape[0]
    x = qkv.view(B, Hq + 2 * Hkv, D).float()
    c, sn = cos[pos.long()].view(B, 1, D // 2), sin[pos.long()].view(B, 1, D // 2)

    def rot(t):
        t1, t2 = t[..., : D // 2], t[..., D // 2:]
        return torch.cat([t1 * c - t2 * sn, t2 * c + t1 * sn], -1).to(qkv.dtype)

    i0, r = _pool_rows(k_codes, block_table, slots, pos)
    for codes, scale, rows in ((k_codes, k_scale, rot(x[:, Hq:Hq + Hkv])), (v_codes, v_scale, qkv.view(B, -1, D)[:, Hq + Hkv:])):
        cd, sc = quant(rows)
        codes[i0, :, r] = cd
        scale[i0, :, r] = sc
    return rot(x[:, :Hq])


def decode_attn_kv8(q: torch.Tensor, k_codes, k_scale, v_codes, v_scale, lens, slots, max_len: int, scale: float,
                    len_off: int = 0, block_table: torch.Tensor | None = None) -> torch.Tensor:
    """``decode_attn`` over a kv8 cache: q [B, Hq, 128] bf16 attends over the first
    ``lens[b] + len_off`` rows of slot ``slots[b]`` -> [B, Hq * 128] bf16.  The CPU path is the
    fp32 softmax expression on the dequantised rows."""
    if use_native(q):
        return native().decode_attn_kv8(q, k_codes, k_scale, v_codes, v_scale, lens, slots, max_len, scale, len_off,
                                        block_table)
    if q.shape[-1] != 128 or k_codes.shape[-1] != 128:
        raise ValueError("decode_attn_kv8: the fp8 KV cache supports head_dim 128 only")
    deq = _kv8_codec()[1]
    bt = block_table.cpu() if block_table is not None else None
    B, Hq, D = q.shape
    Hkv = k_codes.shape[1]
    out = torch.zeros(B, Hq * D, dtype=q.dtype)
    for i in range(B):
        L, s = int(lens[i]) + len_off, int(slots[i]) if slots is not None else i
        if L <= 0:
            continue
        kk = deq(_kv_at(k_codes, bt, s, 0, L), _kv_at(k_scale, bt, s, 0, L)).float().repeat_interleave(Hq // Hkv, 0)
        vv = deq(_kv_at(v_codes, bt, s, 0, L), _kv_at(v_scale, bt, s, 0, L)).float().repeat_interleave(Hq // Hkv, 0)
        sc = torch.einsum("hd,hld->hl", q[i].float(), kk) * scale
        out[i] = torch.einsum("hl,hld->hd", sc.softmax(-1), vv).reshape(-1).to(q.dtype)
    return out


def decode_attention(qkv: torch.Tensor, cos, sin, k_cache, v_cache, pos: torch.Tensor, slots: torch.Tensor,
                     Hq: int, Hkv: int, D: int, max_len: int, block_table: torch.Tensor | None = None,
                     counters: torch.Tensor | None = None, k_scale: torch.Tensor | None = None,
                     v_scale: torch.Tensor | None = None) -> torch.Tensor:
    """Batched single-token step.  qkv [B, NH*D], pos/slots int32 [B] (pos = index
    of the new token).  Appends K/V at ``pos`` and attends over ``pos + 1`` keys.
    ``block_table`` [slots, max_blocks] int32: paged caches [blocks, Hkv, block, D].
    ``counters``: zeroed int32 [>= B * Hkv] owned by the caller — the split-K
    partials then merge inside the attention launch (no combine kernel).
    ``k_scale`` / ``v_scale``: the caches are kv8 code pools with these scale pools (fp8 KV
    cache, head_dim 128; ``counters`` is not used there)."""
    if k_scale is not None or v_scale is not None:
        if k_scale is None or v_scale is None:
            raise ValueError("decode_attention: a kv8 cache needs both k_scale and v_scale")
        if D != 128:
            raise ValueError(f"decode_attention: the fp8 KV cache supports head_dim 128 only, got {D}")
        q = rope_append_kv8(qkv, cos, sin, pos, slots, k_cache, k_scale, v_cache, v_scale, Hq, Hkv, block_table)
        return decode_attn_kv8(q, k_cache, k_scale, v_cache, v_scale, pos, slots, max_len, 1.0 / math.sqrt(D), 1,
                               block_table)
    if use_native(qkv):
        ops = native()
        q = ops.rope_append(qkv.contiguous(), cos, sin, pos, slots, k_cache, v_cache, Hq, Hkv, D, block_table)
        return ops.decode_attn(q, k_cache, v_cache, pos, slots, max_len, 1.0 / math.sqrt(D), 1, block_table,
                               counters)
    bt = block_table.cpu() if block_table is not None else None
    B = qkv.shape[0]
    x = qkv.view(B, Hq + 2 * Hkv, D).float()
    outs = []
    for i in range(B):
        p, s = int(pos[i]), int(slots[i])
        c = cos[p].view(1, D // 2)
        sn = sin[p].view(1, D // 2)

        def rot(t):
            t1, t2 = t[..., : D // 2], t[..., D // 2:]
            return torch.cat([t1 * c - t2 * sn, t2 * c + t1 * sn], -1)

        qi = rot(x[i, :Hq])
        ki = rot(x[i, Hq:Hq + Hkv])
        _kv_at(k_cache, bt, s, p, p + 1)[:, 0] = ki.to(k_cache.dtype)
        _kv_at(v_cache, bt, s, p, p + 1)[:, 0] = x[i, Hq + Hkv:].to(v_cache.dtype)
        kk = _kv_at(k_cache, bt, s, 0, p + 1).float().repeat_interleave(Hq // Hkv, 0)  # [Hq, L, D]
        vv = _kv_at(v_cache, bt, s, 0, p + 1).float().repeat_interleave(Hq // Hkv, 0)
        sc = torch.einsum("hd,hld->hl", qi, kk) / math.sqrt(D)
        outs.append(torch.einsum("hl,hld->hd", sc.softmax(-1), vv).reshape(-1))
    return torch.stack(outs).to(qkv.dtype)


# ---------------------------------------------------------------- speculative decoding: verify + accept
def verify_attn(q: torch.Tensor, k_cache, v_cache, lens, nq, slots, n: int, max_len: int, scale: float,
                block_table: torch.Tensor | None = None, k_scale: torch.Tensor | None = None,
                v_scale: torch.Tensor | None = None) -> torch.Tensor:
    """Decode attention for up to ``n`` consecutive query rows per sequence.  q [B * n, Hq, D]: row
    ``b * n + j`` is the query at position ``lens[b] + j`` of cache slot ``slots[b]`` (None: b), for
    ``j < nq[b]``; the rows' K/V are in the cache already and row j sees keys 0 .. lens[b] + j.
    -> [B * n, Hq * D]; rows ``j >= nq[b]`` are zeros.  ``k_scale`` / ``v_scale``: kv8 pools.

    GPU: ``verify_attn`` / ``verify_attn_kv8`` (csrc/kernels/decode.hip): the K/V of a sequence are
    streamed once for all its rows, and row j is bit for bit ``decode_attn`` / ``decode_attn_kv8`` of
    that row as a sequence of its own (lens[b] + j, len_off 1, the same ``max_len``).  bf16,
    head_dim 128, n * (Hq / Hkv) <= 32 (``mx::vf_takes``); anything else is an error.
    CPU: the fp32 softmax expression per row (kv8: over the dequantised rows)."""
    if (k_scale is None) != (v_scale is None):
        raise ValueError("verify_attn: a kv8 cache needs both k_scale and v_scale")
    if use_native(q):
        if k_scale is not None:
            return native().verify_attn_kv8(q, k_cache, k_scale, v_cache, v_scale, lens, nq, slots, n, max_len, scale,
                                            block_table)
        return native().verify_attn(q, k_cache, v_cache, lens, nq, slots, n, max_len, scale, block_table)
    R, Hq, D = q.shape
    if n < 1 or R % n:
        raise ValueError(f"verify_attn: q has {R} rows, not a multiple of n = {n}")
    deq = _kv8_codec()[1] if k_scale is not None else None
    bt = block_table.cpu() if block_table is not None else None
    Hkv = k_cache.shape[1]
    out = torch.zeros(R, Hq * D, dtype=q.dtype)
    for b in range(R // n):
        L0, s = int(lens[b]), int(slots[b]) if slots is not None else b
        for j in range(min(max(int(nq[b]), 0), n)):
            L = L0 + j + 1
            kk, vv = _kv_at(k_cache, bt, s, 0, L), _kv_at(v_cache, bt, s, 0, L)
            if deq is not None:
                kk, vv = deq(kk, _kv_at(k_scale, bt, s, 0, L)), deq(vv, _kv_at(v_scale, bt, s, 0, L))
            kk, vv = kk.float().repeat_interleave(Hq // Hkv, 0), vv.float().repeat_interleave(Hq // Hkv, 0)
            sc = torch.einsum("hd,hld->hl", q[b * n + j].float(), kk) * scale
            out[b * n + j] = torch.einsum("hl,hld->hd", sc.softmax(-1), vv).reshape(-1).to(q.dtype)
    return out


def verify_attention(qkv: torch.Tensor, cos, sin, k_cache, v_cache, pos: torch.Tensor, slots: torch.Tensor,
                     lens: torch.Tensor, nq: torch.Tensor, seq_slots: torch.Tensor, n: int, Hq: int, Hkv: int, D: int,
                     max_len: int, block_table: torch.Tensor | None = None, k_scale: torch.Tensor | None = None,
                     v_scale: torch.Tensor | None = None, q: torch.Tensor | None = None) -> torch.Tensor:
    """The attention of a verify step: ``n`` rows per sequence, qkv [B * n, NH*D].  ``pos`` /
    ``slots`` int32 [B * n]: where each ROW's K/V are appended (a row that is not in use points at a
    scratch slot); ``lens`` / ``nq`` / ``seq_slots`` int32 [B]: each SEQUENCE's length before the
    step, its rows in use and its slot.  RoPE and the cache append of every row (``rope_append`` /
    ``rope_append_kv8``), then ``verify_attn``.  ``q``: the rotated queries when the QKV GEMM's
    epilogue has done the RoPE and the append already."""
    scale = 1.0 / math.sqrt(D)
    if q is None:
        if k_scale is not None:
            if D != 128:
                raise ValueError(f"verify_attention: the fp8 KV cache supports head_dim 128 only, got {D}")
            q = rope_append_kv8(qkv, cos, sin, pos, slots, k_cache, k_scale, v_cache, v_scale, Hq, Hkv, block_table)
        elif use_native(qkv):
            q = native().rope_append(qkv.contiguous(), cos, sin, pos, slots, k_cache, v_cache, Hq, Hkv, D, block_table)
        else:  # decode_attention's CPU expression: q stays fp32, K rounded to the cache's type
            R = qkv.shape[0]
            x = qkv.view(R, Hq + 2 * Hkv, D).float()
            c, sn = cos[pos.long()].view(R, 1, D // 2).float(), sin[pos.long()].view(R, 1, D // 2).float()

            def rot(t):
                t1, t2 = t[..., : D // 2], t[..., D // 2:]
                return torch.cat([t1 * c - t2 * sn, t2 * c + t1 * sn], -1)

            q, kr = rot(x[:, :Hq]), rot(x[:, Hq:Hq + Hkv])
            bt = block_table.cpu() if block_table is not None else None
            for r in range(R):
                p, s = int(pos[r]), int(slots[r])
                _kv_at(k_cache, bt, s, p, p + 1)[:, 0] = kr[r].to(k_cache.dtype)
                _kv_at(v_cache, bt, s, p, p + 1)[:, 0] = x[r, Hq + Hkv:].to(v_cache.dtype)
            return verify_attn(q, k_cache, v_cache, lens, nq, seq_slots, n, max_len, scale, block_table).to(qkv.dtype)
    return verify_attn(q, k_cache, v_cache, lens, nq, seq_slots, n, max_len, scale, block_table, k_scale, v_scale)


def spec_accept(drawn: torch.Tensor, tokens: torch.Tensor, nq: torch.Tensor) -> torch.Tensor:
    """Acceptance of deterministic drafts.  Sequence b fed ``tokens[b, :nq[b]]`` to its rows (row 0:
    its last token, rows 1..: the drafts) and drew ``drawn[b, j]`` on row j.  The proposal is one-hot,
    so exact speculative sampling reduces to: draft j + 1 is accepted iff every row before it was
    and ``drawn[b, j] == tokens[b, j + 1]``.  drawn, tokens int64 [B, n], nq int32 [B] ->
    int32 [B, n + 1]: ``out[b, 0] = a``, the number of accepted drafts (-1 for ``nq[b] <= 0``),
    ``out[b, 1 : a + 2]`` the tokens the step emits (the draws of rows 0 .. a: the accepted drafts,
    then the correction or bonus token), the rest -1.  GPU: csrc/kernels/sampling.hip."""
    if drawn.dim() != 2 or tokens.shape != drawn.shape or nq.numel() != drawn.shape[0]:
        raise ValueError("spec_accept: drawn and tokens [B, n], nq [B]")
    if use_native(drawn):
        return native().spec_accept(drawn.to(torch.long).contiguous(), tokens.to(drawn.device, torch.long).contiguous(),
                                    nq.to(drawn.device, torch.int32).contiguous())
    B, n = drawn.shape
    out = torch.full((B, n + 1), -1, dtype=torch.int32)
    for b in range(B):
        m = min(int(nq[b]), n)
        if m <= 0:
            continue
        a = 0
        while a + 1 < m and int(drawn[b, a]) == int(tokens[b, a + 1]):
            a += 1
        out[b, 0] = a
        out[b, 1:a + 2] = drawn[b, :a + 1].to(torch.int32)
    return out


def sample(logits: torch.Tensor, temperature: float = 0.0, seed: int = 0, step: int = 0,
           top_p: float = 1.0, top_k: int = 0) -> torch.Tensor:
    """logits [B, V] -> token ids [B] int64, every row with the same parameters
    (see ``sample_rows``)."""
    B = logits.shape[0]
    return sample_rows(logits, [temperature] * B, [top_p] * B, [top_k] * B, [seed] * B, [step] * B)


def sample_rows(logits: torch.Tensor, temps, top_ps, top_ks, seeds, steps) -> torch.Tensor:
    """Batched sampling with per-row parameters (OpenAI semantics): softmax of
    logits / T, keep the top_k most likely (k <= 0: all), then the smallest
    most-likely prefix whose mass reaches top_p, renormalise, draw; T <= 0 is
    greedy.  GPU: ONE launch for the whole batch (csrc/kernels/sampling.hip:
    radix-select thresholds + Gumbel-max over the kept set, keyed by
    (seed, step, token) so a request's draws do not depend on batching).
    CPU: ``filter_probs`` + torch.multinomial.  ``top_p <= 0`` (an empty nucleus)
    is the limit of a vanishing nucleus: that row is sampled greedily on both paths;
    a NaN top_p / temperature is rejected."""
    B = logits.shape[0]
    temps, top_ps = list(temps), list(top_ps)
    for i, (t, p) in enumerate(zip(temps, top_ps)):
        if p != p or t != t:
            raise ValueError(f"row {i}: top_p={p}, temperature={t} (NaN)")
        if p <= 0:
            temps[i], top_ps[i] = 0.0, 1.0
    if use_native(logits):
        ops = native()
        x = logits if logits.dtype in (torch.bfloat16, torch.float32) else logits.float()
        x = x.contiguous()
        if all(t <= 0 for t in temps):
            return ops.sample(x, 0.0, 0, 0)  # batched greedy: one argmax pass
        dev = logits.device
        prm = torch.tensor([[float(t), float(p), float(k)] for t, p, k in zip(temps, top_ps, top_ks)],
                           dtype=torch.float32).pin_memory().to(dev, non_blocking=True)
        st = torch.tensor([[int(sd), int(sp)] for sd, sp in zip(seeds, steps)], dtype=torch.int64).pin_memory()
        st = st.to(dev, non_blocking=True)
        if all(p >= 1.0 for p in top_ps) and all(k <= 0 for k in top_ks):
            # temperature / greedy rows only: the vocabulary-split kernel (same draws)
            return ops.sample_temp_rows(x, prm[:, 0].contiguous(), st[:, 0].contiguous(), st[:, 1].int().contiguous())
        return ops.sample_rows(x, prm[:, 0].contiguous(), prm[:, 1].contiguous(), prm[:, 2].int().contiguous(),
                               st[:, 0].contiguous(), st[:, 1].int().contiguous())
    out = torch.empty(B, dtype=torch.long)
    for i in range(B):
        if temps[i] <= 0:
            out[i] = logits[i].float().argmax()
            continue
        g = torch.Generator(device=logits.device)
        g.manual_seed(int(seeds[i]) * 1000003 + int(steps[i]))
        pr = filter_probs(logits[i], temps[i], top_ks[i], top_ps[i])
        out[i] = torch.multinomial(pr, 1, generator=g)[0]
    return out.to(logits.device)


def filter_probs(row: torch.Tensor, temperature: float, top_k: int = 0, top_p: float = 1.0) -> torch.Tensor:
    """fp32 reference of the sampling distribution of one logits row: softmax(row / T)
    restricted to the top_k most likely tokens, then to the smallest most-likely
    prefix reaching top_p of that mass (the crossing token kept), renormalised.
    Ties at a boundary are kept (the GPU kernel's threshold semantics)."""
    x = row.float() / max(float(temperature), 1e-20)
    keep = torch.ones_like(x, dtype=torch.bool)
    if 0 < top_k < x.numel():
        kth = torch.topk(x, top_k).values[-1]
        keep &= x >= kth
    p = torch.softmax(x.masked_fill(~keep, float("-inf")), -1)
    if top_p < 1.0:
        srt, idx = torch.sort(p, descending=True)
        before = srt.cumsum(0) - srt  # mass strictly above each token
        cut = srt[(before < top_p * srt.sum()).nonzero().max()]  # smallest kept probability
        keep &= p >= cut
        p = torch.softmax(x.masked_fill(~keep, float("-inf")), -1)
    return p


# ---------------------------------------------------------------- penalties, logit_bias, logprobs
# Token state of a request (int32 [n_slots, V]): bits 0..30 count the token's occurrences in
# the request's output, bit 31 says that it occurs in the prompt.
PROMPT_FLAG = -(1 << 31)
COUNT_MASK = 0x7FFFFFFF
TOP_LOGPROBS_MAX = 20


def _row_param(v, dtype, device) -> torch.Tensor:
    if isinstance(v, torch.Tensor):
        return v.to(device=device, dtype=dtype).contiguous()
    t = torch.tensor(list(v), dtype=dtype)
    if device.type == "cuda":
        t = t.pin_memory().to(device, non_blocking=True)
    return t


def adjust_logits_rows(logits: torch.Tensor, state, slots, presence, frequency, repetition,
                       bias=None) -> torch.Tensor:
    """Sampling penalties and logit_bias: logits [B, V] (bf16 / f32) -> f32 [B, V].

    ``state`` int32 [n_slots, V] (``PROMPT_FLAG`` / ``COUNT_MASK``; None: no token seen), ``bias``
    f32 [n_slots, V] or None, ``slots`` [B] the row of both tables that belongs to each logits row
    (< 0: the row is only converted), ``presence`` / ``frequency`` / ``repetition`` [B].
    Per element, in this order, every fp32 operation rounded on its own:

      1. x = float(logit)
      2. token in the prompt or the output, repetition != 1: x = x / repetition if x > 0 else
         x * repetition  (HF / vLLM repetition penalty: prompt and output tokens)
      3. output count c > 0: x = x - (frequency * float(c) + presence)  (OpenAI: output tokens only)
      4. bias != 0: x = x + bias

    An element that no step touches is the input converted to f32 bit for bit (-0.0 stays -0.0).
    GPU: one elementwise launch (csrc/kernels/logits_proc.hip); the CPU expression below gives the
    same bits."""
    dev = logits.device
    sl = _row_param(slots, torch.int32, dev)
    pres = _row_param(presence, torch.float32, dev)
    freq = _row_param(frequency, torch.float32, dev)
    rep = _row_param(repetition, torch.float32, dev)
    if use_native(logits):
        x = logits if logits.dtype in (torch.bfloat16, torch.float32) else logits.float()
        return native().logits_adjust_rows(x.contiguous(), state, sl, pres, freq, rep, bias)
    x = logits.float().clone()
    B, V = x.shape
    live = (sl >= 0).view(B, 1)
    idx = sl.clamp(min=0).long()
    if state is not None:
        st = state[idx]
        cnt = st & COUNT_MASK
        r = rep.view(B, 1).expand(B, V)
        pen = torch.where(x > 0, x / r, x * r)
        x = torch.where(live & (st != 0) & (r != 1), pen, x)
        sub = x - (freq.view(B, 1) * cnt.float() + pres.view(B, 1))
        x = torch.where(live & (cnt > 0), sub, x)
    if bias is not None:
        bb = bias[idx]
        x = torch.where(live & (bb != 0), x + bb, x)
    return x


def token_state_update(state: torch.Tensor, slots, ids: torch.Tensor) -> None:
    """Count the tokens just drawn: ``state[slots[b], ids[b]] += 1`` in place (rows with
    ``slots[b] < 0`` skipped)."""
    sl = _row_param(slots, torch.int32, state.device)
    if use_native(state):
        native().token_state_update(state, sl, ids.to(state.device, torch.long).contiguous())
        return
    for s_, t in zip(sl.tolist(), ids.tolist()):
        if s_ >= 0:
            state[s_, t] += 1


def logprob_rows(logits: torch.Tensor, ids: torch.Tensor, n_top):
    """Log-probabilities of the chosen token ``ids[b]`` and of the ``n_top[b]`` most likely
    tokens of every logits row: (chosen_lp f32 [B], top_ids int32 [B, 20], top_lp f32 [B, 20]).

    fp32 log-softmax: lse = max + log(sum exp(x - max)), logprob = x - lse.  The top list is in
    descending order, ties broken by the LOWER token id (the greedy sampler's rule, so for a
    greedy row top_ids[:, 0] is the sampled id and top_lp[:, 0] == chosen_lp bit for bit).
    ``n_top[b]`` in 0..20; -1 skips the row.  Skipped rows and entries beyond ``n_top`` hold
    -1 / -inf.  GPU: csrc/kernels/logits_proc.hip, one workgroup per row, no float atomics."""
    dev = logits.device
    nt = _row_param(n_top, torch.int32, dev)
    if use_native(logits):
        x = logits if logits.dtype in (torch.bfloat16, torch.float32) else logits.float()
        return native().logprob_rows(x.contiguous(), ids.to(dev, torch.long).contiguous(), nt)
    x = logits.float()
    B, V = x.shape
    chosen = torch.full((B,), float("-inf"))
    top_ids = torch.full((B, TOP_LOGPROBS_MAX), -1, dtype=torch.int32)
    top_lp = torch.full((B, TOP_LOGPROBS_MAX), float("-inf"))
    for b, n in enumerate(nt.tolist()):
        if n < 0:
            continue
        row = x[b]
        mx = row.max()
        lse = mx + torch.log(torch.exp(row - mx).sum())
        chosen[b] = row[int(ids[b])] - lse
        n = min(n, TOP_LOGPROBS_MAX, V)
        if n > 0:
            order = torch.sort(row, descending=True, stable=True).indices[:n]  # equal values: lower id first
            top_ids[b, :n] = order.to(torch.int32)
            top_lp[b, :n] = row[order] - lse
    return chosen, top_ids, top_lp
