"""Fused attention block: QKV split + Llama-3 RoPE + causal GQA flash attention.

SURVEY §2.4 K6 + K7 (+K13 prefill).  The whole ``qkv -> o`` segment is ONE
autograd node so the backward can hand the attention kernel's f32 dQ and
per-q-head dK/dV partials straight to the inverse-RoPE merge kernel, which
writes d(qkv) in the projection's token-major layout — no intermediate
re-layout tensors and no autograd shape constraints between them.

GPU path (csrc/kernels/rope.hip, attn_fwd.hip, attn_bwd.hip):
  forward : qkv [T,(Hq+2Hkv)D] --rope_split--> q [B,Hq,S,D], k,v [B,Hkv,S,D]
            --attn_fwd (MFMA 32x32x16 bf16)--> o [B,S,Hq*D] token-major, lse [B,Hq,S]
  backward: attn_bwd -> dq f32 [B,Hq,S,D] (dS^T through HBM + a dQ kernel by
            default; f32-atomic and partial-sum modes selectable), dk/dv partials
            [B,Hq,S,D] f32 --rope_merge_bwd--> d(qkv) bf16 [T,(Hq+2Hkv)D]; at D = 128 the
            dQ kernel writes d(q) of d(qkv) itself (attn_bwd_rope, backward_dqkv)

Packed documents (``doc = doc_bounds(ids, eos_id)``; csrc/kernels/attn_doc.hip): query i sees key j iff
``doc_start[b, i] <= j <= i``.  Positions stay 0..S-1: RoPE is relative (and the Llama-3 scaling acts on
the frequencies), so a document's scores do not depend on where it sits in the window -- in exact
arithmetic this equals resetting ``position_ids`` per document as HF packing does.  The document route
is the split backward only (f32 dQ -> rope_merge_bwd): it honours neither ``MXLLM_ATTN_DQ_MODE`` 1 / 2
nor the RoPE-fused dQ.
"""
from __future__ import annotations

import math
import os

import torch

from . import reference as ref
from ._ext import native, use_native


def split_heads_ref(qkv: torch.Tensor, B: int, S: int, Hq: int, Hkv: int, D: int):
    x = qkv.view(B, S, Hq + 2 * Hkv, D)
    return x[:, :, :Hq], x[:, :, Hq:Hq + Hkv], x[:, :, Hq + Hkv:]


class _AttnBlockFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, cos, sin, B, S, Hq, Hkv, D, causal, out_pad, grad_pad, doc=None):
        ops = native()
        q, k, v = ops.rope_split(qkv, cos, sin, B, S, Hq, Hkv, D)
        o, lse = attn_forward(q, k, v, causal, out_pad, doc)
        ctx.save_for_backward(q, k, v, o, lse, cos, sin, *(doc or ()))
        ctx.dims = (B, S, Hq, Hkv, D, causal, grad_pad)
        return o.view(B * S, Hq * D)

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse, cos, sin, *doc = ctx.saved_tensors
        B, S, Hq, Hkv, D, causal, grad_pad = ctx.dims
        dqkv = backward_dqkv(do, q, k, v, o, lse, cos, sin, causal, grad_pad, doc=tuple(doc) or None)
        return dqkv, None, None, None, None, None, None, None, None, None, None, None


def doc_bounds(ids: torch.Tensor, eos_id: int):
    """The document tables of packed token ids [B, S]: ``(doc_start, doc_end)`` int32 [B, S] on the ids'
    device -- position s lies in the document ``[doc_start[b, s], doc_end[b, s])``.  A document starts at
    position 0 and after every EOS (the EOS belongs to the document it closes); the last one ends at S.
    Plain torch ops, no host sync."""
    B, S = ids.shape
    pos = torch.arange(S, device=ids.device, dtype=torch.int32).expand(B, S)
    eos = ids == eos_id
    first = torch.ones_like(eos)
    first[:, 1:] = eos[:, :-1]
    start = torch.where(first, pos, pos.new_zeros(())).cummax(dim=1).values
    last = eos.clone()
    last[:, -1] = True
    end = torch.where(last, pos + 1, pos.new_full((), S)).flip(1).cummin(dim=1).values.flip(1)
    return start.contiguous(), end.contiguous()


def attn_forward(q, k, v, causal: bool, out_pad: int = 0, doc=None):
    """(o, lse) of the training attention forward on the GPU: ``attn_fwd``, or ``attn_doc_fwd`` over
    packed documents (causal self-attention only)."""
    scale = 1.0 / math.sqrt(q.shape[-1])
    if doc is None:
        return native().attn_fwd(q, k, v, causal, scale, out_pad)
    if not causal:
        raise ValueError("the document mask is causal")
    return native().attn_doc_fwd(q, k, v, doc[0], scale, out_pad)


_DS_BUDGET = float(os.environ.get("MXLLM_ATTN_DS_BUDGET_GB", "4")) * 2**30


def _ds_bytes_per_head(S: int, Sk: int) -> int:
    """The dS^T image of one q head in the split mode: ``mx::ab_work_bytes`` per (batch row, q head)
    (csrc/kernels/attn_args.h; tests/test_attn_args.py holds the two together)."""
    return (Sk + 127) // 128 * 128 * ((S + 63) // 64 * 64) * 2


def attn_bwd_takes_rope(mode: int, D: int, S: int, Sk: int) -> bool:
    """Whether ``attn_bwd_rope`` takes the backward (``mx::ab_takes_rope``): split mode, D = 128,
    self-attention."""
    return mode == 3 and D == 128 and Sk == S


def backward_dqkv(do, q, k, v, o, lse, cos, sin, causal: bool, grad_pad: int = 0, doc=None) -> torch.Tensor:
    """d(qkv) [B*S, (Hq+2Hkv)*D (+grad_pad)] bf16 of the RoPE'd attention block.  The split backward at
    D = 128 writes it directly (``attn_bwd_rope``: the dQ kernel applies the inverse RoPE to d(q) and
    rounds once, rope_merge_bwd fills only the k / v columns; no fp32 dQ through HBM -- 70B training
    shape: -201 MB of traffic per layer); otherwise fp32 dQ + dK / dV partials then rope_merge_bwd.
    ``MXLLM_ATTN_DQ_ROPE=0`` forces the two-step path (A/B).  ``doc`` = (doc_start, doc_end): the
    document-masked split backward (``attn_doc_bwd``), always two-step."""
    ops = native()
    B, Hq, S, D = q.shape
    Hkv, Sk = k.shape[1], k.shape[2]
    scale = 1.0 / math.sqrt(D)
    mode = 3 if doc is not None else dq_mode()
    if (doc is None and attn_bwd_takes_rope(mode, D, S, Sk) and B * Hq * _ds_bytes_per_head(S, Sk) <= _DS_BUDGET
            and os.environ.get("MXLLM_ATTN_DQ_ROPE", "1") != "0"):
        return ops.attn_bwd_rope(do.contiguous(), q, k, v, o, lse, causal, scale, cos, sin, grad_pad)
    dq, dkp, dvp = attn_bwd(do.contiguous(), q, k, v, o, lse, causal, scale, mode, doc)
    return ops.rope_merge_bwd(dq, dkp, dvp, cos, sin, B, S, Hq, Hkv, D, grad_pad)


def attn_bwd(do, q, k, v, o, lse, causal: bool, scale: float, mode: int, doc=None):
    """``native().attn_bwd`` with bounded memory.  The split dQ mode (3) passes dS^T through an
    HBM image of B * Hq * Sk * S bf16 -- O(S^2): 1.1 GB at the 70B training shape, 64 GiB for one
    8B sequence of 32k tokens.  Above ``MXLLM_ATTN_DS_BUDGET_GB`` (4 GiB) the call runs per
    (sequence, chunk of whole KV groups), each chunk's image within the budget, writing its dQ and
    dK / dV partials into head ranges of the full outputs (a KV head's partials stay consecutive for
    rope_merge_bwd).  With ``doc`` = (doc_start, doc_end) every call is ``attn_doc_bwd`` (the same
    image; one partial per q head), a chunk's with the table rows of its sequence.
    ``do`` [B*S, Hq*D] or [B, S, Hq*D], ``o`` [B, S, Hq*D] (row-strided allowed)."""
    ops = native()
    B, Hq, S, D = q.shape
    Hkv, Sk = k.shape[1], k.shape[2]
    per_head = _ds_bytes_per_head(S, Sk)

    def run(b0, b1, do_, q_, k_, v_, o_, lse_, *outs):
        if doc is None:
            return ops.attn_bwd(do_, q_, k_, v_, o_, lse_, causal, scale, mode, *outs)
        return ops.attn_doc_bwd(do_, q_, k_, v_, o_, lse_, doc[0][b0:b1], doc[1][b0:b1], scale, *outs)

    if mode != 3 or B * Hq * per_head <= _DS_BUDGET:
        return run(0, B, do, q, k, v, o, lse)
    G = Hq // Hkv
    hpc = G  # heads per chunk: whole KV groups, a divisor of Hq (equal chunks -> equal partial layout)
    for c in range(G, Hq + 1, G):
        if Hq % c == 0 and c * per_head <= _DS_BUDGET:
            hpc = c
    do4 = do.reshape(B, S, Hq, D)
    o3 = o.view(B, S, o.shape[-1]) if o.dim() != 3 else o
    n = Hq // hpc
    dq = dk = dv = None
    for b in range(B):
        for i in range(n):
            h0, h1 = i * hpc, (i + 1) * hpc
            args = (do4[b:b + 1, :, h0:h1].contiguous(), q[b:b + 1, h0:h1], k[b:b + 1, h0 // G:h1 // G],
                    v[b:b + 1, h0 // G:h1 // G], o3[b:b + 1, :, h0 * D:h1 * D], lse[b:b + 1, h0:h1])
            if dq is None:  # first chunk: its partial-head count sizes the full dK / dV partials
                dq_c, dk_c, dv_c = run(b, b + 1, *args)
                P = dk_c.shape[1]
                dq = torch.empty(B, Hq, S, D, dtype=dq_c.dtype, device=dq_c.device)
                dk = torch.empty(B, n * P, Sk, D, dtype=dk_c.dtype, device=dk_c.device)
                dv = torch.empty_like(dk)
                dq[0:1, h0:h1].copy_(dq_c)
                dk[0:1, 0:P].copy_(dk_c)
                dv[0:1, 0:P].copy_(dv_c)
                del dq_c, dk_c, dv_c
            else:  # every other chunk writes its head range in place
                run(b, b + 1, *args, dq[b:b + 1, h0:h1], dk[b:b + 1, i * P:(i + 1) * P], dv[b:b + 1, i * P:(i + 1) * P])
    return dq, dk, dv


def dq_mode() -> int:
    """How the attention backward forms dQ (csrc/kernels/attn_bwd.hip):
    3 = split (dS^T to HBM, separate dQ kernel; fastest and deterministic, default),
    2 = per-key-block partials + ordered reduction, 1 = f32 atomics (non-deterministic).
    ``MXLLM_ATTN_DQ_MODE`` overrides; with ``torch.use_deterministic_algorithms(True)``
    or ``MXLLM_DETERMINISTIC=1`` mode 1 is never used."""
    m = int(os.environ.get("MXLLM_ATTN_DQ_MODE", "3"))
    if m == 1 and (torch.are_deterministic_algorithms_enabled() or os.environ.get("MXLLM_DETERMINISTIC") == "1"):
        m = 3
    return m


def attention_block(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, B: int, S: int, Hq: int,
                    Hkv: int, D: int, causal: bool = True, out_pad: int = 0, grad_pad: int = 0,
                    doc=None) -> torch.Tensor:
    """qkv [B*S, (Hq+2Hkv)*D] -> attention output [B*S, Hq*D] (RoPE at positions 0..S-1).
    ``out_pad`` / ``grad_pad``: padded row layouts of the output and of d(qkv)
    for LoRA-augmented GEMM neighbours (mxllm/ops/linear.py).  ``doc`` = (doc_start, doc_end) of
    ``doc_bounds``: attention inside the packed documents only."""
    if use_native(qkv):
        return _AttnBlockFn.apply(qkv.contiguous(), cos, sin, B, S, Hq, Hkv, D, causal, out_pad, grad_pad, doc)
    q, k, v = split_heads_ref(qkv, B, S, Hq, Hkv, D)
    q = ref.apply_rope(q, cos, sin)
    k = ref.apply_rope(k, cos, sin)
    o = ref.attention(q, k, v, causal=causal, doc_start=None if doc is None else doc[0])
    return o.reshape(B * S, Hq * D)
