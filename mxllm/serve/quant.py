"""FP8 (OCP e4m3) weight-only quantisation for serving (MI355X / gfx950).

Decode is bound by streaming every projection weight once per step (the bf16
GEMMs already run at ~5.6 TB/s), so 1-byte weights roughly halve the step time
of the memory-bound phase and the weight footprint (70B: 141 -> 70 GB, leaving
more HBM for the KV cache).  Activations stay bf16; the HIP kernel
(``csrc/kernels/fp8_gemm.hip``) dequantises 16 weights per lane in registers and
feeds bf16 MFMAs, and applies the per-output-channel scale in its epilogue.

Format: per output channel n, ``scale[n] = amax(|W[n, :]|) / 448`` and
``q[n, k] = e4m3(W[n, k] / scale[n])`` (round to nearest even, saturating).
Codes whose exponent field would be 0 (zero and subnormals, |W/scale| < 2^-6)
are stored as the smallest normal of the same sign: that error is at most
2^-6 * scale (<= 1/28672 of the row's largest weight) and it lets the kernel
decode every byte with four integer ALU operations and no special cases.

Up to ``SMALL_M`` tokens per call (small decode batches) the projection runs on the
weight-only HIP kernel with bf16 activations; larger calls quantise the activations
per token as well and use hipBLASLt's fp8 GEMM (``torch._scaled_mm``, row-wise
scales).  Training never uses this path (the fine-tuning benchmark is bf16 end to
end).

MXFP4 (OCP Microscaling, 4.25 bits per weight; ``--weights mxfp4``) halves the weight
bytes once more: the format, :func:`quantize_mxfp4`, :class:`W4Linear` and
:func:`quantize_model_mxfp4_` are further down, the HIP kernel is
``csrc/kernels/mxfp4_gemm.hip``.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn

from ..ops._ext import native, use_native

E4M3_MAX = 448.0
# Calls of up to SMALL_M tokens use the weight-only HIP kernel (bf16 activations, the fp8
# weights streamed once per call); larger calls quantise the activations per token too
# and run hipBLASLt's fp8 MFMA GEMM (W8A8).  The threshold is aligned to the graphed
# decode's power-of-two batch buckets (mxllm/serve/engine.py), which is where it was
# measured (70B decode step, archive/profiles/r1g_fp8_decode_ab.md): the 8-row bucket 21.1 ms on
# the HIP kernel vs 27.7 ms on hipBLASLt, the 16-row bucket (9..16 live sequences; the
# profile's "12 tokens" row also ran 16-row GEMMs) 25.2 vs 24.6 ms.  Eager calls with 9..15
# rows were not measured separately.  Decode accuracy of both routings at the 16-row
# bucket: tests/test_model_gpu.py::test_engine_fp8_graphed_decode_b16_close_to_bf16.
SMALL_M = int(os.environ.get("MXLLM_W8_SMALL_M", "8"))


def quantize_e4m3(w: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """w [N, K] -> (codes uint8 [N, K], scale f32 [N])."""
    wf = w.float()
    amax = wf.abs().amax(dim=1).clamp_min(1e-30)
    scale = amax / E4M3_MAX
    v = (wf / scale[:, None]).clamp_(-E4M3_MAX, E4M3_MAX)
    q = v.to(torch.float8_e4m3fn).view(torch.uint8)
    exp0 = (q & 0x78) == 0  # zero or subnormal -> smallest normal, same sign
    q = torch.where(exp0, (q & 0x80) | 0x08, q)
    return q.contiguous(), scale.contiguous()


def dequantize_e4m3(q: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """Reference decode (fp32) of codes produced by :func:`quantize_e4m3`."""
    qi = q.to(torch.int32)
    e = (qi >> 3) & 0xF
    m = (qi & 7).float()
    mag = torch.ldexp(1.0 + m / 8.0, e - 7)
    v = torch.where((qi & 0x80) != 0, -mag, mag)
    return v * scale.float()[:, None]


# ---------------------------------------------------------------- kv8: the fp8 KV-cache row format
# A row is the 128 values of one (token, KV head).  scale = 2^e, the smallest power of two with
# amax(|row|) / scale <= 448, so amax / scale lies in (224, 448]: with amax = m * 2^E (1 <= m < 2),
# e = E - 8 if m <= 1.75 else E - 7, clamped to >= -100; an all-zero row has scale 1.
# code = e4m3fn(x / scale), round to nearest even, true zero and subnormals kept (unlike the weight
# format above).  The scale is a power of two, so x / scale is exact and code * scale is a bf16
# value: the dequantised cache is a bf16 cache.  Inputs are finite.  The HIP kernels
# (csrc/kernels/decode.hip kv8_*) produce the same bits; this is their reference and the CPU path.
KV8_DIM = 128
KV8_MIN_EXP = -100


def kv8_quantize(x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """x [..., 128] bf16 -> (codes uint8 [..., 128], scale f32 [...])."""
    if x.dtype != torch.bfloat16 or x.shape[-1] != KV8_DIM:
        raise ValueError(f"kv8_quantize: bf16 rows of {KV8_DIM} values, got {x.dtype} {tuple(x.shape)}")
    xf = x.float()
    bits = xf.abs().amax(-1).view(torch.int32)
    e = (bits >> 23) - 135 + ((bits & 0x7FFFFF) > 0x600000).to(torch.int32)
    e = torch.where(bits == 0, torch.zeros_like(e), e.clamp_min(KV8_MIN_EXP))
    scale = ((e + 127) << 23).view(torch.float32)
    inv = ((127 - e) << 23).view(torch.float32)
    codes = (xf * inv.unsqueeze(-1)).to(torch.float8_e4m3fn).view(torch.uint8)
    return codes.contiguous(), scale.contiguous()


def kv8_dequantize(codes: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """codes uint8 [..., 128], scale f32 [...] -> bf16 [..., 128] (exact: see above)."""
    return (codes.view(torch.float8_e4m3fn).float() * scale.unsqueeze(-1)).to(torch.bfloat16)


class W8Linear(nn.Module):
    """Frozen projection y = x W^T with fp8 weights (serving only)."""

    def __init__(self, weight: torch.Tensor):
        super().__init__()
        q, s = quantize_e4m3(weight.detach())
        self.register_buffer("q", q)
        self.register_buffer("scale", s)
        self.out_features, self.in_features = q.shape

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x2 = x.reshape(-1, self.in_features)
        if x2.stride(1) != 1 or x2.stride(0) % 8:
            x2 = x2.contiguous()  # the HIP kernels take 16-B-aligned rows
        M = x2.shape[0]
        if not use_native(x2):
            y = torch.matmul(x2, dequantize_e4m3(self.q, self.scale).to(x2.dtype).t())
        elif M <= SMALL_M or self.in_features % 16:
            # weight-streaming HIP kernel: bf16 activations, weights dequantised in registers
            # (it falls back to dequantise + hipBLASLt for shapes it does not take)
            y = native().w8_linear(x2, self.q, self.scale)
        else:
            # larger batches / prefill: fp8 x fp8 MFMA GEMM (hipBLASLt), per-token activation
            # scales and the per-channel weight scales applied by the GEMM epilogue
            xq, sa = native().quant_rows_e4m3(x2)  # one HIP pass
            y = torch._scaled_mm(xq.view(torch.float8_e4m3fn), self.q.view(torch.float8_e4m3fn).t(), scale_a=sa,
                                 scale_b=self.scale.view(1, -1), out_dtype=x2.dtype)
        return y.view(*x.shape[:-1], self.out_features)


# ---------------------------------------------------------------- MXFP4 projection weights
# OCP Microscaling v1.0 "MXFP4" on a weight W [N, K], K % 32 == 0.  A block is 32 consecutive k of one
# output channel; its shared scale is 2^e, stored as the e8m0 byte e + 127 with
# e = floor(log2(amax |block|)) - 2 clamped to [-126, 127] (read from the float's exponent field), an
# all-zero block as byte 127; bytes 0 and 255 are never emitted.  Elements are e2m1: magnitudes
# {0, 0.5, 1, 1.5, 2, 3, 4, 6} as codes 0..7, bit 3 the sign.  |w| / 2^e (exact: a power of two) is
# rounded to nearest on that grid, ties to the even code, saturating at 6 (the floor rule leaves
# amax / 2^e in [4, 8)); the sign bit is set only on a non-zero magnitude, so there is no negative zero
# and the quantiser is idempotent on its own output.  codes uint8 [N, K/2], the even k in the low nibble
# (the packing of torch.float4_e2m1fn_x2); scales uint8 [N, K/32]; no second-level scale.
# Every dequantised value +-grid * 2^e has at most two mantissa bits: the dequantised weight is a bf16
# matrix (like the kv8 cache), which is what lets the HIP kernels (csrc/kernels/mxfp4_gemm.hip) be
# tested bit for bit against these functions -- the reference, the CPU path and the load-time quantiser.
# Cost of round-to-nearest MXFP4, measured on Gaussian rows: relative RMS weight error 0.114 .. 0.115,
# about 2 % of the elements saturate.  End-task accuracy on real checkpoints has NOT been measured.
MXFP4_BLOCK = 32
MXFP4_GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)

# w4_linear streams the 4-bit weights once per 32 rows, so a call of M rows costs ceil(M / 32) weight
# passes; calls of more than STREAM_M rows dequantise into a bf16 temporary and run the hipBLASLt GEMM
# instead.  The default is the largest M at which the passes still won on the Llama-3.1 70B projection
# shapes (bench/w4_probe.py --crossover; table in profiles/mxfp4/README.md), passes / dequantise + GEMM in
# us for the four projections of a layer: 32 rows 307 / 753, 64 rows 554 / 805 (qkv alone loses, 95 / 69),
# 128 rows 1049 / 899, 256 rows 2046 / 1089.  Both routes are slower than the bf16 and fp8 engines at 64
# rows (70B decode step 48.6 ms against 36.2 / 26.2 ms): the 32-row kernel is bound by its X traffic.
STREAM_M = int(os.environ.get("MXLLM_W4_STREAM_M", "64"))


def quantize_mxfp4(w: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """w [N, K] (finite, K % 32 == 0) -> (codes uint8 [N, K/2], scales uint8 [N, K/32])."""
    if w.dim() != 2 or w.shape[1] % MXFP4_BLOCK:
        raise ValueError(f"quantize_mxfp4: [N, K] with K % {MXFP4_BLOCK} == 0, got {tuple(w.shape)}")
    N, K = w.shape
    wf = w.detach().float().reshape(N, K // MXFP4_BLOCK, MXFP4_BLOCK)
    a = wf.abs()
    bits = a.amax(-1).view(torch.int32)
    e = ((bits >> 23) - 129).clamp_(-126, 127)  # floor(log2 amax) - 2; f32 subnormals clamp
    e = torch.where(bits == 0, torch.zeros_like(e), e)
    inv = ((127 - e) << 23).view(torch.float32)  # 2^-e, a normal f32 for every e in [-126, 125]
    v = a * inv.unsqueeze(-1)
    # nearest grid point, ties to the even code: the midpoints 0.25 1.25 2.5 5 round down, 0.75 1.75 3.5 up
    code = ((v > 0.25).to(torch.uint8) + (v >= 0.75) + (v > 1.25) + (v >= 1.75) + (v > 2.5) + (v >= 3.5) + (v > 5.0))
    code = code.to(torch.uint8)
    code = code | (((wf < 0) & (code != 0)).to(torch.uint8) << 3)
    code = code.reshape(N, K // 2, 2)
    codes = code[..., 0] | (code[..., 1] << 4)
    return codes.contiguous(), (e + 127).to(torch.uint8).contiguous()


def dequantize_mxfp4(codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """Reference decode: codes uint8 [N, K/2], scales uint8 [N, K/32] (bytes 1..254) -> f32 [N, K]."""
    N, K = codes.shape[0], 2 * codes.shape[1]
    nib = torch.stack((codes & 0xF, codes >> 4), dim=-1).reshape(N, K).to(torch.int64)
    mag = torch.tensor(MXFP4_GRID, dtype=torch.float32, device=codes.device)[nib & 7]
    v = torch.where((nib & 8) != 0, -mag, mag)
    scale = (scales.to(torch.int32) << 23).view(torch.float32)  # 2^(byte - 127)
    return (v.reshape(N, K // MXFP4_BLOCK, MXFP4_BLOCK) * scale.unsqueeze(-1)).reshape(N, K)


class W4Linear(nn.Module):
    """Frozen projection y = x W^T with MXFP4 weights (serving only).  From a weight (quantised here)
    or from ``codes`` / ``scales`` in the format above."""

    def __init__(self, weight: torch.Tensor | None = None, *, codes: torch.Tensor | None = None,
                 scales: torch.Tensor | None = None):
        super().__init__()
        if weight is not None:
            if codes is not None or scales is not None:
                raise ValueError("W4Linear: a weight, or codes and scales")
            codes, scales = quantize_mxfp4(weight.detach())
        if codes is None or scales is None or codes.dtype != torch.uint8 or scales.dtype != torch.uint8 \
                or codes.dim() != 2 or scales.dim() != 2 or codes.shape[1] % 16 \
                or tuple(scales.shape) != (codes.shape[0], codes.shape[1] // 16):
            raise ValueError("W4Linear: codes uint8 [N, K/2] and scales uint8 [N, K/32], K % 32 == 0")
        if bool(((scales == 0) | (scales == 255)).any()):
            raise ValueError("W4Linear: scale bytes 0 (2^-127) and 255 (NaN) are not part of the format")
        self.register_buffer("codes", codes.contiguous())
        self.register_buffer("scales", scales.contiguous())
        self.out_features, self.in_features = codes.shape[0], 2 * codes.shape[1]

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x2 = x.reshape(-1, self.in_features)
        if x2.stride(1) != 1 or x2.stride(0) % 8:
            x2 = x2.contiguous()  # the HIP kernel takes 16-B-aligned rows
        if not use_native(x2):
            y = torch.matmul(x2, dequantize_mxfp4(self.codes, self.scales).to(x2.dtype).t())
        else:
            # weight-streaming HIP kernel, one pass per 32 rows up to STREAM_M rows; beyond, and for
            # shapes it does not take, w4_linear dequantises to bf16 and runs hipBLASLt
            y = native().w4_linear(x2, self.codes, self.scales, STREAM_M)
        return y.view(*x.shape[:-1], self.out_features)


@torch.no_grad()
def quantize_model_mxfp4_(model) -> int:
    """Replace every transformer projection (qkv, o, gate/up, down) of a Llama whose ``in_features`` is a
    multiple of 32 by a :class:`W4Linear` (LoRA adapters are merged first).  Embedding, norms and the LM
    head stay bf16.  Returns the number of weight bytes saved."""
    from ..models.llama import FusedLinear
    from .engine import merge_lora_

    merge_lora_(model)
    saved = 0
    for layer in model.layers:
        for name in ("wqkv", "wo", "wgu", "wd"):
            lin = getattr(layer, name)
            if isinstance(lin, FusedLinear) and lin.weight.shape[1] % MXFP4_BLOCK == 0:
                w = lin.weight
                q = W4Linear(w)
                setattr(layer, name, q)
                saved += w.numel() * w.element_size() - q.codes.numel() - q.scales.numel()
                del lin, w
    if torch.cuda.is_available():
        torch.cuda.empty_cache()
    return saved


@torch.no_grad()
def quantize_model_fp8_(model) -> int:
    """Replace every transformer projection (qkv, o, gate/up, down) of a Llama by
    a :class:`W8Linear` (LoRA adapters are merged first).  Embedding, norms and
    the LM head stay bf16.  Returns the number of weight bytes saved."""
    from ..models.llama import FusedLinear
    from .engine import merge_lora_

    merge_lora_(model)
    saved = 0
    for layer in model.layers:
        for name in ("wqkv", "wo", "wgu", "wd"):
            lin = getattr(layer, name)
            if isinstance(lin, FusedLinear):
                w = lin.weight
                setattr(layer, name, W8Linear(w))
                saved += w.numel() * (w.element_size() - 1)
                del lin, w
    if torch.cuda.is_available():
        torch.cuda.empty_cache()
    return saved
