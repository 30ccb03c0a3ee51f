"""The CPU path of ``prefill_attention_paged`` over kv8 pools, one segment that crosses a block boundary: the chunk's
rows land in the pools through ``kv8_quantize`` (K rotated and rounded to bf16 first) and the output is the softmax
over the DEQUANTISED rows, against the fp64 expression written out here (``_parity.DECODE_O_F32``: fp32 softmax -> bf16).
"""
import math

import pytest
import torch

from mxllm.ops import decode as dops
from mxllm.serve.quant import kv8_dequantize, kv8_quantize
from tests import _parity as P
from tests._parity import assert_exact, assert_parity

BF16, F64 = torch.bfloat16, torch.float64
Hq, Hkv, D, BLK = 4, 2, 128, 256
N, P0, TABLE = 40, 236, [2, 0]  # positions 236 .. 275: blocks 2 and 0


def test_cpu_path_over_kv8_pools():
    g = torch.Generator().manual_seed(5)
    L = P0 + N
    pos = torch.arange(L + 8, dtype=torch.float32)[:, None] * torch.exp2(-torch.arange(D // 2) / 8.0)[None]
    cos, sin = pos.cos(), pos.sin()
    qkv = torch.randn(N, (Hq + 2 * Hkv) * D, generator=g).to(BF16)
    old_k, old_v = (torch.randn(Hkv, P0, D, generator=g).to(BF16) for _ in range(2))
    kq, vq = (torch.full((3, Hkv, BLK, D), 0x7F, dtype=torch.uint8) for _ in range(2))  # NaN everywhere else
    ks, vs = (torch.full((3, Hkv, BLK), float("nan")) for _ in range(2))
    for codes, scale, rows in ((kq, ks, old_k), (vq, vs, old_v)):
        codes[TABLE[0], :, :P0], scale[TABLE[0], :, :P0] = kv8_quantize(rows)
    bt = torch.tensor([TABLE], dtype=torch.int32)

    with pytest.raises(ValueError):
        dops.prefill_attention_paged(qkv, cos, sin, kq, vq, bt, [(0, N, 0, P0)], Hq, Hkv, D, k_scale=ks)
    out = dops.prefill_attention_paged(qkv, cos, sin, kq, vq, bt, [(0, N, 0, P0)], Hq, Hkv, D, k_scale=ks, v_scale=vs)

    x = qkv.view(N, Hq + 2 * Hkv, D).float()
    c, s = cos[P0:L].view(N, 1, D // 2), sin[P0:L].view(N, 1, D // 2)
    rot = lambda t: torch.cat([t[..., :D // 2] * c - t[..., D // 2:] * s, t[..., D // 2:] * c + t[..., :D // 2] * s], -1).to(BF16)
    want = {"k": rot(x[:, Hq:Hq + Hkv]).transpose(0, 1), "v": qkv.view(N, -1, D)[:, Hq + Hkv:].transpose(0, 1)}
    rows = {}
    for name, codes, scale, old in (("k", kq, ks, old_k), ("v", vq, vs, old_v)):
        lc = torch.cat([codes[TABLE[0]], codes[TABLE[1]]], 1)[:, :L]  # the slot's rows by plain indexing
        lsc = torch.cat([scale[TABLE[0]], scale[TABLE[1]]], 1)[:, :L]
        wc, wsc = kv8_quantize(torch.cat([old, want[name]], 1))
        assert_exact(lc, wc, name=f"{name} codes")
        assert_exact(lsc, wsc, name=f"{name} scales")
        rows[name] = kv8_dequantize(lc, lsc).to(F64).repeat_interleave(Hq // Hkv, 0)  # [Hq, L, D]
    assert (kq[1] == 0x7F).all() and ks[1].isnan().all()  # the block of no slot is untouched
    sc = torch.einsum("nhd,hld->hnl", rot(x[:, :Hq]).to(F64), rows["k"]) / math.sqrt(D)
    dead = torch.arange(L).view(1, 1, L) > torch.arange(N).view(1, N, 1) + P0
    ref = torch.einsum("hnl,hld->nhd", sc.masked_fill(dead, float("-inf")).softmax(-1), rows["v"])
    assert_parity(out.view(N, Hq, D), ref, P.DECODE_O_F32, name="O")
