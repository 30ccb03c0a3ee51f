"""Paged KV cache for the serving engine (VERDICT r2 missing #5).

Per layer, K and V are POOLS of fixed-size blocks ``[blocks, Hkv, block, D]``
(bf16; ``kv_dtype="fp8"``: e4m3 codes with one f32 scale per row, see below)
and every sequence slot maps its token positions to pool blocks through
a block table ``bt [slots, max_blocks]`` (int32, on the device).  Token ``p`` of
slot ``s`` lives in block ``bt[s, p // block]`` at row ``p % block``.  The HIP
decode kernels (csrc/kernels/decode.hip ``kv_row``: RoPE + cache append, the
split-K decode attention, the fused QKV GEMM epilogue) read the table; the block
size is a multiple of the 256-key decode split, so every split streams ONE
contiguous block.

Two modes:
  * static (``pool_tokens=None``): every slot owns ``max_blocks`` blocks for
    life — the memory of the old ``[slots, Hkv, max_seq, D]`` slab;
  * paged (``pool_tokens=N``): a shared pool of ``ceil(N / block)`` blocks; a
    request reserves only ``ceil(min(prompt + max_new_tokens, max_seq) / block)``
    blocks at admission and returns them when it finishes.  The reference
    workload's IMDB reviews are ~0.3-4k tokens, so with a 70B model (320 KiB of
    KV per token) a pool sized for the AVERAGE length serves several times more
    concurrent requests than slots sized for the longest one.

One spare slot with one block takes the padding rows of a graphed decode step.

``kv_dtype="fp8"`` (head_dim 128): the kv8 row format of mxllm/serve/quant.py.  ``k`` / ``v`` are
uint8 code pools of the same shape and ``k_scale`` / ``v_scale`` f32 pools ``[blocks, Hkv, block]``
hold one power-of-two scale per (token, KV head) row: 132 bytes per row instead of 256.  ``write``
quantises (HIP ``kv8_quant_rows``; CPU: the codec), ``gather`` returns the dequantised bf16 rows,
and block accounting is the same.
"""
from __future__ import annotations

import math

import torch

BLOCK = 256
KV_DTYPES = ("bf16", "fp8")


class KVCache:
    def __init__(self, n_layers: int, n_kv_heads: int, head_dim: int, dtype, device, n_slots: int, max_seq: int,
                 pool_tokens: int | None = None, block: int = BLOCK, scratch_slot: int | None = None,
                 kv_dtype: str = "bf16"):
        if block % 256:
            raise ValueError("KV block size must be a multiple of 256 tokens (the decode split)")
        if kv_dtype not in KV_DTYPES:
            raise ValueError(f"kv_dtype must be one of {KV_DTYPES}, got {kv_dtype!r}")
        if kv_dtype == "fp8" and (head_dim != 128 or dtype != torch.bfloat16):
            raise ValueError(f"the fp8 KV cache supports head_dim 128 and bf16 models only, got head_dim {head_dim}, {dtype}")
        self.kv_dtype = kv_dtype
        self.fp8 = kv_dtype == "fp8"
        self.block = block
        self.max_seq = max_seq
        self.maxb = math.ceil(max_seq / block)
        self.n_slots = n_slots
        self.paged = pool_tokens is not None
        self.scratch_slot = scratch_slot
        if self.paged:
            n_blocks = max(math.ceil(pool_tokens / block), 1)
        else:
            n_blocks = (n_slots - (1 if scratch_slot is not None else 0)) * self.maxb
        n_blocks += 1 if scratch_slot is not None else 0
        self.n_blocks = n_blocks
        self.k = [torch.zeros(n_blocks, n_kv_heads, block, head_dim, dtype=torch.uint8 if self.fp8 else dtype,
                              device=device) for _ in range(n_layers)]
        self.v = [torch.zeros_like(k) for k in self.k]
        # fp8: zero codes under scale 1 (a row never written decodes to zeros)
        self.k_scale = [torch.ones(n_blocks, n_kv_heads, block, dtype=torch.float32, device=device)
                        for _ in range(n_layers if self.fp8 else 0)]
        self.v_scale = [torch.ones_like(s) for s in self.k_scale]
        self.bt_host = torch.zeros(n_slots, self.maxb, dtype=torch.int32)
        self.owned: dict[int, list[int]] = {}
        self.free: list[int] = []
        if self.paged:
            self.free = list(range(n_blocks - (1 if scratch_slot is not None else 0)))
        else:
            for s in range(n_slots):
                if s == scratch_slot:
                    continue
                j = s - (1 if scratch_slot is not None and s > scratch_slot else 0)
                self.owned[s] = list(range(j * self.maxb, (j + 1) * self.maxb))
                self.bt_host[s] = torch.tensor(self.owned[s], dtype=torch.int32)
        if scratch_slot is not None:
            self.owned[scratch_slot] = [n_blocks - 1]
            self.bt_host[scratch_slot, :] = n_blocks - 1
        self.bt = self.bt_host.to(device)

    # ------------------------------------------------------------------ accounting
    def blocks_for(self, tokens: int) -> int:
        return math.ceil(max(1, min(tokens, self.max_seq)) / self.block)

    @property
    def free_blocks(self) -> int:
        return len(self.free) if self.paged else 0

    def can_reserve(self, tokens: int) -> bool:
        return not self.paged or self.blocks_for(tokens) <= len(self.free)

    def fits_at_all(self, tokens: int) -> bool:
        return not self.paged or self.blocks_for(tokens) <= self.n_blocks - (1 if self.scratch_slot is not None else 0)

    def reserve(self, slot: int, tokens: int) -> None:
        """Give ``slot`` the blocks for positions [0, tokens) (paged mode; a no-op
        in static mode, where every slot owns max_seq positions)."""
        if not self.paged:
            return
        self.release(slot)
        n = self.blocks_for(tokens)
        if n > len(self.free):
            raise RuntimeError(f"KV pool exhausted: need {n} blocks, {len(self.free)} free")
        blocks, self.free = self.free[:n], self.free[n:]
        self.owned[slot] = blocks
        row = torch.zeros(self.maxb, dtype=torch.int32)
        row[:n] = torch.tensor(blocks, dtype=torch.int32)
        row[n:] = blocks[-1]  # never read (lengths stay inside the reservation); keeps the table in range
        self.bt_host[slot] = row
        self.bt[slot].copy_(row.to(self.bt.device), non_blocking=False)

    def capacity(self, slot: int) -> int:
        """Positions ``slot`` can hold."""
        if not self.paged:
            return self.max_seq
        return min(len(self.owned.get(slot, ())) * self.block, self.max_seq)

    def release(self, slot: int) -> None:
        if self.paged and slot in self.owned and slot != self.scratch_slot:
            self.free.extend(self.owned.pop(slot))

    # ------------------------------------------------------------------ data
    def write(self, layer: int, slot: int, k: torch.Tensor, v: torch.Tensor) -> None:
        """Store K/V rows of positions [0, S) of ``slot``: k, v [Hkv, S, D] (fp8: quantised here)."""
        Hkv, S, D = k.shape
        nb = math.ceil(S / self.block)
        blocks = self.owned[slot][:nb]
        if len(blocks) < nb:
            raise RuntimeError(f"slot {slot} holds {len(blocks)} KV blocks, {nb} needed")
        if not self.fp8:
            self._store(self.k[layer], blocks, k)
            self._store(self.v[layer], blocks, v)
            return
        from ..ops.decode import kv8_quant_rows

        for codes, scale, x in ((self.k[layer], self.k_scale[layer], k), (self.v[layer], self.v_scale[layer], v)):
            cd, sc = kv8_quant_rows(x.to(torch.bfloat16).reshape(Hkv * S, D))
            self._store(codes, blocks, cd.view(Hkv, S, D))
            self._store(scale, blocks, sc.view(Hkv, S))

    def _store(self, pool: torch.Tensor, blocks: list[int], x: torch.Tensor) -> None:
        """x [Hkv, S, ...] -> rows [0, S) of the pool blocks ``blocks`` (pool [blocks, Hkv, block, ...])."""
        Hkv, S, tail = x.shape[0], x.shape[1], x.shape[2:]
        full = S // self.block
        if full:
            src = x[:, :full * self.block].reshape(Hkv, full, self.block, *tail).transpose(0, 1)
            if all(blocks[j] == blocks[0] + j for j in range(full)):  # consecutive blocks: views
                pool[blocks[0]:blocks[0] + full].copy_(src)
            else:
                pool.index_copy_(0, torch.tensor(blocks[:full], device=pool.device), src)
        rem = S - full * self.block
        if rem:
            pool[blocks[full], :, :rem].copy_(x[:, full * self.block:])

    def _rows(self, pool: torch.Tensor, slot: int, L: int) -> torch.Tensor:
        """Rows [0, L) of ``slot`` of one pool [blocks, Hkv, block, ...] as [Hkv, L, ...]."""
        nb = math.ceil(L / self.block)
        idx = self.bt_host[slot, :nb].to(torch.long).to(pool.device)
        t = pool.index_select(0, idx)  # [nb, Hkv, block, ...]
        return t.transpose(0, 1).reshape(t.shape[1], nb * self.block, *t.shape[3:])[:, :L]

    def gather(self, layer: int, slot: int, L: int) -> tuple[torch.Tensor, torch.Tensor]:
        """K/V of positions [0, L) of ``slot`` as [Hkv, L, D] bf16 (fp8: dequantised; reference
        paths / tests)."""
        if self.fp8:
            from .quant import kv8_dequantize

            kc, ks, vc, vs = self.gather_raw(layer, slot, L)
            return kv8_dequantize(kc, ks), kv8_dequantize(vc, vs)
        return self._rows(self.k[layer], slot, L), self._rows(self.v[layer], slot, L)

    def gather_raw(self, layer: int, slot: int, L: int):
        """fp8: the stored (k_codes, k_scale, v_codes, v_scale) of positions [0, L) of ``slot`` as
        [Hkv, L, 128] uint8 / [Hkv, L] f32."""
        return (self._rows(self.k[layer], slot, L), self._rows(self.k_scale[layer], slot, L),
                self._rows(self.v[layer], slot, L), self._rows(self.v_scale[layer], slot, L))

    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self.k + self.v + self.k_scale + self.v_scale)
