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

``prefix_cache=True`` (paged mode only): blocks are reference-counted and FULL blocks can be shared
between sequences.  An index maps ``(adapter key, parent entry id, tuple of the block's token
ids)`` to ``(entry id, block)``: a block is found only through the chain of its predecessors, so it
holds the K/V of exactly that token prefix under that adapter.  Entry ids count up and are never
reused -- an evicted and re-used block can never be reached through a stale child -- and the token
tuple itself is the dict key, not its hash, so a hash collision cannot serve the wrong K/V.
``match_prefix`` finds the longest cached chain, ``reserve(..., shared=blocks)`` puts it first in the
slot's table row, ``register`` enters a slot's full blocks, ``release`` lowers the counts:
unreferenced indexed blocks wait in an LRU list (last block of a chain first, so a chain is evicted
from its tail) and are evicted only when the free list is empty.  A shared block is full and never
written: a sequence writes only positions at or beyond its cached length, which lie in its own blocks.
"""
from __future__ import annotations

import itertools
import math
from collections import OrderedDict

import torch

BLOCK = 256
KV_DTYPES = ("bf16", "fp8")


class KVCache:
    def __init__(self, n_layers: int, n_kv_heads: int, head_dim: int, dtype, device, n_slots: int, max_seq: int,
                 pool_tokens: int | None = None, block: int = BLOCK, scratch_slot: int | None = None,
                 kv_dtype: str = "bf16", prefix_cache: bool = False):
        if prefix_cache and pool_tokens is None:
            raise ValueError("prefix_cache needs the paged KV cache (pool_tokens)")
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
        # prefix cache: reference counts, the index and the LRU list of unreferenced indexed blocks
        self.prefix_cache = bool(prefix_cache)
        self.ref = [0] * n_blocks
        self.index: dict[tuple, tuple[int, int]] = {}      # (adapter, parent entry, tokens) -> (entry, block)
        self.block_key: dict[int, tuple] = {}              # indexed block -> its index key
        self.lru: OrderedDict[int, None] = OrderedDict()   # unreferenced indexed blocks, evicted from the front
        self._entry_ids = itertools.count(1)               # 0: the root (no parent)

    # ------------------------------------------------------------------ accounting
    def blocks_for(self, tokens: int) -> int:
        return math.ceil(max(1, min(tokens, self.max_seq)) / self.block)

    @property
    def free_blocks(self) -> int:
        return len(self.free) if self.paged else 0

    @property
    def evictable_blocks(self) -> int:
        return len(self.lru)

    def can_reserve(self, tokens: int, shared=()) -> bool:
        """``shared``: cached blocks the reservation would take from ``match_prefix`` (they are not
        taken from the free list, and those waiting in the LRU list are not evictable for it)."""
        if not self.paged:
            return True
        have = len(self.free) + len(self.lru) - sum(1 for b in shared if b in self.lru)
        return self.blocks_for(tokens) - len(shared) <= have

    def fits_at_all(self, tokens: int) -> bool:
        return not self.paged or self.blocks_for(tokens) <= self.n_blocks - (1 if self.scratch_slot is not None else 0)

    def reserve(self, slot: int, tokens: int, shared=()) -> None:
        """Give ``slot`` the blocks for positions [0, tokens) (paged mode; a no-op
        in static mode, where every slot owns max_seq positions).  ``shared`` (prefix cache): the
        cached blocks of ``match_prefix`` come first in the table row, their counts raised; the rest
        comes from the free list and, when that is empty, from the least-recently-used unreferenced
        cached blocks, which are evicted."""
        if not self.paged:
            return
        self.release(slot)
        n = self.blocks_for(tokens)
        shared = list(shared)
        if shared and not self.prefix_cache:
            raise ValueError("shared blocks need prefix_cache=True")
        if len(shared) > n:
            raise ValueError(f"{len(shared)} shared blocks for a reservation of {n}")
        if not self.can_reserve(tokens, shared):
            raise RuntimeError(f"KV pool exhausted: need {n - len(shared)} blocks, {len(self.free)} free, "
                               f"{len(self.lru)} evictable")
        for b in shared:  # referenced first: a block in use is never evicted
            self.ref[b] += 1
            self.lru.pop(b, None)
        own = n - len(shared)
        while len(self.free) < own:
            self._evict()
        blocks, self.free = shared + self.free[:own], self.free[own:]
        for b in blocks[len(shared):]:
            self.ref[b] = 1
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
        if not (self.paged and slot in self.owned and slot != self.scratch_slot):
            return
        blocks = self.owned.pop(slot)
        if not self.prefix_cache:
            self.free.extend(blocks)
            return
        for b in reversed(blocks):  # the last block of a chain enters the LRU list first: evicted first
            self.ref[b] -= 1
            if self.ref[b] > 0:
                continue
            if b in self.block_key:
                self.lru[b] = None
                self.lru.move_to_end(b)
            else:
                self.free.append(b)

    # ------------------------------------------------------------------ prefix cache
    def _evict(self) -> int:
        """Drop the least-recently-used unreferenced cached block from the index; it joins the free list."""
        b, _ = self.lru.popitem(last=False)
        del self.index[self.block_key.pop(b)]
        self.free.append(b)
        return b

    def match_prefix(self, tokens, adapter=None) -> list[int]:
        """The longest chain of cached full blocks that holds a prefix of ``tokens`` under ``adapter``
        (any hashable key; None: the base model), at most ``(len(tokens) - 1) // block`` blocks so
        that at least one token is always computed."""
        if not self.prefix_cache:
            return []
        out, parent = [], 0
        for j in range((len(tokens) - 1) // self.block):
            hit = self.index.get((adapter, parent, tuple(tokens[j * self.block:(j + 1) * self.block])))
            if hit is None:
                break
            parent = hit[0]
            out.append(hit[1])
        return out

    def register(self, slot: int, tokens, adapter=None, upto: int | None = None) -> int:
        """Enter the full blocks of ``slot`` that lie below ``upto`` written positions (default: all of
        ``tokens``) into the index; ``tokens`` are the ids at the slot's positions.  A key that is
        already present keeps its block: the slot keeps its own copy, unindexed, and the chain goes on
        under the indexed entry.  Returns the number of blocks newly entered."""
        if not self.prefix_cache or slot not in self.owned or slot == self.scratch_slot:
            return 0
        upto = len(tokens) if upto is None else min(upto, len(tokens))
        blocks, parent, new = self.owned[slot], 0, 0
        for j in range(min(upto // self.block, len(blocks))):
            key = (adapter, parent, tuple(tokens[j * self.block:(j + 1) * self.block]))
            hit = self.index.get(key)
            if hit is None:
                if blocks[j] in self.block_key:  # already indexed under another chain: leave it there
                    break
                hit = (next(self._entry_ids), blocks[j])
                self.index[key] = hit
                self.block_key[blocks[j]] = key
                new += 1
            parent = hit[0]
        return new

    def drop_adapter(self, adapter) -> int:
        """Remove every index entry of ``adapter``: unreferenced blocks join the free list, blocks
        still in use become ordinary owned blocks.  Returns the number of entries removed."""
        keys = [k for k in self.index if k[0] == adapter]
        for k in keys:
            _, b = self.index.pop(k)
            del self.block_key[b]
            if b in self.lru:
                del self.lru[b]
                self.free.append(b)
        return len(keys)

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
