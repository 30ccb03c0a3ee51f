"""mxllm inference engine: KV cache + prefill/decode + continuous batching.

This replaces the reference's remote API offload: ``get_model_response``
(reference src/distributed_inference.py:34-41) called an external Llama-3.1-70B
over HTTP, one blocking request per prompt.  Here every rank
serves its own shard of prompts from its own GPU, batched.

MI355X-first sizing: the KV cache (mxllm/serve/kvcache.py) is a pool of
256-token blocks per layer addressed through a per-slot block table.  Static
mode gives every slot max_seq positions (70B: 320 KiB/token, 16 slots x 8k
tokens = 43 GB beside the 141 GB of weights on one 288 GB MI355X); paged mode
(``kv_pool_tokens``) shares a pool and a request reserves only
prompt + max_new_tokens, so many more short requests run at once.  Prefill
runs the MFMA flash-attention kernel; decode runs the split-K decode kernel
(one workgroup streams 256 cached keys of one (sequence, kv-head) and serves
all q-heads of that GQA group).  Scheduling is continuous batching: new
requests are prefilled between decode steps (all prompts admitted together in
one pass: concatenated tokens through the GEMMs, attention per sequence) and
join the running batch.

Decode is launch-bound at small batch (a 32-layer step is ~300 kernel
launches), so on GPU each decode step is replayed from a hipGraph
(``torch.cuda.CUDAGraph`` is hipGraph capture on ROCm).  One graph per
(batch bucket, key-split bucket): the batch is padded to a power of two with
entries that write into a scratch cache slot, the split-K decode kernel gets
a power-of-two key bound (splits past a sequence's length exit at once), and
the step's only host->device traffic is one [3, B] int64 copy of
(token, position, slot).

LoRA adapters (``max_adapters`` > 0): one copy of the base weights and static tables of adapters;
a request names its adapter and requests with different adapters share a batch.  The step input
is then [4, B] (the fourth row: each row's adapter table slot, -1 = none) and graphs are keyed
(batch bucket, key bucket, any_adapter): a step in which no row has an adapter replays the same
fused launches as an engine without tables; a step with adapters runs every projection unfused
followed by the two gather kernels of ``ops.lora_delta_rows_``.

Speculative decoding (``speculate=K``, off by default): a decode step may carry up to K + 1 rows of one
sequence -- its last token and up to K drafted tokens (mxllm/serve/speculate.py: prompt lookup, no
second model).  The rows run through the same projections (the weights are streamed once), each row's
K/V are appended at its own position, ``dops.verify_attention`` streams the sequence's K/V once for all
its rows, the sampler draws on every row and ``dops.spec_accept`` keeps the drafts the draws confirm.
The drafts are deterministic, so this is exact speculative sampling: the token stream is the plain
engine's.  Such a step is replayed from a graph keyed ("verify", row bucket, key bucket, K + 1) beside
the keys above; a step in which no request has a draft, or some row has a LoRA adapter, is the plain step.
"""
from __future__ import annotations

import itertools
import logging
import math
import os
import threading
import time
from dataclasses import dataclass, field

import torch

from .. import ops
from ..models.llama import FusedLinear
from ..ops import decode as dops

_SWIGLU_FUSED = os.environ.get("MXLLM_SWIGLU_FUSED", "1") != "0"  # A/B switch (bench/serve_bench.py)
_NORM_FUSED = os.environ.get("MXLLM_NORM_FUSED", "1") != "0"  # A/B switch: RMSNorm in the decode GEMM prologue
_ROPE_FUSED = os.environ.get("MXLLM_ROPE_FUSED", "1") != "0"  # A/B switch: RoPE + cache append in the QKV epilogue
# the split-K attention merge in the o-projection GEMM's prologue (decode rows <= 4): OFF by
# default -- measured 8B decode, same box: batch 1 3.424 vs 3.433 ms (a wash), batch 4 4.113 vs
# 3.841 ms (the prologue slows the weight stream more than the combine launch costs;
# archive/profiles/r3d_decode_merge_ab.md).  MXLLM_MERGE_FUSED=1 turns it on.
_MERGE_FUSED = os.environ.get("MXLLM_MERGE_FUSED", "0") == "1"
# Small-batch decode: while the (latency-bound) attention runs, a side-stream kernel reads
# the layer's o-projection weight so the o-projection GEMM streams it from the Infinity
# Cache instead of HBM (MXLLM_DECODE_PREFETCH=1; up to PREFETCH_MAX_B rows).  Measured
# slower (fork/join + competing reads; archive/profiles/r3g/README.md): off by default.
_PREFETCH = os.environ.get("MXLLM_DECODE_PREFETCH", "0") == "1"
PREFETCH_MAX_B = 8
log = logging.getLogger("mxllm.engine")


@dataclass
class SamplingParams:
    max_new_tokens: int = 64
    temperature: float = 0.0
    top_p: float = 1.0
    top_k: int = 0
    stop_ids: tuple = ()
    seed: int = 0
    # Sampling penalties, logit_bias and logprobs (mxllm/ops/decode.py adjust_logits_rows /
    # logprob_rows).  Each logits row is edited in this order: repetition penalty (HF / vLLM:
    # tokens of the prompt AND the output, x / r if x > 0 else x * r), then
    # frequency * count + presence subtracted (OpenAI: tokens of the output only), then
    # logit_bias added.  ``logprobs``: None = off, else the number (0..20) of most likely tokens
    # listed per output token besides the chosen token's own log-probability.  The
    # log-probabilities are the log-softmax of the logits AFTER penalties and bias and BEFORE
    # temperature and the top-k / top-p cut; ties in the top list go to the lower token id.
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0
    repetition_penalty: float = 1.0
    logit_bias: dict | None = None
    logprobs: int | None = None

    def __post_init__(self):
        if not (self.top_p == self.top_p and self.temperature == self.temperature):
            raise ValueError("top_p / temperature must not be NaN")
        if self.top_p < 0:
            raise ValueError(f"top_p must be in [0, 1] (0 = greedy), got {self.top_p}")
        if self.max_new_tokens < 0:
            raise ValueError(f"max_new_tokens must be >= 0, got {self.max_new_tokens}")
        for name in ("presence_penalty", "frequency_penalty"):
            v = getattr(self, name)
            if not (isinstance(v, (int, float)) and -2.0 <= v <= 2.0):
                raise ValueError(f"{name} must be in [-2, 2], got {v!r}")
        r = self.repetition_penalty
        if not (isinstance(r, (int, float)) and 0.0 < r < float("inf")):
            raise ValueError(f"repetition_penalty must be > 0, got {r!r}")
        if self.logit_bias is not None:
            if not isinstance(self.logit_bias, dict) or len(self.logit_bias) > 300:
                raise ValueError("logit_bias must be a dict of at most 300 token ids")
            bias = {}
            for k, v in self.logit_bias.items():
                try:
                    k = int(k)
                except (TypeError, ValueError):
                    raise ValueError(f"logit_bias key {k!r} is not a token id") from None
                if isinstance(v, bool) or not isinstance(v, (int, float)) or not -100.0 <= v <= 100.0:
                    raise ValueError(f"logit_bias values must be in [-100, 100], got {v!r}")
                bias[k] = float(v)
            self.logit_bias = bias or None
        if self.logprobs is not None:
            if isinstance(self.logprobs, bool) or not isinstance(self.logprobs, int) or not 0 <= self.logprobs <= 20:
                raise ValueError(f"logprobs must be None or in 0..20, got {self.logprobs!r}")

    @property
    def penalised(self) -> bool:
        """Needs the per-request token counts."""
        return self.presence_penalty != 0 or self.frequency_penalty != 0 or self.repetition_penalty != 1

    @property
    def adjusts(self) -> bool:
        return self.penalised or bool(self.logit_bias)


@dataclass
class Request:
    rid: int
    prompt: list
    params: SamplingParams
    output: list = field(default_factory=list)
    slot: int = -1
    done: threading.Event = field(default_factory=threading.Event)
    finish_reason: str | None = None
    t_submit: float = field(default_factory=time.perf_counter)
    t_first: float | None = None
    t_done: float | None = None
    error: str | None = None
    # one (logprob, [(token id, logprob), ...]) per output token when params.logprobs is set
    logprobs: list = field(default_factory=list)
    adapter: str | None = None  # name of a loaded LoRA adapter (Engine.load_adapter); None = the base model
    cached_tokens: int = 0  # prompt tokens served from the prefix cache (Engine(prefix_cache=True))
    prefilled: int = 0      # prompt positions whose K/V are in the cache (paged prefill: cached + computed chunks)
    spec_index: object = None  # speculative decoding: the request's n-gram index (mxllm/serve/speculate.py)

    def __post_init__(self):
        # any penalty / logit_bias / logprobs: the request takes the adjusted sampling path
        self.special = self.params.adjusts or self.params.logprobs is not None


class Engine:
    def __init__(self, model, max_batch: int = 8, max_seq: int = 4096, device=None, eos_ids=(),
                 use_graphs: bool | None = None, prefill_tokens: int = 16384, tp_group=None,
                 kv_pool_tokens: int | None = None, kv_block: int = 256, kv_dtype: str | None = None,
                 max_adapters: int = 0, max_lora_rank: int = 16, prefix_cache: bool | None = None,
                 prefill_chunk: int | None = None, speculate: int | None = None, drafter=None):
        """``tp_group``: serve a tensor-parallel shard (mxllm/parallel/tensor.py
        ``shard_llama`` / ``random_shard``) with the other ranks of the group;
        every rank of the group runs the same schedule (same submissions in the
        same order, e.g. SPMD ``generate`` or ``serve_follower``).
        ``kv_pool_tokens``: paged KV cache of that many tokens shared by all slots
        (None: every slot owns max_seq positions; env MXLLM_KV_POOL_TOKENS).
        ``kv_dtype``: "bf16" or "fp8" (None: env MXLLM_KV_CACHE, default bf16).  fp8 stores the
        cache as e4m3 codes with one power-of-two scale per (token, KV head) row
        (mxllm/serve/kvcache.py; head_dim 128): prefill attends over the fresh bf16 K/V and only
        the cache write quantises; a decode step runs RMSNorm + QKV GEMM + ``rope_append_kv8`` +
        ``decode_attn_kv8`` (the fused QKV epilogue cannot see a whole row's amax, so
        MXLLM_ROPE_FUSED, MXLLM_DECODE_COMBINE=fused and MXLLM_MERGE_FUSED do not apply).
        ``max_adapters`` > 0: serve that many LoRA adapters beside the base weights
        (``load_adapter``; a request names its adapter), each of rank <= ``max_lora_rank`` (8, 16,
        32 or 64).  The tables (mxllm/ops/lora_serve.py ``AdapterTables``) are allocated once; 0
        allocates nothing and leaves every code path as it is without adapters.
        ``prefix_cache`` (None: env MXLLM_PREFIX_CACHE=1; needs ``kv_pool_tokens``): full 256-token
        blocks of finished and running requests stay indexed by their token prefix and adapter
        (mxllm/serve/kvcache.py); a request whose prompt starts with a cached chain shares those
        blocks and prefills only the rest.  ``prefill_chunk`` = N (None: env MXLLM_PREFILL_CHUNK):
        a step prefills at most N prompt tokens before the running batch gets its decode step, so a
        long prompt no longer stalls streaming requests for its whole prefill.  With either option
        every prefill runs through ``prefill_segments`` (``dops.prefill_attention_paged``: attention
        of a chunk over the rows already in the block pool); with both off nothing changes.
        Neither works with ``kv_dtype="fp8"`` or ``tp_group`` yet (ValueError).  Two new requests of
        ONE admission pass that share a prefix both miss: blocks are registered when a prompt completes.
        ``speculate`` = K (None: env MXLLM_SPECULATE; 0 / None: off): speculative decoding with up to K
        drafted tokens per request and step (``verify``; the module docstring).  ``drafter``: any
        callable ``(tokens: list[int], k: int) -> list[int]`` that proposes at most k tokens to follow
        ``tokens`` (prompt + output); None: prompt lookup, kept incrementally per request
        (mxllm/serve/speculate.py).  Requests with penalties, logit_bias or logprobs get no drafts, a
        step with a LoRA row is the plain step, and tensor parallelism is not supported yet (ValueError).
        (K + 1) * (n_heads / n_kv_heads) must not exceed 32, the columns of the verify kernel."""
        if speculate is None and os.environ.get("MXLLM_SPECULATE"):
            speculate = int(os.environ["MXLLM_SPECULATE"])
        speculate = int(speculate or 0)
        if speculate < 0:
            raise ValueError(f"speculate must be >= 0, got {speculate}")
        if speculate and tp_group is not None:
            raise ValueError("speculate is not supported under tensor parallelism (tp_group) yet")
        if speculate:
            group = model.cfg.n_heads // model.cfg.n_kv_heads
            if (speculate + 1) * group > 32:
                raise ValueError(f"speculate={speculate}: {speculate + 1} rows of {group} q-heads per KV head exceed the "
                                 f"32 columns of the verify kernel; this model allows speculate <= {32 // group - 1}")
        self.speculate = speculate
        self.drafter = drafter
        if max_adapters < 0:
            raise ValueError(f"max_adapters must be >= 0, got {max_adapters}")
        if max_adapters > 0 and tp_group is not None:
            raise ValueError("LoRA adapters are served by single-GPU engines (tp_group with max_adapters > 0)")
        if prefix_cache is None:
            prefix_cache = os.environ.get("MXLLM_PREFIX_CACHE", "0") not in ("", "0")
        if prefill_chunk is None and os.environ.get("MXLLM_PREFILL_CHUNK"):
            prefill_chunk = int(os.environ["MXLLM_PREFILL_CHUNK"])
        if prefill_chunk is not None and prefill_chunk < 1:
            raise ValueError(f"prefill_chunk must be >= 1, got {prefill_chunk}")
        self.prefix_cache = bool(prefix_cache)
        self.prefill_chunk = prefill_chunk
        self.paged_prefill = self.prefix_cache or prefill_chunk is not None  # every prefill through prefill_segments
        if self.paged_prefill and tp_group is not None:
            raise ValueError("prefix_cache / prefill_chunk are not supported under tensor parallelism (tp_group) yet")
        self.model = model
        self.tp = None
        if tp_group is not None:
            from ..parallel.tensor import TPComm

            self.tp = TPComm(tp_group, getattr(model, "tp_vocab", model.cfg.vocab_size),
                             device=device or model.tok_emb.device)
            if self.tp.world == 1:
                self.tp = None
        self.prefill_budget = max(1, prefill_tokens)  # tokens per prefill pass
        self.cfg = model.cfg
        self.device = device or model.tok_emb.device
        self.max_batch = max_batch
        self.max_seq = min(max_seq, self.cfg.max_seq_len)
        if self.device.type == "cuda":
            # tuned hipBLASLt/rocBLAS solution table (read-only; incl. the 70B decode shapes,
            # bench/tune_decode_gemms.py); MXLLM_GEMM_TUNING=0 keeps the library defaults
            from ..utils import gemm_tuning

            gemm_tuning.enable()
        if use_graphs is None:
            use_graphs = self.device.type == "cuda" and os.environ.get("MXLLM_DECODE_GRAPHS", "1") != "0"
            if self.tp is not None:  # RCCL collectives are graph-capturable, gloo's are not
                import torch.distributed as dist

                use_graphs = use_graphs and dist.get_backend(self.tp.group) == "nccl"
        self.use_graphs = bool(use_graphs)
        self._graphs: dict = {}
        self._pool = None
        self.scratch_slot = max_batch  # padding rows of a graphed step write here
        c = self.cfg
        dt = model.tok_emb.dtype
        # the spare slot: padding rows of a graphed step, and of a verify step, write there
        spare = self.use_graphs or bool(speculate)
        n_slots = max_batch + (1 if spare else 0)
        if speculate and self.device.type == "cuda" and (c.head_dim != 128 or dt != torch.bfloat16):
            raise ValueError(f"speculate: the verify kernel takes bf16 models of head_dim 128; this one is {dt}, "
                             f"head_dim {c.head_dim}")
        if kv_pool_tokens is None and os.environ.get("MXLLM_KV_POOL_TOKENS"):
            kv_pool_tokens = int(os.environ["MXLLM_KV_POOL_TOKENS"])
        from .kvcache import KV_DTYPES, KVCache

        if kv_dtype is None:
            kv_dtype = os.environ.get("MXLLM_KV_CACHE") or "bf16"
        if kv_dtype not in KV_DTYPES:
            raise ValueError(f"kv_dtype / MXLLM_KV_CACHE must be one of {KV_DTYPES}, got {kv_dtype!r}")
        if kv_dtype == "fp8" and c.head_dim != 128:
            raise ValueError(f"the fp8 KV cache supports head_dim 128 only; this model has head_dim {c.head_dim}")
        self.kv_dtype = kv_dtype
        if self.paged_prefill and kv_dtype == "fp8":
            raise ValueError("prefix_cache / prefill_chunk are not supported over the fp8 KV cache yet")
        if self.prefix_cache and kv_pool_tokens is None:
            raise ValueError("prefix_cache needs the paged KV cache (kv_pool_tokens / MXLLM_KV_POOL_TOKENS)")
        self.kv = KVCache(c.n_layers, c.n_kv_heads, c.head_dim, dt, self.device, n_slots, self.max_seq,
                          pool_tokens=kv_pool_tokens, block=kv_block,
                          scratch_slot=self.scratch_slot if spare else None, kv_dtype=kv_dtype,
                          prefix_cache=self.prefix_cache)
        # MXLLM_DECODE_COMBINE=fused: the split-K partials merge inside the attention launch (the
        # last workgroup of each (seq, kv-head) combines; these counters stay zero between calls)
        # instead of the combine kernel -- measured slower in the graphed step at every batch
        # (archive/profiles/r3g/README.md), so off by default
        self._attn_cnt = None
        if (self.device.type == "cuda" and not self.kv.fp8
                and os.environ.get("MXLLM_DECODE_COMBINE", "kernel") == "fused"):
            self._attn_cnt = torch.zeros((n_slots + 64) * self.kv.k[0].shape[1], dtype=torch.int32,
                                         device=self.device)
        self._pf_stream = torch.cuda.Stream(self.device) if self.device.type == "cuda" and _PREFETCH else None
        # LoRA adapters: static tables, name -> table slot, and the adapter (table slot, -1 = none)
        # of the sequence in each cache slot
        self.lora = None
        self.adapters: dict[str, int] = {}
        self.slot_adapter = [-1] * n_slots
        if max_adapters > 0:
            self.lora = ops.AdapterTables(c, max_adapters, max_lora_rank, self.device, max_rows=max_batch, dtype=dt)
        self.eos_ids = tuple(eos_ids) if eos_ids else (c.eos_id,)
        self.free_slots = list(range(max_batch))
        self.active: dict[int, Request] = {}
        self.waiting: list[Request] = []
        self.prefilling: list[Request] = []  # paged prefill: admitted, prompt not complete yet (FIFO)
        self.lens = [0] * max_batch
        self._ids = itertools.count()
        self._lock = threading.Lock()
        self._cv = threading.Condition(self._lock)
        self._thread = None
        self._stop = False
        self._tasks: list = []  # (fn, result box, event): run by the engine thread between steps
        self.steps = 0
        self.tokens_generated = 0
        # sampling penalties / logit_bias (``_admit_state``): allocated when the first request that
        # needs each is admitted.  int32 [max_batch, vocab] token state and f32 [max_batch, vocab] bias
        self.vocab = getattr(model, "tp_vocab", c.vocab_size)
        self._tok_state = None
        self._tok_bias = None
        # latency / throughput counters: exported by the server's
        # /metrics and by stats()
        self.prefill_tokens = 0
        self.prefill_s = 0.0
        self.decode_s = 0.0
        self.decode_tokens = 0
        self.ttft_sum = 0.0
        self.latency_sum = 0.0
        self.finished = 0
        self.prefix_query_tokens = 0  # prompt tokens of requests admitted with the prefix cache on
        self.prefix_hit_tokens = 0    # ... of which served from cached blocks
        self.prefill_chunks = 0       # segments run by prefill_segments in step()
        self.spec_steps = 0             # verify steps
        self.spec_draft_tokens = 0      # drafted tokens verified
        self.spec_accepted_tokens = 0   # ... of which accepted

    # ------------------------------------------------------------------ model pieces
    def _norm_proj(self, delta, h, gamma, lin, swiglu: bool):
        """(proj(rmsnorm(h + delta) * gamma), h + delta); ``swiglu``: proj = swiglu(lin(.)).
        Decode rows of a plain bf16 projection run as ONE launch (RMSNorm in the GEMM
        prologue, SwiGLU in its epilogue: csrc/kernels/skinny_gemm.hip)."""
        eps = self.cfg.norm_eps
        plain = type(lin) is FusedLinear and lin.lora_r == 0
        if _NORM_FUSED and plain:
            r = ops.norm_linear(delta, h, gamma, eps, lin.weight, swiglu)
            if r is not None:
                return r
        if delta is None:
            xn = ops.rms_norm(h, gamma, eps)
        else:
            xn, h = ops.add_rms_norm(delta, h, gamma, eps)
        if not swiglu:
            return lin(xn), h
        mid = None
        if _SWIGLU_FUSED and plain and xn.dim() == 2:
            mid = ops.linear_swiglu(xn, lin.weight)  # decode rows: SwiGLU in the GEMM epilogue
        if mid is None:
            mid = ops.swiglu(lin(xn))
        return mid, h

    @torch.no_grad()
    def _layers(self, x: torch.Tensor, attn_fn, qkv_fn=None, lora=None) -> torch.Tensor:
        """``qkv_fn(i, delta, h, gamma, layer)`` (decode): the fused norm + QKV + RoPE/cache-append
        projection returning (rotated q, new residual) or None; ``attn_fn(i, qkv, q=None)``.
        ``lora(i, proj, y, x)``: the pass has rows on LoRA adapters (``_layers_lora``)."""
        if lora is not None:
            return self._layers_lora(x, attn_fn, lora)
        m, c = self.model, self.cfg
        h = x
        delta, gamma = None, m.layers[0].attn_norm  # sub-block output not yet added to h, next norm
        for i, layer in enumerate(m.layers):
            r = qkv_fn(i, delta, h, gamma, layer) if qkv_fn is not None else None
            if r is not None:
                q, h = r
                o = attn_fn(i, None, q)
            else:
                qkv, h = self._norm_proj(delta, h, gamma, layer.wqkv, False)
                o = attn_fn(i, qkv)
            if isinstance(o, tuple):  # split-K partials: merged in the o-projection's prologue
                a = ops.native().skinny_merge_linear(o[0], o[1], layer.wo.weight)
            else:
                a = layer.wo(o)
            if self.tp is not None:  # row-parallel Wo: sum the heads' partial outputs
                self.tp.all_reduce_(a)
            mid, h = self._norm_proj(a, h, layer.mlp_norm, layer.wgu, True)
            d = layer.wd(mid)
            if self.tp is not None:  # row-parallel Wdown
                self.tp.all_reduce_(d)
            delta, gamma = d, (m.layers[i + 1].attn_norm if i + 1 < len(m.layers) else m.final_norm)
        if delta is None:
            return ops.rms_norm(h, gamma, c.norm_eps)
        xn, h = ops.add_rms_norm(delta, h, gamma, c.norm_eps)
        return xn

    def _layers_lora(self, x: torch.Tensor, attn_fn, lora) -> torch.Tensor:
        """``_layers`` for a pass with rows on LoRA adapters: ``lora(i, proj, y, x)`` adds the rows'
        deltas to the projection output y in place.  The unfused route -- RMSNorm kernel, projection,
        delta, ``attn_fn(i, qkv)``, SwiGLU kernel; no GEMM prologue or epilogue -- whatever the
        projection's class (``FusedLinear``, ``W8Linear``, ``W4Linear``)."""
        m, c = self.model, self.cfg
        h, delta, gamma = x, None, m.layers[0].attn_norm
        for i, layer in enumerate(m.layers):
            if delta is None:
                xn = ops.rms_norm(h, gamma, c.norm_eps)
            else:
                xn, h = ops.add_rms_norm(delta, h, gamma, c.norm_eps)
            qkv = layer.wqkv(xn)
            lora(i, "wqkv", qkv, xn)
            o = attn_fn(i, qkv)
            a = layer.wo(o)
            lora(i, "wo", a, o)
            xn, h = ops.add_rms_norm(a, h, layer.mlp_norm, c.norm_eps)
            gu = layer.wgu(xn)
            lora(i, "wgu", gu, xn)
            mid = ops.swiglu(gu)
            d = layer.wd(mid)
            lora(i, "wd", d, mid)
            delta, gamma = d, (m.layers[i + 1].attn_norm if i + 1 < len(m.layers) else m.final_norm)
        if delta is None:
            return ops.rms_norm(h, gamma, c.norm_eps)
        return ops.add_rms_norm(delta, h, gamma, c.norm_eps)[0]

    @property
    def k_cache(self):
        return self.kv.k

    @property
    def v_cache(self):
        return self.kv.v

    def reserve(self, slot: int, tokens: int) -> None:
        """Make ``slot`` able to hold ``tokens`` positions (paged KV: take blocks from the
        pool; static: nothing to do).  The scheduler reserves prompt + max_new_tokens at
        admission; direct ``prefill`` / ``decode`` callers may reserve themselves."""
        self.kv.reserve(slot, tokens)

    def _ensure(self, slot: int, tokens: int) -> None:
        if self.kv.capacity(slot) < tokens:
            if self.kv.paged and not self.kv.owned.get(slot):
                self.kv.reserve(slot, self.max_seq if self.kv.can_reserve(self.max_seq) else tokens)
            else:
                raise ValueError(f"slot {slot} holds {self.kv.capacity(slot)} KV positions, {tokens} needed")

    @torch.no_grad()
    def prefill(self, slot: int, ids: list[int]) -> torch.Tensor:
        """Run the prompt through the model, filling ``slot``'s cache; returns
        last-position logits [V] (f32)."""
        m, c = self.model, self.cfg
        S = len(ids)
        if S >= self.max_seq:
            raise ValueError(f"prompt of {S} tokens exceeds max_seq {self.max_seq}")
        self._ensure(slot, S + 1)
        t = torch.tensor(ids, dtype=torch.long, device=self.device)
        x = ops.embedding(t, m.tok_emb)

        def attn(i, qkv):
            return dops.prefill_attention(qkv, m.rope_cos, m.rope_sin, lambda k, v: self.kv.write(i, slot, k, v),
                                          S, c.n_heads, c.n_kv_heads, c.head_dim)

        xn = self._layers(x, attn)
        self.lens[slot] = S
        self.slot_adapter[slot] = -1
        return self._logits(xn[-1:]).float()[0]

    def _adapter_index(self, name) -> int:
        """Table slot of the adapter ``name`` (None: -1, the base model)."""
        if name is None:
            return -1
        if self.lora is None or name not in self.adapters:
            raise ValueError(f"unknown LoRA adapter {name!r}")
        return self.adapters[name]

    def _logits(self, xn: torch.Tensor) -> torch.Tensor:
        out = ops.linear(xn, self.model.head_weight)  # decode rows: the weight-streaming HIP GEMM
        if self.tp is not None:  # vocab-parallel head
            out = self.tp.gather_logits(out)
        return out

    @torch.no_grad()
    def prefill_batch(self, slots: list[int], prompts: list[list[int]], adapters=None) -> torch.Tensor:
        """Prefill several prompts in ONE pass: their tokens are concatenated so
        every GEMM / norm / SwiGLU runs once over all of them (each weight is
        read once per batch instead of once per prompt); attention runs per
        sequence into its own cache slot.  Returns last-position logits [n, V] f32.
        ``adapters``: one loaded adapter's name or None per prompt; the sequences keep their
        adapter in the decode steps that follow.  Each of the four projections then adds the
        delta of the runs of tokens that share an adapter (``lora_delta_rows_`` segments)."""
        m, c = self.model, self.cfg
        lens = [len(p) for p in prompts]
        if any(S >= self.max_seq for S in lens):
            raise ValueError(f"prompt exceeds max_seq {self.max_seq}")
        aidx = [self._adapter_index(a) for a in adapters] if adapters is not None else [-1] * len(prompts)
        if len(aidx) != len(prompts):
            raise ValueError("one adapter (or None) per prompt")
        for s_, S in zip(slots, lens):
            self._ensure(s_, S + 1)
        t = torch.tensor([tok for p in prompts for tok in p], dtype=torch.long, device=self.device)
        x = ops.embedding(t, m.tok_emb)
        offs = [0]
        for S in lens:
            offs.append(offs[-1] + S)

        def attn(i, qkv):
            outs = [dops.prefill_attention(qkv[offs[j]:offs[j + 1]], m.rope_cos, m.rope_sin,
                                           lambda k, v, j=j: self.kv.write(i, slots[j], k, v), lens[j], c.n_heads,
                                           c.n_kv_heads, c.head_dim)
                    for j in range(len(prompts))]
            return outs[0] if len(outs) == 1 else torch.cat(outs, 0)

        lora = None
        if any(a >= 0 for a in aidx):
            segs = ops.lora_serve.merge_segments([a for a, S in zip(aidx, lens) for _ in range(S)])

            def lora(i, proj, y, xin):
                ops.lora_delta_rows_(y, xin, None, self.lora.layers[i][proj], segments=segs)

        xn = self._layers(x, attn, lora=lora)
        for s_, S, a in zip(slots, lens, aidx):
            self.lens[s_] = S
            self.slot_adapter[s_] = a
        last = torch.tensor([o - 1 for o in offs[1:]], device=self.device)
        return self._logits(xn.index_select(0, last)).float()

    @torch.no_grad()
    def prefill_segments(self, slots: list[int], chunks: list[list[int]], starts: list[int],
                         adapters=None) -> torch.Tensor:
        """The general prefill pass: ``chunks[j]`` are the tokens at positions ``starts[j] ..`` of
        cache slot ``slots[j]``, whose rows [0, starts[j]) are already in the cache (an earlier chunk
        or shared prefix blocks).  The chunks' tokens are concatenated through the GEMMs like
        ``prefill_batch``; attention is ``dops.prefill_attention_paged`` -- RoPE and the cache append
        of the chunk, then causal attention of each chunk over its slot's rows in the block pool.
        Returns the last-row logits of each chunk [n, V] f32.  ``adapters`` as in ``prefill_batch``."""
        m, c = self.model, self.cfg
        if self.kv.fp8 or self.tp is not None:
            raise NotImplementedError("prefill_segments: bf16 KV cache, single GPU")
        ns = [len(ch) for ch in chunks]
        if not (len(slots) == len(chunks) == len(starts)) or any(n <= 0 for n in ns) or any(st < 0 for st in starts):
            raise ValueError("prefill_segments: one non-empty chunk and one start >= 0 per slot")
        if len(set(slots)) != len(slots):
            raise ValueError("prefill_segments: one chunk per slot and pass")
        if any(st + n >= self.max_seq for st, n in zip(starts, ns)):
            raise ValueError(f"prompt exceeds max_seq {self.max_seq}")
        aidx = [self._adapter_index(a) for a in adapters] if adapters is not None else [-1] * len(chunks)
        if len(aidx) != len(chunks):
            raise ValueError("one adapter (or None) per chunk")
        for s_, st, n in zip(slots, starts, ns):
            self._ensure(s_, st + n + 1)
        t = torch.tensor([tok for ch in chunks for tok in ch], dtype=torch.long, device=self.device)
        x = ops.embedding(t, m.tok_emb)
        offs = [0]
        for n in ns:
            offs.append(offs[-1] + n)
        plan = dops.PrefillPlan([(offs[j], ns[j], slots[j], starts[j]) for j in range(len(chunks))], offs[-1],
                                self.device, block_table=self.kv.bt_host)

        def attn(i, qkv):
            return dops.prefill_attention_paged(qkv, m.rope_cos, m.rope_sin, self.kv.k[i], self.kv.v[i], self.kv.bt,
                                                plan, c.n_heads, c.n_kv_heads, c.head_dim)

        lora = None
        if any(a >= 0 for a in aidx):
            segs = ops.lora_serve.merge_segments([a for a, n in zip(aidx, ns) for _ in range(n)])

            def lora(i, proj, y, xin):
                ops.lora_delta_rows_(y, xin, None, self.lora.layers[i][proj], segments=segs)

        xn = self._layers(x, attn, lora=lora)
        for s_, st, n, a in zip(slots, starts, ns, aidx):
            self.lens[s_] = st + n
            self.slot_adapter[s_] = a
        last = torch.tensor([o - 1 for o in offs[1:]], device=self.device)
        return self._logits(xn.index_select(0, last)).float()

    @torch.no_grad()
    def decode(self, slots: list[int], tokens: torch.Tensor) -> torch.Tensor:
        """One token for each sequence in ``slots``; returns logits [B, V]."""
        B = len(slots)
        max_len = max(self.lens[s] for s in slots) + 1
        for s in slots:
            self._ensure(s, self.lens[s] + 1)
        # each row's adapter (table slot, -1 = none); a step in which no row has one is today's step
        aidx = [self.slot_adapter[s] for s in slots] if self.lora is not None else None
        any_adapter = aidx is not None and any(a >= 0 for a in aidx)
        if self.use_graphs:
            logits = self._decode_graphed(slots, tokens, max_len, aidx, any_adapter)
        else:
            rows = [tokens.to(self.device, torch.long),
                    torch.tensor([self.lens[s] for s in slots], device=self.device),
                    torch.tensor(slots, device=self.device)]
            if aidx is not None:
                rows.append(torch.tensor(aidx, device=self.device))
            logits = self._decode_body(torch.stack(rows), max_len, any_adapter)
        for s in slots:
            self.lens[s] += 1
        return logits[:B]

    def _decode_body(self, inp: torch.Tensor, max_len: int, any_adapter: bool = False) -> torch.Tensor:
        """inp int64 [3, B] = (token, position of the new token, cache slot); an engine with adapter
        tables: [4, B], the fourth row each row's adapter table slot (-1 = none).  ``any_adapter``:
        some row has one -- the step runs unfused and every projection adds the rows' deltas
        (``lora_delta_rows_``); otherwise the fourth row is not looked at."""
        m, c = self.model, self.cfg
        pos = inp[1].to(torch.int32)
        sl = inp[2].to(torch.int32)
        x = ops.embedding(inp[0], m.tok_emb)
        lora = None
        if any_adapter:
            ids = inp[3].to(torch.int32)

            def lora(i, proj, y, xin):
                ops.lora_delta_rows_(y, xin, ids, self.lora.layers[i][proj])

        bt = self.kv.bt
        B = inp.shape[1]
        nsplit = (min(max_len, self.kv.maxb * self.kv.block) + 255) // 256
        fp8 = self.kv.fp8
        merge = _MERGE_FUSED and not fp8 and c.head_dim == 128 and B <= 4 and nsplit <= 16
        cnt = self._attn_cnt
        if cnt is not None and B * self.kv.k[0].shape[1] > cnt.numel():
            cnt = None

        pf = self._pf_stream if B <= PREFETCH_MAX_B else None

        def attn(i, qkv, q=None):
            if pf is None:
                return attn_(i, qkv, q)
            wo = getattr(m.layers[i].wo, "weight", None)
            if wo is None or not wo.is_contiguous():
                return attn_(i, qkv, q)
            cur = torch.cuda.current_stream(self.device)
            pf.wait_stream(cur)
            with torch.cuda.stream(pf):
                ops.native().prefetch(wo, 128)
            out = attn_(i, qkv, q)
            cur.wait_stream(pf)  # joins the side branch before the o-projection
            return out

        def attn_(i, qkv, q=None):
            if q is not None:  # RoPE and the cache append already done by the QKV GEMM
                wo = m.layers[i].wo
                K = q.shape[1] * 128  # this rank's heads (tensor parallel: a shard)
                if merge and type(wo) is FusedLinear and wo.lora_r == 0 and ops.merge_linear_ok(B, K, wo.weight):
                    # partials only: the split merge runs in the o-projection's prologue
                    return ops.native().decode_attn_partials(q, self.kv.k[i], self.kv.v[i], pos, sl, max_len,
                                                             1.0 / math.sqrt(c.head_dim), 1, bt)
                return ops.native().decode_attn(q, self.kv.k[i], self.kv.v[i], pos, sl, max_len,
                                                1.0 / math.sqrt(c.head_dim), 1, bt, cnt)
            if fp8:
                return dops.decode_attention(qkv, m.rope_cos, m.rope_sin, self.kv.k[i], self.kv.v[i], pos, sl,
                                             c.n_heads, c.n_kv_heads, c.head_dim, max_len, bt,
                                             k_scale=self.kv.k_scale[i], v_scale=self.kv.v_scale[i])
            return dops.decode_attention(qkv, m.rope_cos, m.rope_sin, self.kv.k[i], self.kv.v[i], pos, sl,
                                         c.n_heads, c.n_kv_heads, c.head_dim, max_len, bt, cnt)

        qkv_fn = self._qkv_rope_fn(pos, sl)
        xn = self._layers(x, attn, qkv_fn if lora is None else None, lora=lora)
        return self._logits(xn)

    def _qkv_rope_fn(self, pos: torch.Tensor, sl: torch.Tensor):
        """``_layers``' ``qkv_fn`` of a decode or verify step whose rows are appended at position
        ``pos[r]`` of slot ``sl[r]``: what it fuses depends on the rows of the step, not on its
        sequences (``ops.qkv_rope_linear`` / ``qkv_rope_ok`` look at h)."""
        m, c = self.model, self.cfg
        bt, fp8 = self.kv.bt, self.kv.fp8

        def qkv_fn(i, delta, h, gamma, layer):
            # QKV GEMM with the RoPE/cache-append epilogue; 1-2 rows also with the RMSNorm prologue
            # (one launch), more rows after the RMSNorm kernel
            # (not into an fp8 cache: a row's amax spans the workgroups of that epilogue)
            if not (_ROPE_FUSED and not fp8 and self.tp is None and c.head_dim == 128
                    and type(layer.wqkv) is FusedLinear and layer.wqkv.lora_r == 0):
                return None
            rope = (layer.wqkv.weight, m.rope_cos, m.rope_sin, pos, sl, self.kv.k[i], self.kv.v[i],
                    c.n_heads, c.n_kv_heads, bt)
            if _NORM_FUSED:
                r = ops.qkv_rope_linear(delta, h, gamma, c.norm_eps, *rope)
                if r is not None:
                    return r
            if not ops.qkv_rope_ok(h, layer.wqkv.weight, m.rope_cos, m.rope_sin, self.kv.k[i], self.kv.v[i],
                                   Hq=c.n_heads, Hkv=c.n_kv_heads, norm=False):
                return None
            if delta is None:
                xn = ops.rms_norm(h, gamma, c.norm_eps)
            else:
                xn, h = ops.add_rms_norm(delta, h, gamma, c.norm_eps)
            q, _ = ops.qkv_rope_linear(None, xn, None, c.norm_eps, *rope)
            return q, h

        return qkv_fn

    def _buckets(self, B: int, max_len: int) -> tuple[int, int]:
        bb = 1
        while bb < B:
            bb *= 2
        bb = min(bb, self.max_batch)
        ns, cap = (max_len + 255) // 256, (self.max_seq + 255) // 256
        nb = 1
        while nb < ns:
            nb *= 2
        return bb, min(nb, cap) * 256

    def _decode_graphed(self, slots: list[int], tokens: torch.Tensor, max_len: int, aidx=None,
                        any_adapter: bool = False) -> torch.Tensor:
        B = len(slots)
        bb, kl = self._buckets(B, max_len)
        entry = self._graphs.get((bb, kl, any_adapter))
        if entry is None:
            entry = self._capture(bb, kl, any_adapter)
        inp, out, graph, host = entry
        if aidx is not None:  # padding rows: no adapter
            host[3, :B] = torch.tensor(aidx)
            host[3, B:] = -1
        # the previous step's copy from ``host`` has completed: its logits were
        # read back (sampling) before this step was scheduled
        host[0, :B] = tokens.to("cpu", torch.long)
        host[1, :B] = torch.tensor([self.lens[s] for s in slots])
        host[2, :B] = torch.tensor(slots)
        host[0, B:] = 0
        host[1, B:] = 0
        host[2, B:] = self.scratch_slot
        inp.copy_(host, non_blocking=True)
        graph.replay()
        return out

    def _capture(self, bb: int, kl: int, any_adapter: bool = False):
        """One graph per (batch bucket, key bucket, any_adapter).  The adapter tables are static
        buffers read through the step's ids, so loading or unloading an adapter leaves every
        captured graph valid; warm-up rows use table slot 0, whatever it holds."""
        inp = torch.zeros(3 if self.lora is None else 4, bb, dtype=torch.long, device=self.device)
        inp[2].fill_(self.scratch_slot)  # warm-up / capture traffic goes to the scratch slot
        side = torch.cuda.Stream(self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            for _ in range(2):  # library handles / workspace set up outside capture
                self._decode_body(inp, kl, any_adapter)
        torch.cuda.current_stream(self.device).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        if self._pool is None:
            self._pool = torch.cuda.graph_pool_handle()
        with torch.cuda.graph(graph, pool=self._pool, capture_error_mode="thread_local"):
            out = self._decode_body(inp, kl, any_adapter)
        host = torch.empty(inp.shape[0], bb, dtype=torch.long, pin_memory=True)
        self._graphs[(bb, kl, any_adapter)] = (inp, out, graph, host)
        log.debug("captured decode graph: batch %d, key bound %d, adapters %s", bb, kl, any_adapter)
        return self._graphs[(bb, kl, any_adapter)]

    # ------------------------------------------------------------------ speculative decoding
    @torch.no_grad()
    def verify(self, slots: list[int], rows: list[list[int]]):
        """One verify step: ``rows[i]`` are the tokens at positions ``lens[s] ..`` of ``slots[i]`` -- the
        sequence's last token and its drafts, 1 .. speculate + 1 of them.  Every row's K/V are appended
        at its position and row j attends over keys 0 .. lens[s] + j.  Returns (logits [B * n, V], the
        rows' tokens [B, n] and the sequences' row counts [B] on the device, what ``dops.spec_accept``
        takes); n = speculate + 1, sequence i's row j at ``i * n + j`` (rows past ``len(rows[i])`` are padding).
        ``lens`` is NOT advanced: the caller keeps what it accepts (``lens[s] += accepted + 1``); the
        K/V rows of rejected drafts stay behind as stale rows past ``lens``, which nothing reads and
        the next step overwrites (kv8: codes and scales alike)."""
        n, B = self.speculate + 1, len(slots)
        if n < 2:
            raise ValueError("verify: the engine was built without speculate")
        if any(not 1 <= len(r) <= n for r in rows) or len(rows) != B:
            raise ValueError(f"verify: 1 .. {n} rows per sequence")
        if self.lora is not None and any(self.slot_adapter[s] >= 0 for s in slots):
            raise ValueError("verify: sequences on a LoRA adapter take the plain step")
        for s_, r in zip(slots, rows):
            self._ensure(s_, self.lens[s_] + len(r))
        max_len = max(self.lens[s_] + len(r) for s_, r in zip(slots, rows))
        if self.use_graphs:
            bb, kl = self._buckets(B, max_len)
            entry = self._graphs.get(("verify", bb, kl, n)) or self._capture_verify(bb, kl, n)
            inp, out, graph, host = entry
        else:
            bb = B
            host = torch.empty(3 * bb * (n + 1), dtype=torch.long)
        # host: (token, position, slot) of every row [3, bb * n], then (base length, rows in use, slot) of
        # every sequence [3, bb]; rows not in use: token 0, position 0, the spare slot
        rv, sv = host[:3 * bb * n].view(3, bb, n), host[3 * bb * n:].view(3, bb)
        rv[0].zero_()
        rv[1].zero_()
        rv[2].fill_(self.scratch_slot)
        sv[0].zero_()
        sv[1].zero_()
        sv[2].fill_(self.scratch_slot)
        for i, (s_, r) in enumerate(zip(slots, rows)):
            L, m = self.lens[s_], len(r)
            rv[0, i, :m] = torch.tensor(r)
            rv[1, i, :m] = torch.arange(L, L + m)
            rv[2, i, :m] = s_
            sv[0, i], sv[1, i], sv[2, i] = L, m, s_
        if self.use_graphs:
            inp.copy_(host, non_blocking=True)
            graph.replay()
        else:
            inp = host.to(self.device)
            out = self._verify_body(inp, bb, max_len, n)
        return out[:B * n], inp[:bb * n].view(bb, n)[:B], inp[3 * bb * n + bb:3 * bb * n + 2 * bb][:B]

    def _verify_body(self, inp: torch.Tensor, bb: int, max_len: int, n: int) -> torch.Tensor:
        """inp int64 [3 * bb * n + 3 * bb]: ``verify``'s row and sequence tables.  A decode step over
        bb * n rows whose attention is ``dops.verify_attention``.  The shortcuts of ``_decode_body``
        that assume one row per sequence do not apply here: the split merge in the o-projection and
        the in-launch combine counters are not used, and the fused QKV prologue / epilogue decide by
        the rows of the step (``_qkv_rope_fn``)."""
        m, c = self.model, self.cfg
        rows, seq = inp[:3 * bb * n].view(3, bb * n), inp[3 * bb * n:].view(3, bb)
        pos, sl = rows[1].to(torch.int32), rows[2].to(torch.int32)
        lens, nq, ssl = seq[0].to(torch.int32), seq[1].to(torch.int32), seq[2].to(torch.int32)
        x = ops.embedding(rows[0], m.tok_emb)
        bt = self.kv.bt
        scales = (lambda i: (self.kv.k_scale[i], self.kv.v_scale[i])) if self.kv.fp8 else (lambda i: (None, None))

        def attn(i, qkv, q=None):
            ks, vs = scales(i)
            return dops.verify_attention(qkv, m.rope_cos, m.rope_sin, self.kv.k[i], self.kv.v[i], pos, sl, lens, nq, ssl,
                                         n, c.n_heads, c.n_kv_heads, c.head_dim, max_len, bt, ks, vs, q=q)

        xn = self._layers(x, attn, self._qkv_rope_fn(pos, sl))
        return self._logits(xn)

    def _capture_verify(self, bb: int, kl: int, n: int):
        """One graph per (sequence bucket, key bucket, n): rows laid out [bb, n]."""
        inp = torch.zeros(3 * bb * (n + 1), dtype=torch.long, device=self.device)
        inp[2 * bb * n:3 * bb * n].fill_(self.scratch_slot)  # warm-up / capture traffic goes to the spare slot
        inp[3 * bb * n + 2 * bb:].fill_(self.scratch_slot)
        side = torch.cuda.Stream(self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            for _ in range(2):  # library handles / workspace set up outside capture
                self._verify_body(inp, bb, kl, n)
        torch.cuda.current_stream(self.device).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        if self._pool is None:
            self._pool = torch.cuda.graph_pool_handle()
        with torch.cuda.graph(graph, pool=self._pool, capture_error_mode="thread_local"):
            out = self._verify_body(inp, bb, kl, n)
        host = torch.empty(inp.shape[0], dtype=torch.long, pin_memory=True)
        self._graphs[("verify", bb, kl, n)] = (inp, out, graph, host)
        log.debug("captured verify graph: %d sequences x %d rows, key bound %d", bb, n, kl)
        return self._graphs[("verify", bb, kl, n)]

    def _drafts(self, reqs) -> list[list[int]]:
        """At most ``min(speculate, remaining new tokens - 1)`` drafted tokens per request, and never a
        position past what the slot holds; none for requests whose token state depends on every
        earlier token (penalties, logit_bias, logprobs)."""
        out = []
        for r in reqs:
            k = min(self.speculate, r.params.max_new_tokens - len(r.output) - 1,
                    self.kv.capacity(r.slot) - self.lens[r.slot] - 2)
            if k <= 0 or r.special:
                out.append([])
                continue
            toks = r.prompt + r.output
            if self.drafter is not None:
                d = list(self.drafter(toks, k))[:k]
            else:
                if r.spec_index is None:
                    from .speculate import NgramIndex

                    r.spec_index = NgramIndex()
                r.spec_index.sync(toks)
                d = r.spec_index.propose(k)
            d = [int(t) for t in d]
            out.append(d if all(0 <= t < self.vocab for t in d) else [])  # (a drafter's stray id: no draft)
        return out

    def _verify_step(self, slots, reqs, drafts) -> None:
        """The decode part of ``step`` when some request has a draft: one ``verify`` pass, the sampler
        on every row (row j of a request draws with its step + j), ``spec_accept``, one read-back.
        Requests with penalties, logit_bias or logprobs have one row, sampled by ``_sample`` on that row
        (a step that carries such a request beside drafted ones reads back twice)."""
        n, B = self.speculate + 1, len(reqs)
        rows = [[r.output[-1]] + d for r, d in zip(reqs, drafts)]
        logits, tokens, nq = self.verify(slots, rows)
        self.steps += 1
        self.spec_steps += 1
        # sampling parameters per row; rows not in use draw greedily and are ignored
        temps, top_ps, top_ks, seeds, steps = ([0.0] * (B * n), [1.0] * (B * n), [0] * (B * n), [0] * (B * n),
                                               [0] * (B * n))
        for i, (r, row) in enumerate(zip(reqs, rows)):
            p = r.params
            for j in range(len(row)):
                k = i * n + j
                temps[k], top_ps[k], top_ks[k], seeds[k] = p.temperature, p.top_p, p.top_k, p.seed
                steps[k] = len(r.output) + j
        special = [i for i, r in enumerate(reqs) if r.special]
        sp_toks = {}
        if special:  # one row each: the adjusted sampling path, on that row
            idx = torch.tensor([i * n for i in special], device=logits.device)
            sub = [reqs[i] for i in special]
            sp_toks = dict(zip(special, self._sample(logits.index_select(0, idx), sub)))
        drawn = dops.sample_rows(logits, temps, top_ps, top_ks, seeds, steps)
        acc = dops.spec_accept(drawn.view(-1, n)[:B], tokens, nq).tolist()  # the step's read-back
        for i, (r, d) in enumerate(zip(reqs, drafts)):
            a = acc[i][0]
            emitted = [sp_toks[i]] if i in sp_toks else acc[i][1:a + 2]
            self.spec_draft_tokens += len(d)
            self.spec_accepted_tokens += a if i not in sp_toks else 0
            self.decode_tokens += len(emitted)
            slot = r.slot
            for t in emitted:  # one by one: streaming, stop and length handling are the plain step's
                self.lens[slot] += 1
                self._accept(r, int(t))
                if r.done.is_set():
                    break  # an EOS / stop / length inside the run: later tokens are dropped

    # ------------------------------------------------------------------ scheduling
    # ------------------------------------------------------------------ embeddings
    @torch.no_grad()
    def _embed_now(self, prompts: list[list[int]]) -> torch.Tensor:
        if self.tp is not None:
            raise NotImplementedError("embeddings are served by single-GPU engines")
        out = []
        for ids in prompts:
            if not ids:
                raise ValueError("empty input")
            if len(ids) >= self.max_seq:
                raise ValueError(f"input of {len(ids)} tokens exceeds max_seq {self.max_seq}")
            t = torch.tensor([ids], dtype=torch.long, device=self.device)
            h = self.model.hidden_states(t).float()  # [S, H], final RMSNorm applied (no KV cache touched)
            out.append(torch.nn.functional.normalize(h.mean(0), dim=0))
        return torch.stack(out).cpu()

    def embed(self, prompts: list[list[int]], adapter: str | None = None) -> torch.Tensor:
        """Sentence embeddings [n, hidden] (f32, unit norm): the mean of the final
        normed hidden states over each input's tokens.  With the background loop
        running the pass runs on the engine thread between decode steps (it shares
        the model's kernels and workspaces with generation); otherwise inline."""
        if adapter is not None:
            raise NotImplementedError("embeddings with a LoRA adapter are not supported")
        if self._thread is None:
            return self._embed_now(prompts)
        box, ev = {}, threading.Event()

        def task():
            try:
                box["out"] = self._embed_now(prompts)
            except Exception as e:  # noqa: BLE001
                box["err"] = e
            ev.set()

        with self._cv:
            self._tasks.append(task)
            self._cv.notify()
        ev.wait()
        if "err" in box:
            raise box["err"]
        return box["out"]

    def _run_tasks(self) -> None:
        with self._lock:
            tasks, self._tasks = self._tasks, []
        for t in tasks:
            t()

    # ------------------------------------------------------------------ LoRA adapters
    def _between_steps(self, fn):
        """Run ``fn`` on the engine thread between steps when the loop is running, else inline."""
        if self._thread is None or threading.current_thread() is self._thread:
            return fn()
        box, ev = {}, threading.Event()

        def task():
            try:
                box["out"] = fn()
            except Exception as e:  # noqa: BLE001
                box["err"] = e
            ev.set()

        with self._cv:
            self._tasks.append(task)
            self._cv.notify()
        ev.wait()
        if "err" in box:
            raise box["err"]
        return box["out"]

    def load_adapter(self, name: str, path_or_tensors) -> int:
        """Load a LoRA adapter (a PEFT directory, or what ``mxllm.models.adapter.load_adapter``
        returns) into a free table slot under ``name``; requests then name it.  The copy runs
        between steps; the tables are static, so no captured graph is invalidated.  Returns the slot."""
        if self.lora is None:
            raise ValueError("this engine has no adapter tables (max_adapters = 0)")
        if not isinstance(name, str) or not name:
            raise ValueError("an adapter needs a non-empty name")
        ad = path_or_tensors
        if isinstance(ad, (str, os.PathLike)):
            from ..models.adapter import load_adapter

            ad = load_adapter(os.fspath(ad), self.cfg, r_max=self.lora.r_max, dtype=self.model.tok_emb.dtype)

        def do():
            if name in self.adapters:
                raise ValueError(f"adapter {name!r} is already loaded")
            used = set(self.adapters.values())
            free = [i for i in range(self.lora.n_adapters) if i not in used]
            if not free:
                raise ValueError(f"all {self.lora.n_adapters} adapter slots are in use")
            self.lora.put(free[0], ad)
            self.adapters[name] = free[0]
            return free[0]

        return self._between_steps(do)

    def unload_adapter(self, name: str) -> None:
        """Free the adapter's slot (zeroed).  Refused while a waiting or active request uses it."""

        def do():
            if name not in self.adapters:
                raise ValueError(f"unknown LoRA adapter {name!r}")
            with self._lock:
                busy = any(r.adapter == name
                           for r in list(self.waiting) + self.prefilling + list(self.active.values()))
            if busy:
                raise ValueError(f"adapter {name!r} is in use by a waiting or active request")
            self.lora.clear(self.adapters.pop(name))
            self.kv.drop_adapter(name)  # the prefix cache's entries of this adapter

        return self._between_steps(do)

    def submit(self, prompt: list[int], params: SamplingParams | None = None, adapter: str | None = None) -> Request:
        r = Request(next(self._ids), list(prompt), params or SamplingParams(), adapter=adapter)
        with self._cv:
            self.waiting.append(r)
            self._cv.notify()
        return r

    def stats(self) -> dict:
        """Cumulative serving metrics: TTFT / request latency means, prefill and
        decode throughput (tokens/s of engine wall time)."""
        n = max(self.finished, 1)
        return {"requests_finished": self.finished, "tokens_generated": self.tokens_generated,
                "mean_ttft_s": self.ttft_sum / n, "mean_latency_s": self.latency_sum / n,
                "prefill_tokens_per_s": self.prefill_tokens / self.prefill_s if self.prefill_s else 0.0,
                "decode_tokens_per_s": self.decode_tokens / self.decode_s if self.decode_s else 0.0,
                "decode_steps": self.steps, "kv_cache_dtype": self.kv_dtype, "kv_cache_bytes": self.kv.nbytes(),
                "lora_adapters": sorted(self.adapters), "prefix_cache_query_tokens": self.prefix_query_tokens,
                "prefix_cache_hit_tokens": self.prefix_hit_tokens, "prefill_chunks": self.prefill_chunks,
                "spec_steps": self.spec_steps, "spec_draft_tokens": self.spec_draft_tokens,
                "spec_accepted_tokens": self.spec_accepted_tokens}

    def _finish(self, r: Request, reason: str):
        r.finish_reason = reason
        r.t_done = time.perf_counter()
        self.finished += 1
        self.latency_sum += r.t_done - r.t_submit
        if r.t_first is not None:
            self.ttft_sum += r.t_first - r.t_submit
        if r in self.prefilling:
            self.prefilling.remove(r)
        if r.slot >= 0:
            if self.prefix_cache:
                # prompt and output: what multi-turn chat resends.  Only blocks below the slot's written
                # length (a request that failed mid-prefill registers only fully written blocks)
                self.kv.register(r.slot, r.prompt + r.output, r.adapter, upto=self.lens[r.slot])
            self.kv.release(r.slot)
            self.slot_adapter[r.slot] = -1
            self.free_slots.append(r.slot)
            self.active.pop(r.slot, None)
            r.slot = -1
        r.done.set()

    def _accept(self, r: Request, tok: int):
        if r.t_first is None:
            r.t_first = time.perf_counter()
        r.output.append(tok)
        self.tokens_generated += 1
        p = r.params
        if tok in self.eos_ids or tok in p.stop_ids:
            self._finish(r, "stop")
        elif len(r.output) >= p.max_new_tokens:
            self._finish(r, "length")
        elif self.lens[r.slot] + 1 >= self.kv.capacity(r.slot):
            self._finish(r, "length")

    def enable_tp_sync(self) -> None:
        """Server mode of a tensor-parallel group: requests arrive on group rank 0
        only; every ``step`` rank 0 broadcasts the requests it admits (prompt +
        sampling params, usually an empty list) and the other ranks, running
        ``follow()``, admit the same requests into the same slots.  The schedule
        is deterministic from there on (identical logits on every rank)."""
        if self.tp is None:
            return
        self.tp_sync = True
        self._tp_stop = False

    def _sync_admit(self, admit: list, stopping: bool = False) -> list:
        """``stopping`` (rank 0): broadcast the stop sentinel instead of admissions.  It is
        an argument, not a read of ``self._stop``: a stop() arriving mid-step must not turn
        this step's broadcast into the sentinel while rank 0 still runs the step's
        collectives (the followers would have left them)."""
        import torch.distributed as dist

        src = dist.get_global_rank(self.tp.group, 0)
        dev = self.device if dist.get_backend(self.tp.group) == "nccl" else torch.device("cpu")
        if self.tp.rank == 0:
            payload = [None if stopping else [(r.prompt, r.params) for r in admit]]
            dist.broadcast_object_list(payload, src=src, group=self.tp.group, device=dev)
            return admit
        payload = [None]
        dist.broadcast_object_list(payload, src=src, group=self.tp.group, device=dev)
        if payload[0] is None:
            self._tp_stop = True
            return []
        mirrored = []
        for prompt, params in payload[0]:
            r = Request(next(self._ids), list(prompt), params)
            r.slot = self.free_slots.pop(0)
            self.kv.reserve(r.slot, len(r.prompt) + params.max_new_tokens)
            mirrored.append(r)
        return mirrored

    def follow(self) -> None:
        """Non-zero ranks of a TP serving group: mirror rank 0's schedule until it
        stops (``enable_tp_sync`` first)."""
        self.enable_tp_sync()
        while not self._tp_stop:
            self.step()

    def step(self) -> bool:
        """Admit + prefill waiting requests into free slots, then one decode step
        for the running batch.  Returns False when there is nothing to do.
        With ``prefix_cache`` / ``prefill_chunk`` on: at admission the request's prompt is matched
        against the cached blocks under its adapter (it starts at position 256 * matched blocks and
        reserves prompt + max_new_tokens with those blocks shared), and the prefill part is
        ``_prefill_paged``.  Two new requests of one admission pass that share a prefix both miss."""
        with self._lock:
            admit, rejected = [], []
            while self.waiting and self.free_slots:
                r = self.waiting[0]
                need = len(r.prompt) + r.params.max_new_tokens
                if not self.kv.fits_at_all(need):  # larger than the whole KV pool
                    self.waiting.pop(0)
                    r.error = f"request needs {need} KV positions, more than the pool"
                    rejected.append(r)
                    continue
                bad = [t for t in (r.params.logit_bias or ()) if not 0 <= t < self.vocab]
                if bad:
                    self.waiting.pop(0)
                    r.error = f"logit_bias token id {bad[0]} outside the vocabulary [0, {self.vocab})"
                    rejected.append(r)
                    continue
                if r.adapter is not None and r.adapter not in self.adapters:
                    self.waiting.pop(0)
                    r.error = f"unknown LoRA adapter {r.adapter!r}"
                    rejected.append(r)
                    continue
                if self.paged_prefill and not 0 < len(r.prompt) < self.max_seq:
                    # (known before the first chunk runs, not after the last one)
                    self.waiting.pop(0)
                    r.error = f"prompt of {len(r.prompt)} tokens: must hold 1 .. max_seq - 1 = {self.max_seq - 1}"
                    rejected.append(r)
                    continue
                shared = self.kv.match_prefix(r.prompt, r.adapter) if self.prefix_cache else []
                if not self.kv.can_reserve(need, shared):  # paged pool full: wait for finishing requests
                    break
                self.waiting.pop(0)
                r.slot = self.free_slots.pop(0)
                self.kv.reserve(r.slot, need, shared=shared)
                if self.paged_prefill:
                    r.cached_tokens = r.prefilled = len(shared) * self.kv.block
                    self.lens[r.slot] = r.prefilled
                    if self.prefix_cache:
                        self.prefix_query_tokens += len(r.prompt)
                        self.prefix_hit_tokens += r.cached_tokens
                admit.append(r)
        for r in rejected:
            self._finish(r, "error")
        if getattr(self, "tp_sync", False):
            admit = self._sync_admit(admit)
        for r in admit:
            self._admit_state(r)
        if self.paged_prefill:
            self.prefilling.extend(admit)
            self._prefill_paged()
            admit = []  # (their prefill ran, or goes on in later steps)
        # admitted prompts are prefilled together, in groups of at most
        # prefill_tokens tokens (bounds the activation memory of one pass)
        groups, cur, ntok = [], [], 0
        for r in admit:
            if cur and ntok + len(r.prompt) > self.prefill_budget:
                groups.append(cur)
                cur, ntok = [], 0
            cur.append(r)
            ntok += len(r.prompt)
        if cur:
            groups.append(cur)
        for grp in groups:
            try:
                t0 = time.perf_counter()
                logits = self.prefill_batch([r.slot for r in grp], [r.prompt for r in grp],
                                            [r.adapter for r in grp] if self.lora is not None else None)
                for r in grp:
                    self.active[r.slot] = r
                toks = self._sample(logits, grp, first=True)
                self.prefill_s += time.perf_counter() - t0
                for r, tok in zip(grp, toks):
                    self.prefill_tokens += len(r.prompt)
                    self._accept(r, tok)
            except Exception as e:  # noqa: BLE001
                log.exception("prefill failed")
                for r in grp:
                    self.active.pop(r.slot, None)
                    r.error = str(e)
                    self._finish(r, "error")
        if not self.active:
            return bool(admit) or bool(self.prefilling)
        slots = sorted(self.active)
        reqs = [self.active[s] for s in slots]
        t0 = time.perf_counter()
        tokens = torch.tensor([r.output[-1] for r in reqs], dtype=torch.long)
        if self.speculate and not (self.lora is not None and any(self.slot_adapter[s_] >= 0 for s_ in slots)):
            drafts = self._drafts(reqs)
            if any(drafts):
                self._verify_step(slots, reqs, drafts)
                self.decode_s += time.perf_counter() - t0
                return True
        logits = self.decode(slots, tokens)
        self.steps += 1
        nxt = self._sample(logits, reqs)
        self.decode_s += time.perf_counter() - t0  # includes the sampling read-back (a sync)
        self.decode_tokens += len(reqs)
        for r, t in zip(reqs, nxt):
            self._accept(r, int(t))
        return True

    def _prefill_paged(self) -> None:
        """The prefill part of a step with ``prefix_cache`` or ``prefill_chunk`` on.  Requests still
        prefilling go first, FIFO, then the new admissions.  ``prefill_chunk`` = N: ONE pass of at
        most N tokens, the last segment cut to fit; unset: the uncached remainders, grouped by
        ``prefill_tokens`` like ``prefill_batch``'s groups.  A request whose prompt completes in a
        pass is sampled and joins ``active``; its prompt's full blocks are registered at once, so
        later admissions share them while it still runs."""
        passes, cur, ntok = [], [], 0
        if self.prefill_chunk is not None:
            left = self.prefill_chunk
            for r in self.prefilling:
                n = min(len(r.prompt) - r.prefilled, left)
                if n <= 0:
                    break
                cur.append((r, n))
                left -= n
        else:
            for r in self.prefilling:
                n = len(r.prompt) - r.prefilled
                if cur and ntok + n > self.prefill_budget:
                    passes.append(cur)
                    cur, ntok = [], 0
                cur.append((r, n))
                ntok += n
        if cur:
            passes.append(cur)
        for grp in passes:
            reqs = [r for r, _ in grp]
            try:
                t0 = time.perf_counter()
                logits = self.prefill_segments([r.slot for r in reqs], [r.prompt[r.prefilled:r.prefilled + n] for r, n in grp],
                                               [r.prefilled for r in reqs],
                                               [r.adapter for r in reqs] if self.lora is not None else None)
                self.prefill_chunks += len(grp)
                done = []
                for j, (r, n) in enumerate(grp):
                    r.prefilled += n
                    self.prefill_tokens += n
                    if r.prefilled == len(r.prompt):
                        done.append(j)
                if done:
                    fin = [reqs[j] for j in done]
                    for r in fin:
                        self.prefilling.remove(r)
                        self.active[r.slot] = r
                        if self.prefix_cache:
                            self.kv.register(r.slot, r.prompt, r.adapter, upto=len(r.prompt))
                    rows = logits if len(done) == len(grp) else logits[torch.tensor(done, device=logits.device)]
                    toks = self._sample(rows, fin, first=True)
                    for r, tok in zip(fin, toks):
                        self._accept(r, tok)
                self.prefill_s += time.perf_counter() - t0
            except Exception as e:  # noqa: BLE001
                log.exception("prefill failed")
                for r in reqs:
                    self.active.pop(r.slot, None)
                    r.error = str(e)
                    self._finish(r, "error")

    def _admit_state(self, r: Request) -> None:
        """Device state of a request that uses a penalty or a logit_bias: its slot's rows of
        the token state (prompt flags set, counts zero) and of the bias table.  Both tables
        are allocated by the first request that needs them; a request that needs neither
        touches nothing."""
        p = r.params
        if not p.adjusts:
            return
        if p.penalised and self._tok_state is None:
            self._tok_state = torch.zeros(self.max_batch, self.vocab, dtype=torch.int32, device=self.device)
        if p.logit_bias and self._tok_bias is None:
            self._tok_bias = torch.zeros(self.max_batch, self.vocab, dtype=torch.float32, device=self.device)
        # an adjusted row reads its slot's row of both tables: clear what an earlier tenant left
        if self._tok_state is not None:
            self._tok_state[r.slot].zero_()
            if p.penalised:
                seen = sorted({t for t in r.prompt if 0 <= t < self.vocab})
                if seen:
                    self._tok_state[r.slot, torch.tensor(seen, device=self.device)] = dops.PROMPT_FLAG
        if self._tok_bias is not None:
            self._tok_bias[r.slot].zero_()
            if p.logit_bias:
                ids = torch.tensor(list(p.logit_bias), device=self.device)
                self._tok_bias[r.slot, ids] = torch.tensor(list(p.logit_bias.values()), dtype=torch.float32,
                                                           device=self.device)

    def _sample(self, logits: torch.Tensor, reqs, first: bool = False) -> list[int]:
        """One batched draw for every row of ``logits`` with each request's own
        temperature / top-k / top-p; per-request RNG stream keyed by (seed, token
        index), so draws do not depend on batching.  One host read-back.

        A batch in which some request uses a penalty, a logit_bias or logprobs: the logits
        are adjusted (``dops.adjust_logits_rows``, f32; skipped when only logprobs are asked
        for), sampled, the drawn tokens counted for the penalised rows, and the
        log-probabilities taken (``dops.logprob_rows``) of the adjusted logits -- after
        penalties and bias, before temperature and the top-k / top-p cut.  bf16 -> f32 is
        exact and the noise is keyed by (seed, step, token), so a request without
        penalties draws the same tokens in such a batch as alone.  Still one read-back."""
        ps = [r.params for r in reqs]
        steps = [0 if first else len(r.output) for r in reqs]
        if not any(r.special for r in reqs):
            return dops.sample_rows(logits[:len(reqs)], [p.temperature for p in ps], [p.top_p for p in ps],
                                    [p.top_k for p in ps], [p.seed for p in ps], steps).tolist()
        x = logits[:len(reqs)]
        adj = [p.adjusts for p in ps]
        want_lp = [p.logprobs is not None for p in ps]
        if any(adj):
            x = dops.adjust_logits_rows(
                x, self._tok_state, [r.slot if a else -1 for r, a in zip(reqs, adj)],
                [p.presence_penalty for p in ps], [p.frequency_penalty for p in ps],
                [p.repetition_penalty for p in ps], self._tok_bias)
        ids = dops.sample_rows(x, [p.temperature for p in ps], [p.top_p for p in ps], [p.top_k for p in ps],
                               [p.seed for p in ps], steps)
        if any(p.penalised for p in ps):
            dops.token_state_update(self._tok_state, [r.slot if p.penalised else -1 for r, p in zip(reqs, ps)], ids)
        if not any(want_lp):
            return ids.tolist()
        chosen, top_ids, top_lp = dops.logprob_rows(x, ids, [p.logprobs if w else -1 for p, w in zip(ps, want_lp)])
        # one read-back: ids | chosen | top ids | top logprobs as int32 words
        host = torch.cat([ids.to(torch.int32).view(-1, 1), chosen.view(torch.int32).view(-1, 1), top_ids,
                          top_lp.view(torch.int32)], 1).cpu()
        toks = host[:, 0].tolist()
        lps = host[:, 1].contiguous().view(torch.float32).tolist()
        tids = host[:, 2:2 + dops.TOP_LOGPROBS_MAX].tolist()
        tlps = host[:, 2 + dops.TOP_LOGPROBS_MAX:].contiguous().view(torch.float32).tolist()
        for i, (r, p) in enumerate(zip(reqs, ps)):
            if want_lp[i]:
                r.logprobs.append((lps[i], list(zip(tids[i][:p.logprobs], tlps[i][:p.logprobs]))))
        return toks

    # ------------------------------------------------------------------ prompt scoring
    SCORE_ROWS = 2048  # logits rows per head GEMM of ``score`` (bounds the [rows, vocab] buffer)

    @torch.no_grad()
    def _score_now(self, prompts: list[list[int]], top: int = 0) -> list[list]:
        if self.tp is not None:
            raise NotImplementedError("prompt scoring is served by single-GPU engines")
        if not 0 <= top <= dops.TOP_LOGPROBS_MAX:
            raise ValueError(f"top must be in 0..{dops.TOP_LOGPROBS_MAX}, got {top}")
        out = []
        for ids in prompts:
            if not ids:
                raise ValueError("empty input")
            if len(ids) >= self.max_seq:
                raise ValueError(f"input of {len(ids)} tokens exceeds max_seq {self.max_seq}")
            t = torch.tensor([ids], dtype=torch.long, device=self.device)
            h = self.model.hidden_states(t)  # [S, H], final RMSNorm applied (no KV cache touched)
            parts = []
            for a in range(0, len(ids) - 1, self.SCORE_ROWS):
                b = min(len(ids) - 1, a + self.SCORE_ROWS)
                lp = dops.logprob_rows(self._logits(h[a:b]), t[0, a + 1:b + 1], [top] * (b - a))
                parts.append(torch.cat([lp[0].view(torch.int32).view(-1, 1), lp[1], lp[2].view(torch.int32)], 1))
            entries = [None]
            if parts:
                host = torch.cat(parts, 0).cpu()
                lps = host[:, 0].contiguous().view(torch.float32).tolist()
                tids = host[:, 1:1 + dops.TOP_LOGPROBS_MAX].tolist()
                tlps = host[:, 1 + dops.TOP_LOGPROBS_MAX:].contiguous().view(torch.float32).tolist()
                entries += [(lps[i], list(zip(tids[i][:top], tlps[i][:top]))) for i in range(len(lps))]
            out.append(entries)
        return out

    def score(self, prompts: list[list[int]], top: int = 0, adapter: str | None = None) -> list[list]:
        """Prompt scoring: for each prompt one entry per position -- None for the first
        token, then (logprob of token t+1 given tokens <= t, [(id, logprob), ...] of the
        ``top`` most likely tokens there).  One full forward per prompt (no KV cache
        touched), the head GEMM and ``logprob_rows`` over chunks of at most ``SCORE_ROWS``
        rows.  Runs on the engine thread between decode steps like ``embed``."""
        if adapter is not None:
            raise NotImplementedError("prompt scoring with a LoRA adapter is not supported")
        if self._thread is None:
            return self._score_now(prompts, top)
        box, ev = {}, threading.Event()

        def task():
            try:
                box["out"] = self._score_now(prompts, top)
            except Exception as e:  # noqa: BLE001
                box["err"] = e
            ev.set()

        with self._cv:
            self._tasks.append(task)
            self._cv.notify()
        ev.wait()
        if "err" in box:
            raise box["err"]
        return box["out"]

    def generate(self, prompts: list[list[int]], max_new_tokens: int = 32, temperature: float = 0.0,
                 top_p: float = 1.0, top_k: int = 0, stop_ids=(), seed: int = 0, *, presence_penalty: float = 0.0,
                 frequency_penalty: float = 0.0, repetition_penalty: float = 1.0, logit_bias: dict | None = None,
                 logprobs: int | None = None, return_requests: bool = False, adapters=None):
        """Synchronous batched generation (continuous batching when
        len(prompts) > max_batch).  ``return_requests``: the finished ``Request`` objects
        (``.output``, ``.logprobs``, ``.finish_reason``, ``.error``) instead of the token lists.
        ``adapters``: one loaded LoRA adapter's name or None per prompt."""
        if adapters is not None and len(adapters) != len(prompts):
            raise ValueError("adapters: one name or None per prompt")
        reqs = [self.submit(p, SamplingParams(max_new_tokens, temperature, top_p, top_k, tuple(stop_ids), seed,
                                              presence_penalty, frequency_penalty, repetition_penalty,
                                              dict(logit_bias) if logit_bias else None, logprobs),
                            adapters[i] if adapters is not None else None)
                for i, p in enumerate(prompts)]
        if self._thread is not None:
            for r in reqs:
                r.done.wait()
        else:
            while not all(r.done.is_set() for r in reqs):
                self.step()
        return reqs if return_requests else [r.output for r in reqs]

    # ------------------------------------------------------------------ background loop (server)
    def start(self):
        if self._thread is not None:
            return
        self._stop = False

        def loop():
            if self.device.type == "cuda":
                torch.cuda.set_device(self.device)
            sync = getattr(self, "tp_sync", False)
            while True:  # leaves only through the stop branch, which always tells the followers
                with self._cv:
                    while (not self._stop and not self.waiting and not self.active and not self.prefilling
                           and not self._tasks):
                        self._cv.wait(timeout=0.5)
                        if sync:  # idle heartbeat: followers wait inside a broadcast
                            break
                if self._tasks:
                    self._run_tasks()
                if self._stop:
                    if sync:
                        self._sync_admit([], stopping=True)  # tells the followers to stop
                    break
                try:
                    self.step()
                except Exception:  # noqa: BLE001
                    log.exception("engine step failed")
                    for r in list(self.active.values()):
                        r.error = "engine failure"
                        self._finish(r, "error")

        self._thread = threading.Thread(target=loop, name="mxllm-engine", daemon=True)
        self._thread.start()

    def stop(self):
        self._stop = True
        with self._cv:
            self._cv.notify_all()
        if self._thread is not None:
            self._thread.join(timeout=10)
        self._thread = None


@torch.no_grad()
def merge_lora_(model) -> None:
    """Fold LoRA adapters into the base weights (W += s * B @ A) for serving."""
    for mod in model.modules():
        if getattr(mod, "lora_r", 0) > 0:
            delta = mod.scaling * (mod.lora_b.float() @ mod.lora_a.float())
            mod.weight += delta.to(mod.weight.dtype)
            mod.lora_r = 0
            del mod.lora_a
            del mod.lora_b
            if hasattr(mod, "wbt"):
                del mod.wbt
            if hasattr(mod, "wxt"):
                del mod.wxt
