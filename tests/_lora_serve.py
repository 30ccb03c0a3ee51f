"""Inputs, references and bounds of the multi-adapter LoRA serving tests (tests/test_lora_serve.py on
the CPU, tests/test_lora_serve_gpu.py on the GPU).

Inputs are built on the CPU from fixed seeds: x Gaussian bf16, A Gaussian / sqrt(K), B Gaussian /
sqrt(r), y0 Gaussian, s = 2 -- the delta is about twice the base, so a dropped delta cannot hide.
Adapter 1 has rank r_max / 2 (zero-padded); ``ids`` mix -1, 0 and the last adapter.

Bounds (``tests/_parity.py``'s rule; none comes from a kernel): the fp32 PyTorch model of the
documented algorithm (mxllm/ops/lora_serve.py: 512-column fp32 partials added in ascending order,
then s * t B^T added to f32(y)) is compared with fp64 at these inputs,
    abs = max |y32 - ref| / row-max |ref|        rel = max |bf16(y32) - y32| / |y32|
over every shape and M below; the bound is twice each, c_rel at least one bf16 ulp.
``python -m tests.test_lora_serve_gpu`` prints the measurements again (no GPU needed) and asserts
they stay within the recorded ones.  The prefill path (library GEMMs, t rounded to bf16 between
them: that rounding gives its abs term) gets its own pair, obtained the same way.
"""
from __future__ import annotations

import math

import torch

from tests._parity import ULP_BF16

# (K, splits, r_max): the smallest shapes at which each mechanism can go wrong
SHAPES = [
    (256, [256, 64, 64], 16),   # one K chunk, three splits
    (1088, [512], 8),           # K is not a multiple of the 512-column chunk
    (8192, [1024, 1024], 64),   # the largest rank
    (28672, [512], 16),         # the most K chunks (the 70B down projection)
    (11264, [64, 64, 64], 64),  # the widest t (192) over 22 K chunks: the expand kernel's LDS staging
                                # takes five tiles, the last one ragged (8192 above: two full tiles)
]
MAX_M = 64  # the largest decode batch bucket the serving benchmark uses
MS = (1, 5, MAX_M)
N_ADAPTERS = 3

LORA_DELTA_Y_MEASURED = (0.00389, 4.62e-07)
LORA_DELTA_Y = (ULP_BF16, 9.24e-07)  # 2 x 0.00389 < one ulp; 2 x 4.62e-07
LORA_PREFILL_Y_MEASURED = (0.00381, 0.0019)  # at prefill_case()
LORA_PREFILL_Y = (ULP_BF16, 0.0038)  # 2 x 0.00381 < one ulp; 2 x 0.0019

# The serving engine's logits against an fp64 forward of the same model, |diff| / row-max |ref|, on
# tiny-d128 at the prompts of test_engine_teacher_forced (tests/test_lora_serve_gpu.py).  MEASURED is
# the BASE engine (no adapter registered: the code path from before adapters existed), the larger of
# graphs on / off, per KV cache format; the adapter rows get twice that, because the adapter step
# rounds each projection output once more (the delta is added to the bf16 projection output).
ENGINE_LOGITS_MEASURED = {"bf16": 0.00866, "fp8": 0.0254}  # graphs on and off gave the same figures


def engine_logits_bound(kv: str):
    return (0.0, 2.0 * ENGINE_LOGITS_MEASURED[kv])


def ids_for(M: int, all_none: bool = False) -> torch.Tensor:
    if all_none:
        return torch.full((M,), -1, dtype=torch.int32)
    pat = [0, -1, N_ADAPTERS - 1, 1, N_ADAPTERS - 1, 0, -1]
    if M == 1:
        pat = [N_ADAPTERS - 1]
    return torch.tensor([pat[i % len(pat)] for i in range(M)], dtype=torch.int32)


def make_case(K: int, splits, r_max: int, M: int, *, kind: str = "gauss", seed: int = 0, all_none: bool = False):
    """CPU tensors of one case: x [M, K], a [n, R, K], b [n, N, r_max] bf16, s [n] f32, y0 [M, N] bf16,
    ids int32 [M].  ``kind`` "int": small integers (|x| <= 2, |A| <= 1, |B| <= 2, |y0| <= 8, s = 0.5),
    for which all fp32 arithmetic is exact."""
    g = torch.Generator().manual_seed(1000 * seed + K + 7 * r_max + len(splits))
    N, ns = sum(splits), len(splits)
    R = ns * r_max
    if kind == "int":
        ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).to(torch.bfloat16)
        x, a, b, y0 = ri(-2, 2, MAX_M, K), ri(-1, 1, N_ADAPTERS, R, K), ri(-2, 2, N_ADAPTERS, N, r_max), ri(-8, 8, MAX_M, N)
        s = torch.full((N_ADAPTERS,), 0.5)
    else:
        rn = lambda *shape: torch.randn(*shape, generator=g)
        x = rn(MAX_M, K).to(torch.bfloat16)
        a = (rn(N_ADAPTERS, R, K) / math.sqrt(K)).to(torch.bfloat16)
        b = (rn(N_ADAPTERS, N, r_max) / math.sqrt(r_max)).to(torch.bfloat16)
        y0 = rn(MAX_M, N).to(torch.bfloat16)
        s = torch.full((N_ADAPTERS,), 2.0)
    # adapter 1: rank r_max / 2, zero-padded
    h = r_max // 2
    for i in range(ns):
        a[1, i * r_max + h:(i + 1) * r_max] = 0
    b[1, :, h:] = 0
    # rows are a prefix of one fixed [MAX_M, .] draw: row b is the same data whatever M is
    return {"K": K, "splits": list(splits), "r_max": r_max, "M": M, "x": x[:M].contiguous(), "a": a, "b": b, "s": s,
            "y0": y0[:M].contiguous(), "ids": ids_for(M, all_none)}


def tables_of(case, device="cpu", max_rows: int = MAX_M):
    """``ProjTables`` holding the case's adapters."""
    from mxllm.ops.lora_serve import make_proj_tables

    t = make_proj_tables(N_ADAPTERS, case["K"], case["splits"], case["r_max"], device, max_rows)
    t.a.copy_(case["a"])
    t.b.copy_(case["b"])
    t.s.copy_(case["s"])
    t.scales[:] = case["s"].tolist()
    return t


def _by_formula(case, dt, chunk: int | None, round_t: bool = False):
    """y (unrounded, dtype ``dt``) by the documented formula; ``chunk``: the width of the K partials
    (None: one sum); ``round_t``: t rounded to bf16 (the prefill path's GEMM output)."""
    x, y = case["x"].to(dt), case["y0"].to(dt).clone()
    K, r = case["K"], case["r_max"]
    stats = {"t": 0.0, "acc": 0.0}
    for aid in range(N_ADAPTERS):
        rows = (case["ids"] == aid).nonzero().flatten()
        if rows.numel() == 0:
            continue
        A, B, s = case["a"][aid].to(dt), case["b"][aid].to(dt), case["s"][aid].to(dt)
        xr = x[rows]
        if chunk is None:
            t = xr @ A.t()
        else:
            t = None
            for c in range(0, K, chunk):
                p = xr[:, c:c + chunk] @ A[:, c:c + chunk].t()
                t = p if t is None else t + p
        if round_t:
            t = t.to(torch.bfloat16).to(dt)
        stats["t"] = max(stats["t"], float(t.abs().max()))
        off = 0
        for i, n in enumerate(case["splits"]):
            acc = t[:, i * r:(i + 1) * r] @ B[off:off + n].t()
            stats["acc"] = max(stats["acc"], float(acc.abs().max()))
            y[rows, off:off + n] = y[rows, off:off + n] + s * acc
            off += n
    return y, stats


def ref_fp64(case) -> torch.Tensor:
    return _by_formula(case, torch.float64, None)[0]


def model_fp32(case) -> torch.Tensor:
    """The fp32 model of the decode kernels, before the rounding to bf16."""
    return _by_formula(case, torch.float32, 512)[0]


def prefill_model_fp32(case) -> torch.Tensor:
    """The fp32 model of the prefill path: t = bf16(x A_i^T), y = y0 + s (t B_i^T)."""
    return _by_formula(case, torch.float32, None, round_t=True)[0]


def segments_of(ids: torch.Tensor):
    from mxllm.ops.lora_serve import merge_segments

    return merge_segments(ids.tolist())


def prefill_case(seed: int = 0):
    """Three runs of tokens: adapter 0 (5 tokens), none (3), adapter 1 (a run of length 1)."""
    K, splits, r_max = SHAPES[0]
    c = make_case(K, splits, r_max, 9, seed=seed)
    c["ids"] = torch.tensor([0] * 5 + [-1] * 3 + [1], dtype=torch.int32)
    return c


def measure(model, cases) -> tuple[float, float]:
    """(rel, abs) of ``model`` over ``cases`` by the rule of the module docstring."""
    rel = ab = 0.0
    tiny = torch.finfo(torch.bfloat16).tiny
    for c in cases:
        ref, y32 = ref_fp64(c), model(c)
        live = c["ids"] >= 0
        if not bool(live.any()):
            continue
        ref, y32 = ref[live], y32[live].double()
        ab = max(ab, float(((y32 - ref).abs() / ref.abs().amax(-1, keepdim=True)).max()))
        yb = y32.float().to(torch.bfloat16).double()
        ok = yb.abs() >= tiny
        rel = max(rel, float(((yb - y32).abs() / y32.abs())[ok].max()))
    return rel, ab


def decode_cases(kind: str = "gauss"):
    return [make_case(K, sp, r, M, kind=kind) for K, sp, r in SHAPES for M in MS]


# ---------------------------------------------------------------------------- engine references
def random_adapter(cfg, r: int, seed: int, alpha: float | None = None, projections=None, b_std: float = 0.05):
    """A random adapter in ``load_adapter``'s format over ``projections`` (default: all seven), B != 0."""
    from mxllm.models.adapter import PROJECTIONS, proj_shape

    g = torch.Generator().manual_seed(seed)
    alpha = float(2 * r if alpha is None else alpha)
    w = {}
    for i in range(cfg.n_layers):
        for p in (projections or PROJECTIONS):
            n_out, n_in = proj_shape(cfg, p)
            A = ((torch.rand(r, n_in, generator=g) * 2 - 1) / math.sqrt(n_in)).to(torch.bfloat16)
            B = (torch.randn(n_out, r, generator=g) * b_std).to(torch.bfloat16)
            w[(i, p)] = (A, B)
    return {"r": r, "alpha": alpha, "scaling": alpha / r, "weights": w}


def dense_weight(lin) -> torch.Tensor:
    """fp64 weight of a FusedLinear (base weight alone) or a W8Linear (the decoded codes)."""
    if hasattr(lin, "q"):
        from mxllm.serve.quant import dequantize_e4m3

        return dequantize_e4m3(lin.q.cpu(), lin.scale.cpu()).double()
    return lin.weight.detach().cpu().double()


@torch.no_grad()
def forward_fp64(model, tokens, adapter=None) -> torch.Tensor:
    """Logits [S, V] (fp64, CPU) of ``model`` over one sequence, the adapter applied unmerged:
    every projection y = x W^T + s (x A^T) B^T on its own rows."""
    from mxllm.models.adapter import PROJECTIONS

    c = model.cfg
    S, D, Hq, Hkv = len(tokens), c.head_dim, c.n_heads, c.n_kv_heads
    cos, sin = model.rope_cos[:S].cpu().double(), model.rope_sin[:S].cpu().double()

    def proj(i, lin, name, x):
        y = x @ dense_weight(lin).t()
        if adapter is not None:
            off = 0
            for p, (_, lname, si) in PROJECTIONS.items():
                if lname != name:
                    continue
                n = lin.splits[si] if hasattr(lin, "splits") else {"wqkv": [c.q_dim, c.kv_dim, c.kv_dim], "wo": [c.hidden],
                                                                "wgu": [c.ffn, c.ffn], "wd": [c.hidden]}[name][si]
                w = adapter["weights"].get((i, p))
                if w is not None:
                    y[:, off:off + n] += adapter["scaling"] * ((x @ w[0].double().t()) @ w[1].double().t())
                off += n
        return y

    def norm(x, w):
        return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + c.norm_eps) * w.detach().cpu().double()

    def rope(t):  # [S, H, D], rotate-half
        t1, t2 = t[..., :D // 2], t[..., D // 2:]
        cc, ss = cos[:, None, :], sin[:, None, :]
        return torch.cat([t1 * cc - t2 * ss, t2 * cc + t1 * ss], -1)

    h = model.tok_emb.detach().cpu().double()[torch.tensor(tokens)]
    mask = torch.ones(S, S, dtype=torch.bool).tril()
    for i, layer in enumerate(model.layers):
        qkv = proj(i, layer.wqkv, "wqkv", norm(h, layer.attn_norm))
        q = rope(qkv[:, :c.q_dim].view(S, Hq, D))
        k = rope(qkv[:, c.q_dim:c.q_dim + c.kv_dim].view(S, Hkv, D)).repeat_interleave(Hq // Hkv, 1)
        v = qkv[:, c.q_dim + c.kv_dim:].view(S, Hkv, D).repeat_interleave(Hq // Hkv, 1)
        sc = torch.einsum("shd,thd->hst", q, k) / math.sqrt(D)
        p = torch.softmax(sc.masked_fill(~mask, float("-inf")), -1)
        o = torch.einsum("hst,thd->shd", p, v).reshape(S, Hq * D)
        h = h + proj(i, layer.wo, "wo", o)
        gu = proj(i, layer.wgu, "wgu", norm(h, layer.mlp_norm))
        mid = torch.nn.functional.silu(gu[:, :c.ffn]) * gu[:, c.ffn:]
        h = h + proj(i, layer.wd, "wd", mid)
    return norm(h, model.final_norm) @ model.head_weight.detach().cpu().double().t()
