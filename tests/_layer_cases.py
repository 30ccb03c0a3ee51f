"""Cases, references and checks of the strict transformer-layer tests (tests/test_layer_strict_gpu.py on the
GPU, tests/test_layer_cases.py on the CPU).  Everything here is built on the CPU from fixed seeds.

Unit under test: one call of the model's own layer, fed by the op that feeds it in training,

    x, h   = ops.add_rms_norm(d_prev, h_prev, layer.attn_norm, eps, out_pad=model._pad(layer.wqkv))
    x2, h2 = model._layer(i, x, h, B, S)
    loss   = (x2 * gx).sum() + (h2 * gh).sum()          (the last layer: gx alone, h2 unused)

of a two-layer model, for both layers.  Compared per element (tests/_parity.py): x2, h2, the rotated q and k as
they reach the attention kernel (RoPE is relative: positions that run on across the batch rows, the same for q
and k, change no other output of the layer -- tests/test_layer_cases.py shows it), the gradient of d_prev and
of every parameter that requires one (full fine-tune: attn_norm, wqkv, wo, mlp_norm, wgu, wd and the next norm;
LoRA: the A and B of the four projections, B's off-diagonal blocks exactly zero).

Inputs (``layer_weights`` / ``layer_io``), all bf16: h_prev, d_prev, gx, gh ~ N(0, 1); projection weights
~ N(0, 1 / K), so q, k, v and gu are O(1) and the softmax is neither uniform nor one-hot; every norm weight
~ U(0.5, 1.5); LoRA A ~ N(0, 1 / K) and the diagonal blocks of B ~ N(0, 1 / 4r) with s = 2: every adapter term
has the rms of its base term (tests/test_layer_cases.py asserts it), so a wrong adapter product cannot hide,
and q, k stay at rms 1.4 (with the twice larger B of tests/_lora_cases.py the scores have five times the
variance, the softmax is nearly one-hot and the layer amplifies its own roundings ten times).
The model's own init (std 0.02, gamma = 1) hides a wrong gamma, RoPE, mask or softmax.

References (``layer_math`` is the one formula, evaluated twice):
  * ``layer_ref64``: the exact function of the bf16 inputs in fp64 -- RMSNorm, projection, rotate-half RoPE from
    ``ref.rope_tables``, causal GQA softmax attention, SwiGLU, residual adds -- and its true gradients (autograd
    of the fp64 expression); no intermediate is rounded.
  * ``layer_model32``: the same in fp32 with every tensor that the ops store between kernels rounded to bf16
    where they round it.  Forward: h = d_prev + h_prev and every later residual (rmsnorm.hip rounds the sum and
    normalises the rounded value), the normed x, qkv (the GEMM output, rounded before the RoPE in the fused
    epilogue too), the rotated q and k, o, a = o Wo^T, gu, m, d = m Wd^T, the LoRA tails t = s x A^T.  Backward:
    do (the dX of the o projection), d(qkv) (once, after the inverse RoPE of the fp32 dQ / dK / dV), dx of the
    qkv GEMM, the dx of each add_rms_norm (norm term + residual gradient, one rounding), da, dx of the gate-up
    GEMM, dgu, dm (rounded before the SwiGLU backward in the fused epilogue as well), dd, the LoRA g = s dy B.
    Inside the attention (attn_fwd.hip / attn_bwd.hip, as tests/test_attention_strict_gpu.py models them): the
    exp2 domain with one fp32 factor, P~ rounded to bf16 before P~ V, the backward from the rounded O and the
    fp32 lse with P and dS rounded to bf16 before their products.  The outputs themselves (x2, h2, every
    gradient) are returned before their own rounding, as tests/_parity.py measures.
  * ``measure()`` (``python -m tests.test_layer_strict_gpu``, no GPU) prints the (rel, abs) of the model against
    the reference per output: the ``LAYER_*_MEASURED`` constants of tests/_parity.py.

Scale: every output against its row's maximum (a 1-D d-gamma: the vector's).  None of them cancels as a whole
at these inputs: the gradient of d_prev carries the O(1) residual gradient, and a d-gamma is a sum of T terms
of random sign whose rounding errors add up the same way (the measured abs terms are those of the bf16
intermediates, a few 1e-3 of the row maximum).

Gradient targets (``TARGETS``), attached the way FlatParams.attach_grads / the trainer attach them:
``autograd`` (.grad None), ``attached`` (.grad preset to g0: g0 + dW), ``fresh`` (.grad NaN, flagged
``_mx_grad_fresh``: overwritten, flag cleared), ``fp32x2`` (``_mx_grad32`` preset to g0, two micro-batches
accumulate).  g0 is Gaussian with the rms of the gradient it is added to.  ``check_ready`` holds the
gradient-ready notifications of every backward to what their owners rely on.

Routes (``ROUTES``): the switches of mxllm/models/llama.py and mxllm/ops that select one of the three q/k/v and
five MLP routes of ``Llama._layer``; ``apply_route`` sets them and installs the spies, ``check_route_ran`` holds
the spies' record to what the route must have run.  The last section chains the same formula into the whole
two-layer model (embedding, first norm, fused head + cross-entropy) for ``check_whole_model``; ``model_math`` takes
the parameter values and the batch as arguments (``model_params`` / ``model_inputs`` give those of the tests; with
``lora`` the LoRA layers chained the same way, the adapters alone trainable), which is what the reference of a
training step (tests/_step_cases.py) evaluates at the parameters a trainer holds.
"""
from __future__ import annotations

import functools
import importlib
import math
from collections import namedtuple

import torch
import torch.nn.functional as F_

from tests import _lora_cases as LC
from tests import _parity as P
from tests._parity import assert_exact, assert_parity

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
LOG2E = 1.4426950408889634
S_LORA = LC.S_LORA

LayerCase = namedtuple("LayerCase", "preset B S lora")
FULL_256 = LayerCase("tiny-d128", 2, 256, 0)   # the smallest shape every fused route takes: 2 batch rows, 2 M tiles
FULL_192 = LayerCase("tiny-d128", 2, 192, 0)   # T = 384: no gemm8 route, attention_block, standalone SwiGLU
TINY_192 = LayerCase("tiny", 2, 192, 0)        # head dim 32
LORA_256 = LayerCase("tiny-d128", 2, 256, 16)
FULL_CASES = (FULL_256, FULL_192, TINY_192)
CASES = FULL_CASES + (LORA_256,)
TARGETS = ("autograd", "attached", "fresh", "fp32x2")
PROJS = ("wqkv", "wo", "wgu", "wd")
FWD_KEYS = ("x2", "h2", "q", "k")  # q, k: the rotated [B, heads, S, D] that reach the attention kernel
FULL_GRADS = ("dg_attn", "dw_qkv", "dw_o", "dg_mlp", "dw_gu", "dw_d", "dg_next")
LORA_GRADS = tuple(f"d{ab}_{p[1:]}" for p in PROJS for ab in "ab")


def case_id(c):
    return f"{c.preset}-{c.B}x{c.S}" + (f"-lora{c.lora}" if c.lora else "")


def config(c):
    from mxllm.models import get_config

    return get_config(c.preset).replace(n_layers=2)


def grad_keys(c):
    return LORA_GRADS if c.lora else FULL_GRADS


def proj_splits(cfg, name):
    return {"wqkv": (cfg.q_dim, cfg.kv_dim, cfg.kv_dim), "wo": (cfg.hidden,), "wgu": (cfg.ffn, cfg.ffn),
            "wd": (cfg.hidden,)}[name]


def proj_in(cfg, name):
    return {"wqkv": cfg.hidden, "wo": cfg.q_dim, "wgu": cfg.hidden, "wd": cfg.ffn}[name]


# =========================================================================== inputs
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _seed(c):
    return 11000 + 7 * c.S + 3 * c.lora + (0 if c.preset == "tiny" else 1000)


@functools.lru_cache(maxsize=None)
def layer_weights(c):
    """[layer 0, layer 1, final_norm]: per layer attn_norm, mlp_norm ~ U(0.5, 1.5), wqkv / wo / wgu / wd
    ~ N(0, 1 / K) and, LoRA, ``<proj>_a`` ~ N(0, 1 / K), ``<proj>_b`` block-diagonal ~ N(0, 1 / 4r).  bf16."""
    cfg, g = config(c), _gen(_seed(c))
    gamma = lambda: (0.5 + torch.rand(cfg.hidden, generator=g)).to(BF16)  # noqa: E731
    out = []
    for _ in range(2):
        w = {"attn_norm": gamma(), "mlp_norm": gamma()}
        for name in PROJS:
            K, splits = proj_in(cfg, name), proj_splits(cfg, name)
            w[name] = (torch.randn(sum(splits), K, generator=g) * K ** -0.5).to(BF16)
            if c.lora:
                a, b = LC._adapters(g, K, splits, c.lora)
                w[name + "_a"], w[name + "_b"] = a, (0.5 * b.float()).to(BF16)  # (exact: a power of two)
        out.append(w)
    out.append(gamma())
    return out


@functools.lru_cache(maxsize=None)
def layer_io(c, i):
    """h_prev, d_prev and two micro-batches of upstream gradients (gx, gh), (gx2, gh2) ~ N(0, 1), bf16 [T, H]."""
    cfg, g = config(c), _gen(_seed(c) + 101 + i)
    return {k: torch.randn(c.B * c.S, cfg.hidden, generator=g).to(BF16) for k in ("h", "d", "gx", "gh", "gx2", "gh2")}


def rope_tables(c):
    """The model's own tables (fp32 values), the first B S positions (a defect may run on past S)."""
    from mxllm.ops import reference as ref

    cfg = config(c)
    return ref.rope_tables(c.B * c.S, cfg.head_dim, cfg.rope_theta, cfg.rope_scaling)


# =========================================================================== the formula
class _Rnd(torch.autograd.Function):
    """A tensor stored in bf16 between two kernels: the value rounded on the way forward (``fwd``), its gradient
    on the way back (``bwd``)."""

    @staticmethod
    def forward(ctx, t, fwd, bwd):
        ctx.bwd = bwd
        return t.to(BF16).to(t.dtype) if fwd else t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        return (g.to(BF16).to(g.dtype) if ctx.bwd else g), None, None


def _scores(q, k, vis, scale):
    G = q.shape[1] // k.shape[1]
    s = q @ k.repeat_interleave(G, 1).transpose(-1, -2)
    return (s * torch.tensor(scale * LOG2E, dtype=q.dtype)).masked_fill(~vis, float("-inf"))


class _AttnModel(torch.autograd.Function):
    """The documented algorithm of attn_fwd.hip / attn_bwd.hip in the tensors' dtype: q [B, Hq, S, D],
    k, v [B, Hkv, S, D] -> O [B, Hq, S, D] before its rounding; the backward reads the rounded O."""

    @staticmethod
    def forward(ctx, q, k, v, vis, scale):
        G = q.shape[1] // k.shape[1]
        x = _scores(q, k, vis, scale)
        m = x.amax(-1, keepdim=True)
        p = torch.exp2(x - m)
        l = p.sum(-1, keepdim=True)
        o = (p.to(BF16).to(q.dtype) @ v.repeat_interleave(G, 1)) / l
        ctx.save_for_backward(q, k, v, o.to(BF16).to(q.dtype), m + torch.log2(l), vis)
        ctx.scale = scale
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse, vis = ctx.saved_tensors
        B, Hq, S, D = q.shape
        Hkv = k.shape[1]
        G, scale, dt = Hq // Hkv, ctx.scale, q.dtype
        p = torch.exp2(_scores(q, k, vis, scale) - lse).masked_fill(~vis, 0.0)
        dp = do @ v.repeat_interleave(G, 1).transpose(-1, -2)
        delta = (do * o).sum(-1, keepdim=True)
        ds = (p * (dp - delta)).to(BF16).to(dt)
        p = p.to(BF16).to(dt)
        dq = (ds @ k.repeat_interleave(G, 1)) * scale
        dk = (ds.transpose(-1, -2) @ q).view(B, Hkv, G, S, D).sum(2) * scale
        dv = (p.transpose(-1, -2) @ do).view(B, Hkv, G, S, D).sum(2)
        return dq, dk, dv, None, None


def _attn_exact(q, k, v, vis, scale):
    G = q.shape[1] // k.shape[1]
    s = (q @ k.repeat_interleave(G, 1).transpose(-1, -2)) * scale
    return torch.softmax(s.masked_fill(~vis, float("-inf")), -1) @ v.repeat_interleave(G, 1)


def _rms(h, w, eps):
    return h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + eps) * w


def _rope(t, cos, sin):
    """Rotate-half (pairs i, i + D / 2) of t [T, heads, D] at the angles cos / sin [T, 1, D / 2]."""
    a, b = t[..., :t.shape[-1] // 2], t[..., t.shape[-1] // 2:]
    return torch.cat([a * cos - b * sin, b * cos + a * sin], -1)


DEFECTS = ("rope-runs-on", "mask-off-by-one", "dw-qkv-from-h", "no-residual-grad", "dgamma-mlp-short",
           "dgu-tile-zero", "dwd-halves-swapped", "next-gamma-missing", "fresh-added", "fp32x2-overwritten")


def _layer_body(c, W, x, h0, dt, r, model, defect=None, keep=lambda name, t: t):
    """What ``Llama._layer`` computes from (x, h0) with the weights ``W`` (``next_norm`` included): x2 before its
    rounding, h2 before and after, the rotated q / k before theirs, and h1, gu for the planted defects."""
    cfg, T = config(c), c.B * c.S
    Hq, Hkv, D, Fn, eps = cfg.n_heads, cfg.n_kv_heads, cfg.head_dim, cfg.ffn, cfg.norm_eps

    def proj(name, x):
        y = x @ W[name].t()
        if c.lora:  # the stored tail t = s x A^T; its gradient, rounded and times s = 2, is g = s dy B
            y = y + r(S_LORA * (x @ W[name + "_a"].t())) @ W[name + "_b"].t()
        return y

    qkv = r(keep("qkv", proj("wqkv", x)))
    dev = x.device
    pos = (torch.arange(T) % c.S if defect != "rope-runs-on" else torch.arange(T)).to(dev)
    cos, sin = [t.to(dev)[pos].to(dt)[:, None, :] for t in rope_tables(c)]
    q3, k3, v3 = (qkv[:, :Hq * D].view(T, Hq, D), qkv[:, Hq * D:(Hq + Hkv) * D].view(T, Hkv, D),
                  qkv[:, (Hq + Hkv) * D:].view(T, Hkv, D))
    heads = lambda t: t.view(c.B, c.S, -1, D).transpose(1, 2)  # noqa: E731
    q_pre, k_pre = heads(_rope(q3, cos, sin)), heads(_rope(k3, cos, sin))
    qh, kh, vh = r(q_pre, bwd=False), r(k_pre, bwd=False), heads(v3)
    ii, jj = torch.arange(c.S, device=dev).view(-1, 1), torch.arange(c.S, device=dev).view(1, -1)
    vis = jj <= ii + (1 if defect == "mask-off-by-one" else 0)
    scale = 1.0 / math.sqrt(D)
    oh = _AttnModel.apply(qh, kh, vh, vis, scale) if model else _attn_exact(qh, kh, vh, vis, scale)
    o = r(oh.transpose(1, 2).reshape(T, Hq * D))
    a = r(proj("wo", o))
    h1 = r(a + (h0.detach() if defect == "no-residual-grad" else h0))
    x1 = r(keep("x1", _rms(h1, W["mlp_norm"], eps)))
    gu_pre = keep("gu", proj("wgu", x1))
    if defect == "dgu-tile-zero":  # the last 256-row tile of M (rows 256.. of T)
        gu_pre.register_hook(lambda g: torch.cat([g[:256], torch.zeros_like(g[256:])]))
    gu = r(gu_pre)
    m = r(F_.silu(gu[:, :Fn]) * gu[:, Fn:])
    d = r(keep("d", proj("wd", m)))
    h2_pre = d + h1
    h2 = r(h2_pre)
    x2 = _rms(h2, torch.ones_like(W["next_norm"]) if defect == "next-gamma-missing" else W["next_norm"], eps)
    if defect == "next-gamma-missing":
        x2 = x2 + 0.0 * W["next_norm"].sum()
    return {"x2": x2, "h2_pre": h2_pre, "h2": h2, "q": q_pre, "k": k_pre, "h1": h1, "gu": gu}


def layer_math(c, i, dt, model, mb=0, defect=None):
    """One layer of case ``c`` (index ``i``) in ``dt``: the exact function (``model`` False) or the model of
    the ops' stored tensors (module doc).  ``mb``: which micro-batch's upstream gradients.  ``defect``: one of
    DEFECTS planted (tests/test_layer_cases.py).  Returns {x2, h2, q, k, dd, <gradient keys>}, before the
    output rounding."""
    cfg, T, last = config(c), c.B * c.S, i == 1
    Fn, eps = cfg.ffn, cfg.norm_eps
    ws = layer_weights(c)
    W = {k: v.to(dt) for k, v in ws[i].items()}
    W["next_norm"] = (ws[2] if last else ws[1]["attn_norm"]).to(dt)
    io = {k: v.to(dt) for k, v in layer_io(c, i).items()}
    gx, gh = (io["gx"], io["gh"]) if mb == 0 else (io["gx2"], io["gh2"])
    leaves = {"dg_attn": W["attn_norm"], "dg_mlp": W["mlp_norm"], "dg_next": W["next_norm"]}
    if c.lora:
        leaves = {f"d{ab}_{p[1:]}": W[f"{p}_{ab}"] for p in PROJS for ab in "ab"}
    else:
        leaves.update({f"dw_{p[1:]}": W[p] for p in PROJS})
    leaves["dd"] = io["d"]
    for t in leaves.values():
        t.requires_grad_(True)

    def r(t, fwd=True, bwd=True):
        return _Rnd.apply(t, fwd, bwd) if model else t

    tap = {}

    def keep(name, t):
        t.retain_grad()
        tap[name] = t
        return t

    h0 = r(io["d"] + io["h"], bwd=False)  # (the gradient of d_prev is an output: returned before its rounding)
    x = r(_rms(h0, W["attn_norm"], eps))
    t = _layer_body(c, W, x, h0, dt, r, model, defect, keep)
    loss = (t["x2"] * gx).sum() if last else (t["x2"] * gx).sum() + (t["h2"] * gh).sum()
    loss.backward()
    out = {"x2": t["x2"].detach(), "h2": t["h2_pre"].detach(), "q": t["q"].detach(), "k": t["k"].detach()}
    out.update({k: v.grad for k, v in leaves.items()})
    for k in [k for k in out if k.startswith("db_")]:  # B is block-diagonal: the other blocks have no gradient
        out[k] = out[k] * LC.block_mask(proj_splits(cfg, "w" + k[3:]), c.lora)
    if defect == "dw-qkv-from-h":
        out["dw_qkv"] = tap["qkv"].grad.t() @ h0.detach()
    if defect == "dgamma-mlp-short":
        h1 = t["h1"].detach()
        out["dg_mlp"] = (tap["x1"].grad * h1 * torch.rsqrt(h1.pow(2).mean(-1, keepdim=True) + eps))[:T - 64].sum(0)
    if defect == "dwd-halves-swapped":
        g_ = t["gu"].detach()
        out["dw_d"] = tap["d"].grad.t() @ (F_.silu(g_[:, Fn:]) * g_[:, :Fn]).to(BF16).to(dt)
    return out


@functools.lru_cache(maxsize=None)
def layer_ref64(c, i, mb=0):
    return layer_math(c, i, F64, False, mb)


@functools.lru_cache(maxsize=None)
def layer_model32(c, i, mb=0, defect=None):
    return layer_math(c, i, F32, True, mb, defect)


@functools.lru_cache(maxsize=None)
def start_grads(c, i):
    """g0 per gradient key: Gaussian bf16 with the rms of the (fp64) gradient it is added to."""
    g, ref = _gen(_seed(c) + 301 + i), layer_ref64(c, i)
    return {k: (torch.randn(ref[k].shape, generator=g) * LC.rms(ref[k])).to(BF16) for k in grad_keys(c)}


def expected(c, i, target, outs_of=layer_ref64, defect=None):
    """What ``target`` leaves: {x2, h2, dd, gradients} from ``outs_of`` (fp64 reference or fp32 model), g0 and the
    second micro-batch added where the target accumulates them."""
    kw = {"defect": defect} if outs_of is layer_model32 and defect in DEFECTS[:8] else {}
    first = outs_of(c, i, 0, **kw)
    if target in ("autograd", "fresh"):
        out = dict(first)
        if defect == "fresh-added":
            out.update({k: first[k] + float("nan") for k in grad_keys(c)})
        return out
    g0 = start_grads(c, i)
    if target == "attached":
        return {k: (v + g0[k].to(v.dtype) if k in g0 else v) for k, v in first.items()}
    second = outs_of(c, i, 1, **kw)
    if defect == "fp32x2-overwritten":
        return dict(second)
    return {k: (g0[k].to(v.dtype) + first[k] + v if k in g0 else v) for k, v in second.items()}


# =========================================================================== bounds and the check
def bound_name(c, key, target):
    """The name of the output's constant in tests/_parity.py."""
    if c.lora:
        name = "LAYER_LORA_" + key.upper()
    else:
        name = "LAYER_" + key.upper()
    if target == "fp32x2" and key in grad_keys(c):
        name += "_F32"
    return name


def bound_of(c, key, target):
    name = bound_name(c, key, target)
    return getattr(P, name), name


def check_outputs(c, i, target, outs, name):
    """Every element of every output of one (case, layer, target) against fp64; ``outs``: {key: tensor} in the
    dtypes the implementation leaves (bf16; the fp32x2 gradients fp32), on any device."""
    cfg, ref = config(c), expected(c, i, target)
    want_keys = {"x2", "q", "k", "dd"} | set(grad_keys(c)) | (set() if i == 1 else {"h2"})
    assert set(outs) >= want_keys, (sorted(outs), sorted(want_keys))
    for key in sorted(want_keys):
        got = outs[key]
        dev = got.device
        f32 = target == "fp32x2" and key in grad_keys(c)
        assert got.dtype == (F32 if f32 else BF16), f"{name}: {key} is {got.dtype}"
        bound, bname = bound_of(c, key, target)
        if c.lora and key.startswith("db_"):
            proj_name = "w" + key[3:]
            splits = proj_splits(cfg, proj_name)
            for bi, (rows, cols) in enumerate(LC._blocks(splits, c.lora)):
                assert_parity(got[rows, cols], ref[key][rows, cols].to(dev), bound, scale="row",
                              name=f"{name}: {key} block {bi} ({bname})")
            off = ~LC.block_mask(splits, c.lora).to(dev)
            assert_exact(torch.where(off, got, torch.zeros_like(got)), torch.zeros_like(got),
                         f"{name}: {key} off-diagonal blocks")
        else:
            assert_parity(got, ref[key].to(dev), bound, scale="row", name=f"{name}: {key} ({bname})")


def round_outputs(c, target, outs):
    """A model's fp32 outputs in the dtypes an implementation leaves them."""
    return {k: (v.float() if target == "fp32x2" and k in grad_keys(c) else v.to(BF16)) for k, v in outs.items()}


# =========================================================================== the implementation under test
def build_model(c, dev, dtype=BF16):
    """The two-layer Llama of case ``c`` on ``dev`` holding ``layer_weights(c)``, in train() mode."""
    from mxllm.models import Llama

    m = Llama(config(c), device=dev, dtype=dtype, lora_r=c.lora, lora_alpha=S_LORA * c.lora if c.lora else 16.0,
              init=False)
    ws = layer_weights(c)
    with torch.no_grad():
        m.tok_emb.zero_()
        if m.lm_head is not None:
            m.lm_head.zero_()
        for layer, w in zip(m.layers, ws[:2]):
            layer.attn_norm.copy_(w["attn_norm"])
            layer.mlp_norm.copy_(w["mlp_norm"])
            for name in PROJS:
                lin = getattr(layer, name)
                lin.weight.copy_(w[name])
                if c.lora:
                    LC.set_adapters(lin, w[name + "_a"], w[name + "_b"])
        m.final_norm.copy_(ws[2])
        m.refresh_images_()
    if c.lora:
        assert all(getattr(layer, name).augmented() and getattr(layer, name).scaling == S_LORA
                   for layer in m.layers for name in PROJS)
    return m.train()


def layer_params(m, c, i):
    """{gradient key: Parameter} of layer ``i``."""
    layer = m.layers[i]
    if c.lora:
        return {f"d{ab}_{p[1:]}": getattr(getattr(layer, p), f"lora_{ab}") for p in PROJS for ab in "ab"}
    nxt = m.final_norm if i == 1 else m.layers[1].attn_norm
    return {"dg_attn": layer.attn_norm, "dw_qkv": layer.wqkv.weight, "dw_o": layer.wo.weight,
            "dg_mlp": layer.mlp_norm, "dw_gu": layer.wgu.weight, "dw_d": layer.wd.weight, "dg_next": nxt}


def attach_grads(params, target, g0, dev):
    """Gradient targets as their owners attach them (FlatParams.attach_grads and its fp32 fold hook, the trainer's
    fresh flag and guard) plus a recorder of gradient-ready notifications (what DDP registers: ``mark_ready``
    for the gradients ops write themselves, the post-accumulate hook for autograd's).  Returns the recorder."""
    from mxllm.parallel.flat import FlatParams
    from mxllm.train.trainer import _fresh_guard

    ready = []

    def marked(p, key):  # mark_ready: the op wrote the gradient itself -- what the owner would now send off
        tgt = p._mx_grad32 if p._mx_grad32 is not None else p.grad
        ready.append(("mark", key, None if tgt is None else tgt.clone()))

    for key, p in params.items():
        if target == "fp32x2":
            p.register_post_accumulate_grad_hook(functools.partial(FlatParams._fold_hook, None))
        if target == "fresh":
            p.register_hook(_fresh_guard(p))
        p.register_post_accumulate_grad_hook(lambda q, _k=key: ready.append(("acc", _k, None)))
        p._mx_on_grad_ready = functools.partial(marked, key=key)
    reset_grads(params, target, g0, dev)
    return ready


def check_ready(ready, params, target, dev, name):
    """One backward's notifications.  ``mark_ready`` exactly once for every parameter whose gradient an op wrote
    itself (any attached target: every projection weight, and on the GPU every norm weight; never without a
    target), at a moment when the buffer already held its final value; every other parameter through autograd's
    post-accumulate hook (which also fires for a None gradient: owners ignore a second notification).

    This is the contract as the ops implement it today, pinned by hand, not derived from them: which gradients
    are written directly is what ``param_weight_grad`` / ``accum_grad`` do with an attached target (the CPU
    norm has no op of its own: autograd delivers its d-gamma).  A route that moves a gradient from one way of
    delivery to the other has to change this list with it."""
    marks = [k for kind, k, _ in ready if kind == "mark"]
    assert len(set(marks)) == len(marks), f"{name}: mark_ready more than once: {sorted(marks)}"
    direct = set() if target == "autograd" else {k for k in params
                                                 if torch.device(dev).type == "cuda" or not k.startswith("dg_")}
    assert set(marks) == direct, f"{name}: mark_ready for {sorted(marks)}, gradients written directly {sorted(direct)}"
    assert {k for _, k, _ in ready} == set(params), f"{name}: notified {sorted({k for _, k, _ in ready})}"
    for kind, k, snap in ready:
        if kind == "mark":
            p = params[k]
            final = p._mx_grad32 if p._mx_grad32 is not None else p.grad
            assert snap is not None and torch.equal(snap, final), f"{name}: {k} changed after mark_ready"


def reset_grads(params, target, g0, dev):
    for key, p in params.items():
        p.grad, p._mx_grad32, p._mx_grad_fresh = None, None, False
        if target == "attached":
            p.grad = g0[key].to(dev).to(p.dtype).clone()
        elif target == "fresh":
            p.grad = torch.full_like(p, float("nan"))
            p._mx_grad_fresh = True
        elif target == "fp32x2":
            p._mx_grad32 = g0[key].to(dev).float().clone()


def run_layer(m, c, i, dev, mb=0):
    """One forward and backward of the unit under test: (x2, h2, the gradient of d_prev)."""
    from mxllm import ops

    cfg, layer = m.cfg, m.layers[i]
    dt = m.final_norm.dtype
    io = {k: v.to(dev).to(dt) for k, v in layer_io(c, i).items()}
    gx, gh = (io["gx"], io["gh"]) if mb == 0 else (io["gx2"], io["gh2"])
    d = io["d"].clone().requires_grad_(True)
    x, h = ops.add_rms_norm(d, io["h"], layer.attn_norm, cfg.norm_eps, out_pad=m._pad(layer.wqkv))
    x2, h2 = m._layer(i, x, h, c.B, c.S)
    loss = (x2 * gx).sum() if i == 1 else (x2 * gx).sum() + (h2 * gh).sum()
    loss.backward()
    return x2.detach(), h2.detach(), d.grad


def run_target(m, c, i, target, dev, ready, log):
    """Gradients reset to the target's start, the one or two micro-batches run: {key: tensor}; asserts the
    gradient-ready notifications of every backward and the target's own invariants.  q and k are what the spies
    of ``apply_route`` saw go into the attention."""
    params = layer_params(m, c, i)
    reset_grads(params, target, start_grads(c, i), dev)
    for mb in range(2 if target == "fp32x2" else 1):
        del ready[:], log[:]  # (both record one forward + backward: the last)
        x2, h2, dd = run_layer(m, c, i, dev, mb)
        check_ready(ready, params, target, dev, f"micro-batch {mb}")
    seen = [info for k, info in log if k == "attn_in"]
    assert seen, "no attention forward was seen"
    outs = {"x2": x2, "h2": h2, "dd": dd, "q": seen[-1][0].detach().clone(), "k": seen[-1][1].detach().clone()}
    for key, p in params.items():
        if target == "fp32x2":
            assert p.grad is None, f"{key}: .grad set beside the fp32 target"
            outs[key] = p._mx_grad32.clone()
        else:
            assert p.grad is not None and p.grad.dtype == p.dtype, key
            outs[key] = p.grad.clone()
        if target == "fresh":
            assert not p._mx_grad_fresh, f"{key}: still flagged fresh"
            assert not bool(torch.isnan(outs[key]).any()), f"{key}: NaN left in a fresh buffer"
    others = [n for n, p in m.named_parameters() if p.grad is not None and all(p is not q for q in params.values())]
    assert not others, f"gradients of parameters outside layer {i}: {others}"
    return outs


# --------------------------------------------------------------------------- routes
def _mod(name):
    return importlib.import_module(name)  # (mxllm.ops.linear is also a function's name)


_REC = [("mxllm.models.llama", "RECOMPUTE_SWIGLU", "1"), ("mxllm.models.llama", "RECOMPUTE_NORM", "auto")]
_REC_KEEP = [_REC[0], ("mxllm.models.llama", "RECOMPUTE_NORM", "0")]
_UNFUSED_MLP = [("mxllm.models.llama", "REC_FUSED", False)]
_EPI_OFF = [("mxllm.ops.fused", "_ON", False)]
# route -> (module attributes to set, environment variables to set)
ROUTES = {
    "default": ([], {}),
    "no-bwd-epilogue": ([("mxllm.ops.fused", "_BWD_ON", False)], {}),
    "unfused": (_EPI_OFF, {}),
    "rec": (_REC, {}),
    "rec-keep-x": (_REC_KEEP, {}),
    "rec-unfused-mlp": (_REC + _UNFUSED_MLP, {}),
    "rec-unfused": (_REC + _UNFUSED_MLP + _EPI_OFF, {}),
    "deterministic": ([], {"MXLLM_DETERMINISTIC": "1"}),
    "lora-default": ([], {"MXLLM_GEMM8": "all"}),
    "lora-unfused": ([("mxllm.ops.linear", "_LORA_QKV_ROPE", False), ("mxllm.ops.activation", "_FUSE_TAIL", False)],
                     {}),
}
_DEFAULTS = [("mxllm.ops.fused", "_ON", True), ("mxllm.ops.fused", "_BWD_ON", True),
             ("mxllm.models.llama", "RECOMPUTE_SWIGLU", "auto"), ("mxllm.models.llama", "RECOMPUTE_NORM", "auto"),
             ("mxllm.models.llama", "REC_FUSED", True), ("mxllm.ops.linear", "_LORA_QKV_ROPE", True),
             ("mxllm.ops.linear", "_LORA_KERNELS", True), ("mxllm.ops.activation", "_FUSE_TAIL", True)]
_ENV_OFF = ("MXLLM_DETERMINISTIC", "MXLLM_GEMM8", "MXLLM_REFERENCE_OPS", "MXLLM_ATTN_DQ_MODE", "MXLLM_ATTN_DQ_ROPE")


class _NativeSpy:
    """torch.ops.mxllm recording what the named launches answered."""

    def __init__(self, real, names, log):
        self._real, self._names, self._log = real, names, log

    def __getattr__(self, k):
        f = getattr(self._real, k)
        if k not in self._names:
            return f

        def call(*a, **kw):
            res = f(*a, **kw)
            self._log.append(("attn_in", (a[0], a[1])) if k == "attn_fwd" else (k, res))
            return res
        return call


def apply_route(mp, route, c, dev):
    """The route's switches (every other switch at its default, whatever the environment says) and the spies:
    returns the log, a list of (name, info) in call order."""
    for mod, attr, val in _DEFAULTS + ROUTES[route][0]:
        mp.setattr(_mod(mod), attr, val)
    for k in _ENV_OFF:
        mp.delenv(k, raising=False)
    for k, v in ROUTES[route][1].items():
        mp.setenv(k, v)
    gemm, fused, llama, lin = (_mod("mxllm.ops.gemm"), _mod("mxllm.ops.fused"), _mod("mxllm.models.llama"),
                               _mod("mxllm.ops.linear"))
    if route == "lora-default":  # the unfused forward GEMM of this shape on the tail-balanced launch
        cfg = config(c)
        gemm._table()
        mp.setitem(gemm._TAIL, ("tn", c.B * c.S, cfg.q_dim + 2 * cfg.kv_dim, cfg.hidden + 64, "bf16"), 512)
    log = []

    def spy(obj, name, info=lambda a, k: None):
        real = getattr(obj, name)

        def f(*a, **k):
            log.append((name, info(a, k)))
            return real(*a, **k)
        mp.setattr(obj, name, f)

    spy(fused, "qkv_attention", lambda a, k: k.get("norm") is not None)
    spy(fused, "gate_up_swiglu", lambda a, k: k.get("norm") is not None)
    spy(fused, "gate_up_swiglu_down", lambda a, k: (k.get("norm") is not None, bool(k.get("recompute_m"))))
    spy(fused, "_norm_input")
    spy(llama.ops, "attention_block", lambda a, k: (k.get("out_pad", 0), k.get("grad_pad", 0)))
    spy(llama.ops, "swiglu", lambda a, k: (k.get("tail_fwd") is not None, k.get("tail_bwd") is not None))
    spy(llama.ops, "normed_linear")
    spy(llama.ops, "swiglu_linear")
    spy(llama.ops, "lora_qkv_attention")
    spy(lin._LinearFn, "apply", lambda a, k: a[1])
    spy(gemm, "mm", lambda a, k: a[0])
    spy(lin, "transpose2d")
    if torch.device(dev).type == "cuda":  # q, k [B, heads, S, D] as the attention kernel gets them
        nat = _NativeSpy(fused.native(), ("gemm8_swiglu_bwd", "gemm8", "gemm8_tail", "attn_fwd"), log)
        for mod in (fused, gemm, lin, _mod("mxllm.ops.attention")):
            mp.setattr(mod, "native", lambda: nat)
    else:  # the reference attention's [B, S, heads, D]
        real = _mod("mxllm.ops.reference").attention

        def attention(q, k, *a, **kw):
            log.append(("attn_in", (q.transpose(1, 2), k.transpose(1, 2))))
            return real(q, k, *a, **kw)
        mp.setattr(_mod("mxllm.ops.reference"), "attention", attention)
    return log


def count(log, name, info=None):
    return sum(1 for n, i in log if n == name and (info is None or i == info))


def check_route_ran(route, c, log, m, i, dev):
    """The spies' record of ONE forward + backward of one layer against what the route must run."""
    layer, gpu = m.layers[i], torch.device(dev).type == "cuda"
    n = functools.partial(count, log)
    linear_ws = [w for k, w in log if k == "apply"]
    through_linear = lambda p: any(w is p for w in linear_ws)  # noqa: E731
    fused_routes = n("qkv_attention") + n("gate_up_swiglu") + n("gate_up_swiglu_down")
    takes_fused = gpu and c == FULL_256
    msg = f"{route}: {[(k, v) for k, v in log if k not in ('mm', 'apply', 'gemm8', 'transpose2d', 'attn_in')]}"
    if c.lora:
        if route == "lora-default" and gpu:
            assert n("lora_qkv_attention") == 1 and n("attention_block") == 0 and n("swiglu", (True, True)) == 1, msg
        else:
            assert n("lora_qkv_attention") == 0 and n("swiglu", (False, False)) == 1, msg
            assert n("attention_block", (64, 64)) == 1, msg  # out_pad / grad_pad of the LoRA neighbours
        return
    if not takes_fused or route in ("deterministic",):
        assert fused_routes == 0, msg
    if route in ("rec", "rec-keep-x", "rec-unfused-mlp", "rec-unfused"):
        rec_x = route != "rec-keep-x"
        if takes_fused and route in ("rec", "rec-keep-x"):
            assert n("qkv_attention", rec_x) == 1 and n("gate_up_swiglu_down", (rec_x, True)) == 1, msg
            assert n("_norm_input") == (2 if rec_x else 0) and n("normed_linear") == n("swiglu_linear") == 0, msg
            assert n("gemm8_swiglu_bwd", True) == 1, msg
        elif takes_fused and route == "rec-unfused-mlp":
            assert n("qkv_attention", True) == 1 and n("normed_linear") == 1 and n("swiglu_linear") == 1, msg
            assert n("_norm_input") == 1 and n("gate_up_swiglu_down") == n("gate_up_swiglu") == 0, msg
        else:  # rec-unfused, and every recompute route where no fused epilogue takes the shape
            assert n("normed_linear") == (2 if rec_x else 0) and n("attention_block") == 1, msg
            assert n("swiglu_linear") == 1 and fused_routes == 0 and n("swiglu") == 0, msg
        return
    if takes_fused and route == "default":
        assert n("qkv_attention", False) == 1 and n("gate_up_swiglu_down", (False, False)) == 1, msg
        assert n("gemm8_swiglu_bwd", True) == 1 and n("attention_block") == n("swiglu") == 0, msg
    elif takes_fused and route == "no-bwd-epilogue":
        assert n("qkv_attention", False) == 1 and n("gate_up_swiglu", False) == 1, msg
        assert n("gate_up_swiglu_down") == 0 and n("gemm8_swiglu_bwd") == 0 and through_linear(layer.wd.weight), msg
    else:  # unfused, deterministic, and the default switches at a shape no fused route takes
        assert fused_routes == 0 and n("attention_block", (0, 0)) == 1 and n("swiglu", (False, False)) == 1, msg
        assert all(through_linear(getattr(layer, p).weight) for p in PROJS), msg
    if route == "deterministic" and gpu:  # 4 forward, 4 dX and 4 dW GEMMs, each one gemm8 launch that was taken
        assert n("mm") == 12 and n("gemm8", True) + n("gemm8_tail", True) == 12 and n("transpose2d") == 0, msg
        assert n("gemm8", False) == 0, msg


def check_layer(c, route, target, dev, mp, i=0, dtype=BF16):
    """One case: the route's switches set through ``mp`` (pytest's monkeypatch), the layer run on ``dev`` into
    ``target``, the route's spies checked, every output against fp64 -- and all of it once more, bit for bit."""
    log = apply_route(mp, route, c, dev)
    name = f"{case_id(c)} {route} layer {i} {target}"
    m = build_model(c, dev, dtype)
    ready = attach_grads(layer_params(m, c, i), target, start_grads(c, i), dev)
    outs = run_target(m, c, i, target, dev, ready, log)
    check_route_ran(route, c, log, m, i, dev)
    if dtype != BF16:  # fp32 parameters (CPU recompute routes): the same values, compared in the bf16 / fp32 slots
        outs = round_outputs(c, target, outs)
    check_outputs(c, i, target, outs, name)
    again = run_target(m, c, i, target, dev, ready, log)
    if dtype != BF16:
        again = round_outputs(c, target, again)
    for key in outs:
        assert_exact(again[key], outs[key], f"{name}: {key}, second run")
    return outs


# =========================================================================== the whole model
# Two layers of tiny-d128 on ids [2, 256]: the loss and every parameter gradient against the fp64 model of the
# whole network.  This is what reaches ckpt.checkpoint around _layer, the plain rms_norm of the first layer, the
# embedding forward and backward (one id in a quarter of the positions), the tied embedding's two-use gradient
# and the fused head + cross-entropy (a tenth of the labels ignored) inside the model.
MODEL_CASE = FULL_256
IGNORE = -100
REPEATED_ID = 7
CKPT_SETTINGS = (False, True, 1)
MODEL_LAYER_KEYS = FULL_GRADS[:-1]  # per layer; the next norm is the next layer's attn_norm or final_norm


@functools.lru_cache(maxsize=None)
def model_inputs(tied):
    """ids, labels [2, 256] and the embedding / head weights: untied E ~ N(0, 1), head ~ N(0, 1 / H); tied
    E ~ N(0, 1 / H), so the logits are O(1) either way (the first norm rescales the embedding rows)."""
    c, cfg = MODEL_CASE, config(MODEL_CASE)
    g = _gen(_seed(c) + 501 + tied)
    V, H = cfg.vocab_size, cfg.hidden
    ids = torch.randint(0, V, (c.B, c.S), generator=g)
    ids[torch.rand(c.B, c.S, generator=g) < 0.25] = REPEATED_ID
    labels = torch.randint(0, V, (c.B, c.S), generator=g)
    labels[torch.rand(c.B, c.S, generator=g) < 0.1] = IGNORE
    emb = (torch.randn(V, H, generator=g) * (H ** -0.5 if tied else 1.0)).to(BF16)
    head = None if tied else (torch.randn(V, H, generator=g) * H ** -0.5).to(BF16)
    return ids, labels, emb, head


class _CEModel(torch.autograd.Function):
    """The fused head + cross-entropy as mxllm/ops/loss.py ``_LinearCEFn`` stores it: bf16 logits, the loss from
    them in the tensors' dtype, d(logits) = (softmax - onehot) / n_valid rounded to bf16 before the two GEMMs."""

    @staticmethod
    def forward(ctx, x, w, labels):
        lg = (x @ w.t()).to(BF16).to(x.dtype)
        valid = labels != IGNORE
        lab = labels.clamp(min=0)
        n = valid.sum()
        losses = torch.logsumexp(lg, -1) - lg.gather(1, lab[:, None]).squeeze(1)
        g = torch.softmax(lg, -1)
        g[torch.arange(g.shape[0]), lab] -= 1.0
        ctx.save_for_backward(x, w, (g * valid[:, None] / n).to(BF16).to(x.dtype))  # (n > 0: model_math)
        return (losses * valid).sum() / n

    @staticmethod
    def backward(ctx, gl):
        x, w, g = ctx.saved_tensors
        return (g @ w) * gl, (g.t() @ x) * gl, None


def model_params(tied, lora=0):
    """{name: bf16 value} of the whole model of the tests, named as ``Llama.named_parameters`` names them:
    ``layer_weights`` of the full case (``lora``: of LORA_256, adapters included) and the embedding / head of
    ``model_inputs``."""
    c = LORA_256 if lora else MODEL_CASE
    assert lora in (0, LORA_256.lora)
    _, _, emb, head = model_inputs(tied)
    ws = layer_weights(c)
    out = {"tok_emb": emb}
    for i in (0, 1):
        out[f"layers.{i}.attn_norm"], out[f"layers.{i}.mlp_norm"] = ws[i]["attn_norm"], ws[i]["mlp_norm"]
        for p in PROJS:
            out[f"layers.{i}.{p}.weight"] = ws[i][p]
            if lora:
                out[f"layers.{i}.{p}.lora_a"], out[f"layers.{i}.{p}.lora_b"] = ws[i][p + "_a"], ws[i][p + "_b"]
    out["final_norm"] = ws[2]
    if not tied:
        out["lm_head"] = head
    return out


def param_key(name):
    """The key of ``model_math``'s gradient of the parameter ``name``."""
    if name in ("tok_emb", "lm_head", "final_norm"):
        return {"tok_emb": "demb", "lm_head": "dhead", "final_norm": "dg_final"}[name]
    _, i, rest = name.split(".", 2)
    if rest in ("attn_norm", "mlp_norm"):
        return f"l{i}.dg_{rest[:-5]}"
    proj, leaf = rest.split(".")
    return f"l{i}.d{ {'weight': 'w', 'lora_a': 'a', 'lora_b': 'b'}[leaf]}_{proj[1:]}"


def trainable(name, lora):
    return name.endswith(("lora_a", "lora_b")) if lora else True


def model_math(tied, dt, model, defect=None, *, params, batch, lora=0, loss_scale=1.0):
    """The whole network in ``dt`` at the parameter values ``params`` ({name: tensor}, ``model_params`` names) on
    the batch ``batch`` = (ids, labels), on the parameters' device: {loss [1], losses, and the gradient of
    ``loss_scale`` x loss for every trainable parameter: demb, dhead (untied), l<i>.<key>, dg_final; ``lora``:
    l<i>.da_<proj> / l<i>.db_<proj> alone, the off-diagonal blocks of B without a gradient}, before the
    output rounding.  No valid label: loss 0, every gradient 0.  ``defect``: "tied-embedding-use-dropped",
    "ignored-labels-counted", "n-valid-plus-two", "ckpt-layer-dw-missing" / "ckpt-layer-dw-doubled" (the
    gradients of layer 0's parameters -- the layer every checkpoint setting wraps -- not written, or written
    by both of its forward runs) (tests/test_layer_cases.py)."""
    c = LORA_256 if lora else MODEL_CASE
    cfg = config(c)
    dev = params["tok_emb"].device
    ids, labels = [t.to(dev).reshape(-1) for t in batch]
    P_ = {k: v.detach().to(dt).requires_grad_(trainable(k, lora)) for k, v in params.items()}
    L = [{k.split(".", 2)[2].replace(".weight", "").replace(".lora_", "_"): v for k, v in P_.items()
          if k.startswith(f"layers.{i}.")} for i in (0, 1)]
    final, E = P_["final_norm"], P_["tok_emb"]
    Wh = E if tied else P_["lm_head"]

    def r(t, fwd=True, bwd=True):
        return _Rnd.apply(t, fwd, bwd) if model else t

    # tied: the embedding's fp32 row sums and the head's dW GEMM each round to bf16 before autograd adds them
    Eg = (E.detach() if defect == "tied-embedding-use-dropped" else r(E, fwd=False)) if tied else E
    h = r(Eg[ids], fwd=False)  # the norm's dx and the residual gradient, both bf16, added in bf16 by autograd
    x = r(_rms(r(h, fwd=False), L[0]["attn_norm"], cfg.norm_eps))
    for i in (0, 1):
        W = dict(L[i], next_norm=final if i == 1 else L[1]["attn_norm"])
        t = _layer_body(c, W, x, h, dt, r, model)
        x, h = r(t["x2"]), t["h2"]
    wh = r(Wh, fwd=False) if tied else Wh
    n_valid = int((labels != IGNORE).sum())
    if n_valid == 0:
        loss = (x @ wh.t()).sum() * 0.0
    elif model:
        loss = _CEModel.apply(x, wh, labels)
    else:
        loss = F_.cross_entropy(x @ wh.t(), labels, ignore_index=IGNORE)
    if defect == "ignored-labels-counted":
        loss = loss * float(n_valid) / labels.numel()
    if defect == "n-valid-plus-two":
        loss = loss * float(n_valid) / float(n_valid + 2)
    if loss.requires_grad:
        (loss * loss_scale).backward()
    with torch.no_grad():  # the per-token losses the mean is taken of: what MODEL_LOSS is measured on
        lg, valid = x @ wh.t(), labels != IGNORE
        lg = lg.to(BF16).to(dt) if model else lg
        losses = (torch.logsumexp(lg, -1) - lg.gather(1, labels.clamp(min=0)[:, None]).squeeze(1))[valid]
    out = {"loss": loss.detach().reshape(1), "losses": losses}
    for name, v in P_.items():
        if v.requires_grad:
            out[param_key(name)] = v.grad if v.grad is not None else torch.zeros_like(v)
    for k in [k for k in out if ".db_" in k]:  # B is block-diagonal: the other blocks have no gradient
        out[k] = out[k] * LC.block_mask(proj_splits(cfg, "w" + k.split("_")[1]), c.lora).to(dev)
    if defect in ("ckpt-layer-dw-missing", "ckpt-layer-dw-doubled"):
        f = 0.0 if defect.endswith("missing") else 2.0
        out.update({k: v * f for k, v in out.items() if k.startswith("l0.")})
    return out


@functools.lru_cache(maxsize=None)
def model_ref64(tied):
    return model_math(tied, F64, False, params=model_params(tied), batch=model_inputs(tied)[:2])


@functools.lru_cache(maxsize=None)
def model_model32(tied, defect=None):
    return model_math(tied, F32, True, defect, params=model_params(tied), batch=model_inputs(tied)[:2])


F32_OUTPUTS = ("MODEL_LOSS",)  # the constants whose output dtype is fp32 whatever the gradient target


def model_bound_name(tied, key):
    if key == "demb" and tied:
        return "MODEL_DEMB_TIED"
    return "MODEL_" + key.split(".")[-1].upper()


def round_model_outputs(outs):
    return {k: (v.float() if k == "loss" else v.to(BF16)) for k, v in outs.items() if k != "losses"}


def check_model_outputs(tied, outs, name):
    """The loss (fp32, [1], against its own value) and every parameter gradient (bf16, against its row's maximum)
    of the whole model against fp64.  MODEL_LOSS: ``measure_model`` says how a mean's bound is measured."""
    ref = {k: v for k, v in model_ref64(tied).items() if k != "losses"}
    assert set(outs) == set(ref), (sorted(outs), sorted(ref))
    for key in sorted(ref):
        got = outs[key]
        assert got.dtype == (F32 if key == "loss" else BF16), f"{name}: {key} is {got.dtype}"
        bname = model_bound_name(tied, key)
        assert_parity(got, ref[key].to(got.device), getattr(P, bname), scale="row", name=f"{name}: {key} ({bname})")


def build_whole_model(tied, ckpt, dev):
    from mxllm.models import Llama

    ids, labels, emb, head = model_inputs(tied)
    m = Llama(config(MODEL_CASE).replace(tie_embeddings=tied), device=dev, init=False, activation_checkpointing=ckpt)
    ws = layer_weights(MODEL_CASE)
    with torch.no_grad():
        m.tok_emb.copy_(emb)
        if not tied:
            m.lm_head.copy_(head)
        for layer, w in zip(m.layers, ws[:2]):
            layer.attn_norm.copy_(w["attn_norm"])
            layer.mlp_norm.copy_(w["mlp_norm"])
            for name in PROJS:
                getattr(layer, name).weight.copy_(w[name])
        m.final_norm.copy_(ws[2])
    return m.train()


def run_whole_model(m, tied, dev):
    ids, labels, _, _ = model_inputs(tied)
    m.zero_grad(set_to_none=True)
    loss = m(ids.to(dev), labels.to(dev), ignore_index=IGNORE)
    loss.backward()
    names = {"tok_emb": "demb", "lm_head": "dhead", "final_norm": "dg_final"}
    for i in (0, 1):
        names.update({f"layers.{i}.attn_norm": f"l{i}.dg_attn", f"layers.{i}.mlp_norm": f"l{i}.dg_mlp"})
        names.update({f"layers.{i}.{p}.weight": f"l{i}.dw_{p[1:]}" for p in PROJS})
    outs = {"loss": loss.detach().float().reshape(1)}
    outs.update({names[n]: p.grad.clone() for n, p in m.named_parameters()})
    return outs


def check_whole_model(tied, ckpt, dev, mp):
    """The model's own forward (embedding, first norm, both layers -- checkpointed as ``ckpt`` says --, fused head
    + CE) and backward on ``dev``; spies: how often ``ckpt.checkpoint`` wrapped a layer, which layers recompute
    (``ckpt`` an int: the un-checkpointed ones), one fused head + CE; every output against fp64; twice the same bits."""
    log = apply_route(mp, "default", MODEL_CASE, dev)
    llama = _mod("mxllm.models.llama")
    for obj, name in ((llama.ckpt, "checkpoint"), (llama.ops, "linear_cross_entropy"), (llama.ops, "embedding")):
        real = getattr(obj, name)
        mp.setattr(obj, name, lambda *a, _r=real, _n=name, **k: (log.append((_n, None)), _r(*a, **k))[1])
    name = f"model {'tied' if tied else 'untied'} ckpt={ckpt}"
    m = build_whole_model(tied, ckpt, dev)
    del log[:]
    outs = run_whole_model(m, tied, dev)
    n = functools.partial(count, log)
    assert n("checkpoint") == (2 if ckpt is True else int(ckpt)), (name, n("checkpoint"))
    assert n("linear_cross_entropy") == 1 and n("embedding") == 1, name
    rec = n("swiglu_linear") + n("gate_up_swiglu_down", (True, True))  # layers that rebuild x and m in the backward
    assert rec == (0 if isinstance(ckpt, bool) else 2 - ckpt), (name, rec)
    # every layer's forward once, a checkpointed layer's once more in the backward: on the GPU each through the
    # fused q/k/v and MLP routes (this shape takes them), on the CPU through attention_block
    fwds = 2 + (2 if ckpt is True else int(ckpt))
    if torch.device(dev).type == "cuda":
        assert n("qkv_attention") == n("gate_up_swiglu_down") == fwds and n("attention_block") == 0, (name, fwds)
    else:
        assert n("attention_block") == fwds and n("qkv_attention") == n("gate_up_swiglu_down") == 0, (name, fwds)
    check_model_outputs(tied, outs, name)
    again = run_whole_model(m, tied, dev)
    for key in outs:
        assert_exact(again[key], outs[key], f"{name}: {key}, second run")
    return outs


def measure_model():
    """The ``MODEL_*_MEASURED`` constants: the chained fp32 model against fp64, tied and untied.

    MODEL_LOSS: the loss is ONE number, the mean of n_valid per-token losses whose errors (the bf16 roundings of
    the logits and of everything before them) have either sign.  The error of one evaluation of the model is one
    draw of a sum of n terms: twice that draw is no bound for another summation order or another rounding of
    the same terms.  What the model does measure is the spread of that draw: the rms of the per-token errors
    / sqrt(n_valid), the standard error of the mean (the model's own two draws, untied and tied, lie at 0.7 and
    0.6 of it).  The measured abs term is three standard errors, relative to the loss; the bound doubles it
    like every other."""
    from tests.test_rowwise_strict_gpu import _meas

    acc = {}
    for tied in (False, True):
        mod, ref = model_model32(tied), model_ref64(tied)
        for key in sorted(ref):
            if key not in ("loss", "losses"):
                _meas(acc, model_bound_name(tied, key), mod[key], ref[key], BF16)
        e = mod["losses"].double() - ref["losses"]
        se = float(e.pow(2).mean().sqrt()) / e.numel() ** 0.5
        assert abs(float(mod["loss"].double() - ref["loss"])) < 3 * se  # the model's own draw lies within it
        acc["MODEL_LOSS"] = (0.0, max(acc.get("MODEL_LOSS", (0.0, 0.0))[1], 3 * se / float(ref["loss"])))
    return acc


# =========================================================================== the measurements
def measure():
    """The ``LAYER_*_MEASURED`` constants of tests/_parity.py: ``layer_model32`` against ``layer_ref64`` at the
    inputs of the tests, on the CPU, over both layers of every case and every target that changes the sum."""
    from tests.test_rowwise_strict_gpu import _meas

    acc = {}
    for c in CASES:
        for i in (0, 1):
            for target in (("autograd",) if c.lora else ("autograd", "attached", "fp32x2")):
                mod, ref = expected(c, i, target, layer_model32), expected(c, i, target)
                for key in sorted(mod):
                    if (key == "h2" and i == 1) or (target != "autograd" and key not in grad_keys(c)):
                        continue
                    f32 = target == "fp32x2"
                    name = bound_name(c, key, target)
                    if c.lora and key.startswith("db_"):
                        for rows, cols in LC._blocks(proj_splits(config(c), "w" + key[3:]), c.lora):
                            _meas(acc, name, mod[key][rows, cols], ref[key][rows, cols], BF16)
                    else:
                        _meas(acc, name, mod[key], ref[key], F32 if f32 else BF16)
    return acc
