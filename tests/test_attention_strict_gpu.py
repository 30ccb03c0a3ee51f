"""Per-element parity of the attention kernels (attn_fwd.hip, attn_bwd.hip) with fp64 references.

O, lse, dQ, dK and dV are compared element by element (``tests/_parity.py``) with the exact function
of the same bf16 inputs, computed in fp64: softmax(scale q k^T) v and its true gradients.  The
kernels' own intermediates (their bf16 O, their fp32 lse) are inputs of the backward as in training;
the reference uses none of them.  dK / dV partial heads are summed in fp64 before the comparison.

The cases sit on every tile edge of the kernels: the 64-row query tile, the 64-key forward tile, the
128-row forward block, the 128-key backward block and the 256-row dQ workgroup, each at one row / key
less, exactly and one more; one query row; a cached prefix (bottom-right causal); key tails; S > Sk;
GQA groups of 1, 2, 4 and 16.

The bounds come from no kernel.  ``measure()`` (``python -m tests.test_attention_strict_gpu``, no GPU
needed) runs a plain fp32 PyTorch model of the algorithm documented in the kernels' header comments
at exactly these inputs (built on the CPU from fixed seeds) and prints its error against fp64:

  forward   x = s * (scale log2 e), P~ = exp2(x - rowmax), l = sum P~ (fp32);
            O = (bf16 P~ . V) / l, rounded to bf16; lse = rowmax + log2 l
  backward  P = exp2(x - lse), delta = rowsum(dO * bf16 O), dS = P (dP - delta);
            dQ = scale bf16(dS) K, dK = scale bf16(dS)^T Q, dV = bf16(P)^T dO

O is bounded relative to its row and lse to the tensor's max |ref|.  The gradients cancel: dS = P (dP -
delta) is an exact zero for a query that sees one key (the first causal row; all of dQ and dK at S = Sk
= 1), where the kernel, whose delta comes from the rounded O, legitimately leaves a rounding residue.
Their absolute term is therefore relative to the magnitude of what is subtracted, the largest element
over the tensor of the same products taken with absolute values (``scales``):
    dQ: scale sum_j P (|dP| + |delta|) |K|    dK: scale sum_i P (|dP| + |delta|) |Q|    dV: sum_i P |dO|
"""
import functools
import math

import pytest
import torch

from tests import _parity as P
from tests._parity import assert_parity
from tests.test_rowwise_strict_gpu import _rope_merge, rope_tables

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
LOG2E = 1.4426950408889634

# (B, Hq, Hkv, S, Sk, D, causal)
ATTN_CASES = (
    [(2, 4, 2, 1, 1, 128, True), (1, 2, 1, 1, 200, 128, True)]  # one query row; with a cached prefix
    + [(2, 4, 1, s, s, d, True) for d in (32, 64, 128) for s in (63, 64, 65, 127, 128, 129)]
    + [(1, 8, 2, 257, 257, 128, True),  # 256-row dQ workgroup; G = 4
       (1, 4, 2, 129, 129, 64, True), (1, 4, 2, 65, 65, 32, True),  # dQ-kernel row blocks of the other D
       (2, 2, 2, 65, 200, 128, True),  # bottom-right causal, offset 135
       (1, 4, 2, 100, 300, 64, False), (1, 2, 1, 130, 70, 128, False),  # non-causal: key tail; S > Sk
       (1, 16, 1, 192, 192, 128, True)])  # G = 16
DS_BUDGET_CASE = (2, 8, 2, 257, 257, 128, True)


def case_id(c):
    B, Hq, Hkv, S, Sk, D, causal = c
    return f"B{B}-Hq{Hq}-Hkv{Hkv}-S{S}-Sk{Sk}-D{D}-{'causal' if causal else 'full'}"


ATTN_IDS = [case_id(c) for c in ATTN_CASES]
ROPE_CASES = [c for c in ATTN_CASES if c[3] == c[4] and c[5] == 128]
MODES = (1, 2, 3)


def _ops():
    from mxllm.ops import native

    return native()


@functools.lru_cache(maxsize=4)
def attn_inputs(case):
    """q [B,Hq,S,D], k / v [B,Hkv,Sk,D], dO [B,S,Hq*D], all bf16, N(0, 1), on the CPU."""
    B, Hq, Hkv, S, Sk, D, _ = case
    g = torch.Generator().manual_seed(9000 + 131 * S + 17 * Sk + D + Hq)
    q = torch.randn(B, Hq, S, D, generator=g).to(BF16)
    k = torch.randn(B, Hkv, Sk, D, generator=g).to(BF16)
    v = torch.randn(B, Hkv, Sk, D, generator=g).to(BF16)
    do = torch.randn(B, S, Hq * D, generator=g).to(BF16)
    return q, k, v, do


def _scores(q, k, causal, scale, dt):
    """x = s * scale * log2 e [B,Hq,S,Sk] in ``dt`` and the visibility mask (bottom-right causal)."""
    G = q.shape[1] // k.shape[1]
    S, Sk = q.shape[2], k.shape[2]
    s = q.to(dt) @ k.to(dt).repeat_interleave(G, 1).transpose(-1, -2)
    sl = torch.tensor(scale * LOG2E, dtype=dt)  # fp32 model: the kernel's one rounded factor
    vis = torch.ones(S, Sk, dtype=torch.bool, device=q.device)
    if causal:
        i = torch.arange(S, device=q.device).view(S, 1)
        j = torch.arange(Sk, device=q.device).view(1, Sk)
        vis = j <= i + (Sk - S)
    return s * sl.to(q.device), vis


def attn_fwd_model(q, k, v, causal, scale, dt, model):
    """O [B,Hq,S,D] before its output rounding and lse [B,Hq,S] (log2 domain), in ``dt``.
    ``model``: the kernel's documented roundings (bf16 P~ in the P~ V product); else the exact function."""
    G = q.shape[1] // k.shape[1]
    x, vis = _scores(q, k, causal, scale, dt)
    x = x.masked_fill(~vis, float("-inf"))
    m = x.amax(-1, keepdim=True)
    p = torch.exp2(x - m)
    l = p.sum(-1, keepdim=True)
    pv = (p.to(BF16).to(dt) if model else p) @ v.to(dt).repeat_interleave(G, 1)
    return pv / l, (m + torch.log2(l)).squeeze(-1)


def attn_bwd_model(do, q, k, v, o, lse, causal, scale, dt, model, scales=None):
    """dQ [B,Hq,S,D], dK, dV [B,Hkv,Sk,D] in ``dt`` from dO [B,S,Hq*D], O [B,Hq,S,D] and lse.
    ``model``: the kernel's documented roundings (dS and P to bf16 before their products)."""
    B, Hq, S, D = q.shape
    Hkv, Sk = k.shape[1], k.shape[2]
    G = Hq // Hkv
    x, vis = _scores(q, k, causal, scale, dt)
    p = torch.exp2(x - lse.to(dt).unsqueeze(-1)).masked_fill(~vis, 0.0)
    doh = do.to(dt).view(B, S, Hq, D).transpose(1, 2)
    dp = doh @ v.to(dt).repeat_interleave(G, 1).transpose(-1, -2)
    delta = (doh * o.to(dt)).sum(-1, keepdim=True)
    ds = p * (dp - delta)
    if scales is not None:  # the magnitudes the gradients' errors are relative to (module doc)
        mag = p * (dp.abs() + delta.abs())
        scales.append((mag @ k.to(dt).abs().repeat_interleave(G, 1)).max() * scale)
        scales.append((mag.transpose(-1, -2) @ q.to(dt).abs()).view(B, Hkv, G, Sk, D).sum(2).max() * scale)
        scales.append((p.transpose(-1, -2) @ doh.abs()).view(B, Hkv, G, Sk, D).sum(2).max())
    if model:
        ds, p = ds.to(BF16).to(dt), p.to(BF16).to(dt)
    dq = (ds @ k.to(dt).repeat_interleave(G, 1)) * scale
    dk = (ds.transpose(-1, -2) @ q.to(dt)).view(B, Hkv, G, Sk, D).sum(2) * scale
    dv = (p.transpose(-1, -2) @ doh).view(B, Hkv, G, Sk, D).sum(2)
    return dq, dk, dv


def attn_ref64(case, inputs=None):
    """The exact function of the bf16 inputs in fp64: O [B,Hq,S,D], lse, dQ, dK, dV, and the three
    gradient magnitudes (``scales``: fp64 scalars)."""
    q, k, v, do = inputs if inputs is not None else attn_inputs(case)
    causal, scale = case[6], 1.0 / math.sqrt(case[5])
    o, lse = attn_fwd_model(q, k, v, causal, scale, torch.float64, False)
    scales = []
    return (o, lse) + attn_bwd_model(do, q, k, v, o, lse, causal, scale, torch.float64, False, scales) + (scales,)


def attn_fp32(case):
    """The fp32 model at the same inputs; its backward reads its own rounded O and its fp32 lse."""
    q, k, v, do = attn_inputs(case)
    causal, scale = case[6], 1.0 / math.sqrt(case[5])
    o, lse = attn_fwd_model(q, k, v, causal, scale, torch.float32, True)
    return (o, lse) + attn_bwd_model(do, q, k, v, o.to(BF16), lse, causal, scale, torch.float32, True)


def tok(o_heads):
    """[B,Hq,S,D] -> the kernels' token-major [B,S,Hq*D]."""
    B, Hq, S, D = o_heads.shape
    return o_heads.transpose(1, 2).reshape(B, S, Hq * D)


def check_attention(case, fwd, bwd, dev, modes=MODES):
    """Forward and every backward mode of one case against fp64.  ``fwd(q, k, v, causal, scale)`` ->
    (o [B,S,Hq*D], lse); ``bwd(do, q, k, v, o, lse, causal, scale, mode)`` -> (dq, dK partials, dV
    partials): the native ops on the GPU, the reference ops on the CPU (tests/test_mfma_inputs.py)."""
    B, Hq, Hkv, S, Sk, D, causal = case
    scale = 1.0 / math.sqrt(D)
    q, k, v, do = [t.to(dev) for t in attn_inputs(case)]
    ro, rlse, rdq, rdk, rdv, (sq, sk, sv) = attn_ref64(case, (q, k, v, do))
    o, lse = fwd(q, k, v, causal, scale)
    assert o.shape == (B, S, Hq * D) and lse.shape == (B, Hq, S)
    assert_parity(o.view(B, S, Hq, D), tok(ro).view(B, S, Hq, D), P.ATTN_O, name="O")
    assert_parity(lse, rlse, P.ATTN_LSE, scale="tensor", name="lse")
    for mode in modes:
        dq, dkp, dvp = bwd(do, q, k, v, o, lse, causal, scale, mode)
        assert dq.shape == (B, Hq, S, D)
        assert_parity(dq, rdq, P.ATTN_DQ, scale=float(sq), name=f"dQ (mode {mode})")
        dk = dkp.double().view(B, Hkv, -1, Sk, D).sum(2)
        dv = dvp.double().view(B, Hkv, -1, Sk, D).sum(2)
        assert_parity(dk, rdk, P.ATTN_DK, scale=float(sk), name=f"dK (mode {mode})")
        assert_parity(dv, rdv, P.ATTN_DV, scale=float(sv), name=f"dV (mode {mode})")
    return o, lse


def native_fwd(q, k, v, causal, scale):
    return _ops().attn_fwd(q, k, v, causal, scale)


def native_bwd(do, q, k, v, o, lse, causal, scale, mode):
    return _ops().attn_bwd(do, q, k, v, o, lse, causal, scale, mode)


@pytest.mark.parametrize("case", ATTN_CASES, ids=ATTN_IDS)
def test_attention_fwd_bwd_per_element(gpu, case):
    check_attention(case, native_fwd, native_bwd, gpu)


HPW_CASES = [(c, h) for c in ATTN_CASES if c[5] == 128 for h in (1, 2, 4) if (c[1] // c[2]) % h == 0]


@pytest.mark.parametrize("case,hpw", HPW_CASES, ids=[f"{case_id(c)}-hpw{h}" for c, h in HPW_CASES])
def test_attention_bwd_heads_per_workgroup_per_element(gpu, case, hpw, monkeypatch):
    """The 8-wave split backward with 1, 2 and 4 q-heads of a KV group per workgroup (where that
    divides the group)."""
    monkeypatch.setenv("MXLLM_ATTN_BWD8_HPW", str(hpw))
    check_attention(case, native_fwd, native_bwd, gpu, modes=(3,))


def dqkv_parts(x, Hq, Hkv, D):
    """d(qkv) rows [T, (Hq+2Hkv)*D] -> its q, k and v columns as [T, heads, D]: each has its own
    magnitude (dK and dV sum a KV group's heads), so each is bounded against its own max."""
    T = x.shape[0]
    return (x[:, :Hq * D].reshape(T, Hq, D), x[:, Hq * D:(Hq + Hkv) * D].reshape(T, Hkv, D),
            x[:, (Hq + Hkv) * D:(Hq + 2 * Hkv) * D].reshape(T, Hkv, D))


def rope_dqkv_ref64(case, cos, sin):
    B, Hq, Hkv, S, _, D, _ = case
    _, _, rdq, rdk, rdv, scales = attn_ref64(case)
    return _rope_merge(rdq, rdk, rdv, cos, sin, B, S, Hq, Hkv, D, torch.float64), scales


@pytest.mark.parametrize("out_pad", [0, 64], ids=["pad0", "pad64"])
@pytest.mark.parametrize("case", ROPE_CASES, ids=case_id)
def test_attention_bwd_rope_per_element(gpu, case, out_pad):
    """attn_bwd_rope (the dQ kernel applies the inverse RoPE and writes d(qkv) itself) against the fp64
    rope_merge of the fp64 gradients; one bound per head of a token row."""
    B, Hq, Hkv, S, Sk, D, causal = case
    scale = 1.0 / math.sqrt(D)
    q, k, v, do = [t.to(gpu) for t in attn_inputs(case)]
    cos, sin = [t.to(gpu) for t in rope_tables(S + 3, D)]
    o, lse = _ops().attn_fwd(q, k, v, causal, scale)
    dqkv = _ops().attn_bwd_rope(do, q, k, v, o, lse, causal, scale, cos, sin, out_pad)
    NHD = (Hq + 2 * Hkv) * D
    assert dqkv.shape == (B * S, NHD) and dqkv.stride() == (NHD + out_pad, 1)
    want, scales = rope_dqkv_ref64(case, cos.cpu(), sin.cpu())
    for nm, a, b, s in zip("qkv", dqkv_parts(dqkv, Hq, Hkv, D), dqkv_parts(want.to(gpu), Hq, Hkv, D), scales):
        assert_parity(a, b, P.ATTN_ROPE_DQKV, scale=float(s), name=f"dqkv ({nm} columns)")


PADDED_O_CASES = [(2, 4, 1, 65, 65, 32, True), (2, 4, 1, 129, 129, 64, True), (1, 8, 2, 257, 257, 128, True),
                  (2, 2, 2, 65, 200, 128, True), (1, 2, 1, 130, 70, 128, False)]


@pytest.mark.parametrize("case", PADDED_O_CASES, ids=case_id)
def test_attention_bwd_from_padded_o_is_bitwise(gpu, case):
    """Backward from an ``o`` written with out_pad = 64 (row-strided) equals, bit for bit, the
    backward from a contiguous copy of it."""
    B, Hq, Hkv, S, Sk, D, causal = case
    scale = 1.0 / math.sqrt(D)
    q, k, v, do = [t.to(gpu) for t in attn_inputs(case)]
    o, lse = _ops().attn_fwd(q, k, v, causal, scale, 64)
    assert o.stride() == (S * (Hq * D + 64), Hq * D + 64, 1)
    o0, lse0 = _ops().attn_fwd(q, k, v, causal, scale)
    assert torch.equal(o, o0) and torch.equal(lse, lse0)
    for mode in MODES:
        a = _ops().attn_bwd(do, q, k, v, o, lse, causal, scale, mode)
        b = _ops().attn_bwd(do, q, k, v, o.contiguous(), lse, causal, scale, mode)
        if mode == 1:  # f32 atomics: dQ's summation order is not fixed
            a, b = a[1:], b[1:]
        for x, y in zip(a, b):
            assert torch.equal(x, y), mode


def test_attention_bwd_chunked_ds_image_per_element(gpu, monkeypatch):
    """The bounded-memory split backward (mxllm/ops/attention.py: per sequence and KV-group chunk
    when the dS^T image exceeds its budget) meets the same per-element bound as the one-call path."""
    from mxllm.ops import attention as A

    case = DS_BUDGET_CASE
    per_head = A._ds_bytes_per_head(case[3], case[4])
    monkeypatch.setattr(A, "_DS_BUDGET", 4.5 * per_head)  # one KV group (4 heads) per chunk: 2 x 2 chunks
    calls = []
    real = _ops().attn_bwd

    class Spy:
        def __getattr__(self, name):
            if name == "attn_bwd":
                def f(*a):
                    calls.append(a[1].shape)
                    return real(*a)
                return f
            return getattr(_ops(), name)

    monkeypatch.setattr(A, "native", lambda: Spy())

    def bwd(do, q, k, v, o, lse, causal, scale, mode):
        return A.attn_bwd(do, q, k, v, o, lse, causal, scale, mode)

    check_attention(case, native_fwd, bwd, gpu, modes=(3,))
    assert len(calls) == 4 and all(tuple(s) == (1, 4, 257, 128) for s in calls)


# =========================================================================== yardstick
def _meas(acc, name, y32, r64, out_dtype, scale):
    """As tests/test_rowwise_strict_gpu._meas (rel: the output rounding; abs: the model against fp64),
    with assert_parity's three kinds of scale."""
    y, r = y32.double(), r64.double()
    s = (r.abs().amax(-1, keepdim=True) if scale == "row" else r.abs().max() if scale == "tensor"
         else torch.as_tensor(scale, dtype=torch.float64)).expand_as(r)
    ok = s > 0
    ab = ((y - r).abs()[ok] / s[ok]).max().item() if ok.any() else 0.0
    nz = y.abs() >= torch.finfo(out_dtype).tiny
    rel = ((y32.to(out_dtype).double() - y).abs()[nz] / y.abs()[nz]).max().item() if nz.any() else 0.0
    cur = acc.get(name, (0.0, 0.0))
    acc[name] = (max(cur[0], rel), max(cur[1], ab))


def measure():
    """Error of the fp32 model against fp64 at the tests' inputs, on the CPU: the ``ATTN_*_MEASURED``
    constants of tests/_parity.py (max over every case, the chunked-path case included)."""
    acc = {}
    f32 = torch.float32
    for case in ATTN_CASES + [DS_BUDGET_CASE]:
        B, Hq, Hkv, S, Sk, D, causal = case
        (o, lse, dq, dk, dv), (ro, rlse, rdq, rdk, rdv, (sq, sk, sv)) = attn_fp32(case), attn_ref64(case)
        _meas(acc, "ATTN_O", o, ro, BF16, "row")
        _meas(acc, "ATTN_LSE", lse, rlse, f32, "tensor")
        _meas(acc, "ATTN_DQ", dq, rdq, f32, sq)
        _meas(acc, "ATTN_DK", dk, rdk, f32, sk)
        _meas(acc, "ATTN_DV", dv, rdv, f32, sv)
        if case in ROPE_CASES:
            cos, sin = rope_tables(S + 3, D)
            a = _rope_merge(dq, dk, dv, cos, sin, B, S, Hq, Hkv, D, f32)
            b = _rope_merge(rdq, rdk, rdv, cos, sin, B, S, Hq, Hkv, D, torch.float64)
            for x, y, s in zip(dqkv_parts(a, Hq, Hkv, D), dqkv_parts(b, Hq, Hkv, D), (sq, sk, sv)):
                _meas(acc, "ATTN_ROPE_DQKV", x, y, BF16, s)
    for name, (rel, ab) in acc.items():
        print(f"{name}_MEASURED = ({rel:.3g}, {ab:.3g})")
    return acc


if __name__ == "__main__":
    measure()
