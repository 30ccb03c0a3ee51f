"""Exact (no tolerance) tests of the MFMA kernels: gemm8.hip, lora.hip, attn_fwd.hip, attn_bwd.hip.

Integer GEMM.  Operands are small integers stored in bf16 with max_ij sum_k |a_ik| |b_kj| (times
|alpha|, plus |C0| when beta is 1) < 2^24: every fp32 partial sum is then an integer below 2^24 and
exact in ANY summation order, so an fp32 output must equal the fp64 product bit for bit and a bf16
output its round-to-nearest-even (the kernels convert with __float2bfloat16).  One wrong 16 x 16
fragment, one dropped K-tile, a row read past K or a store into a pad column changes integers.

One-hot attention.  Keys are c * (+-1 codes), every query is c * the code of one visible key; with
the matching score >= 300 log2 units above every other one P is exactly one-hot in fp32, so
O[b, i, h] = V[b, h / G, pi(i)] bit for bit, dS = P (dP - delta) is an exact zero (integer V and dO:
delta = dO . O = dP at the chosen key), dQ = dK = 0 and dV is the scatter-add of the dO rows.

Inputs are built on the CPU from fixed seeds; ``tests/test_mfma_inputs.py`` asserts the input
conditions and runs the reference ops through the same checks without a GPU.
"""
import functools
import math

import pytest
import torch

from tests import _parity as P
from tests._parity import assert_exact, assert_parity
from tests.test_attention_strict_gpu import ATTN_CASES, LOG2E, case_id

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
F32 = torch.float32
POISON = 64.0      # pad columns and rows past K of the operands: any read of one shows in the integers
SENTINEL = -77.0   # pad columns of the outputs (exact in bf16)
PADS = (8, 24, 16)  # row pads of A, B and the output: three different strides
EXACT_LIMIT = 2 ** 24


def _ops():
    from mxllm.ops import native

    return native()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).to(F32)


def _padded(vals, pad, extra_rows=0, dtype=BF16):
    """``vals`` [R, C] inside a [R + extra_rows, C + pad] buffer whose other elements hold POISON."""
    R, C = vals.shape
    buf = torch.full((R + extra_rows, C + pad), POISON, dtype=dtype)
    buf[:R, :C] = vals.to(dtype)
    return buf


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


# =========================================================================== gemm8
ORDERS = [(True, True), (True, False), (False, True), (False, False)]  # (a_kc, b_kc)
GEMM_MN = [(256, 256), (512, 768), (768, 256)]
K_KC = [64, 128, 192, 640]           # an operand k-contiguous: 1, 2, 3 and 10 K-tiles
K_TT = [1, 63, 65, 100, 192, 1000]   # both token-major: any K, rows past K read as zeros
GEMM_CASES = [(o, mn, K) for o in ORDERS for mn in GEMM_MN for K in (K_KC if o[0] or o[1] else K_TT)]
PERSIST_CASES = [(o, (4096, 4352), 192 if o[0] or o[1] else 100) for o in ORDERS]  # 272 tiles > the CU count
# (out fp32, beta, alpha_t, alpha); alpha_t on the device, both alphas powers of two: still exact
VARIANTS = [(True, 0.0, None, 1.0), (False, 0.0, None, 1.0), (True, 1.0, None, 1.0), (False, 1.0, None, 1.0)]
ALPHA_VARIANTS = [(True, 1.0, 0.5, 4.0), (False, 0.0, 0.5, 4.0)]


def gemm_id(c):
    (a_kc, b_kc), (M, N), K = c
    return f"A{'k' if a_kc else 'm'}B{'k' if b_kc else 'n'}-M{M}-N{N}-K{K}"  # k: k-contiguous; m / n: token-major


@functools.lru_cache(maxsize=2)
def gemm_case(case):
    """Buffers (CPU) and the fp64 product of one case.  A in 0..3, B in -1..3 (biased: the sums grow
    with K and need rounding to bf16), C0 in -8..8.  Token-major operands ([K, M] / [K, N]) continue
    for 64..127 poison rows past row K inside the same allocation."""
    (a_kc, b_kc), (M, N), K = case
    g = _gen(100 + 7 * M + 3 * N + K + 2 * a_kc + b_kc)
    A = _ints(g, 0, 3, M, K)   # [M, K]
    B = _ints(g, -1, 3, K, N)  # [K, N]
    extra = (K + 63) // 64 * 64 - K + 64
    a_buf = _padded(A, PADS[0]) if a_kc else _padded(A.t(), PADS[0], extra)
    b_buf = _padded(B.t(), PADS[1]) if b_kc else _padded(B, PADS[1], extra)
    c0 = _ints(g, -8, 8, M, N)
    prod = A.double() @ B.double()
    absprod = float((A.abs().double() @ B.abs().double()).max())
    return dict(a_buf=a_buf, b_buf=b_buf, a_shape=(M, K) if a_kc else (K, M), b_shape=(N, K) if b_kc else (K, N),
                c0=c0, prod=prod, absprod=absprod)


def gemm_expected(c, out_f32, beta, alpha):
    """fp64 reference and the exact expected output; asserts the < 2^24 condition."""
    ref = alpha * c["prod"] + (c["c0"].double() if beta else 0.0)
    assert abs(alpha) * c["absprod"] + (8 if beta else 0) < EXACT_LIMIT
    want = ref.to(F32)
    assert torch.equal(want.double(), ref)
    return ref, (want if out_f32 else want.to(BF16))  # fp32 -> bf16: round to nearest even


def unrepresentable_share(ref):
    return float((ref.to(F32).to(BF16).double() != ref).double().mean())


def view(buf, shape):
    return buf[:shape[0], :shape[1]]


def out_buffer(c, M, N, out_f32, beta, dev):
    """[M, N + pad]: C0 (beta 1) or NaN (beta 0: must be ignored) with sentinel pad columns."""
    dt = F32 if out_f32 else BF16
    buf = torch.full((M, N + PADS[2]), SENTINEL, dtype=dt)
    buf[:, :N] = c["c0"].to(dt) if beta else float("nan")
    return buf.to(dev)


def check_gemm(case, run, dev, variants):
    """``run(a, a_kc, b, b_kc, out, beta, alpha_t, alpha) -> bool`` over the variants of one case."""
    (a_kc, b_kc), (M, N), K = case
    c = gemm_case(case)
    a_buf, b_buf = c["a_buf"].to(dev), c["b_buf"].to(dev)
    a, b = view(a_buf, c["a_shape"]), view(b_buf, c["b_shape"])
    assert len({a.stride(0) - a.shape[1], b.stride(0) - b.shape[1], PADS[2]}) == 3  # three different pads
    for out_f32, beta, alpha_t, alpha in variants:
        name = f"{gemm_id(case)} {'fp32' if out_f32 else 'bf16'} beta {beta:g} alpha {alpha_t}x{alpha:g}"
        ref, want = gemm_expected(c, out_f32, beta, alpha * (alpha_t or 1.0))
        if not out_f32 and K >= 640:
            assert unrepresentable_share(ref) >= 0.10, name  # the bf16 rounding is exercised
        buf = out_buffer(c, M, N, out_f32, beta, dev)
        at = None if alpha_t is None else torch.tensor([alpha_t], dtype=F32, device=dev)
        assert run(a, a_kc, b, b_kc, buf[:, :N], beta, at, alpha), name
        assert_exact(buf[:, :N], want.to(dev), name)
        assert (buf[:, N:] == SENTINEL).all(), f"{name}: output pad columns written"
    assert torch.equal(a_buf, c["a_buf"].to(dev)) and torch.equal(b_buf, c["b_buf"].to(dev))


def native_gemm8(ph):
    def run(a, a_kc, b, b_kc, out, beta, alpha_t, alpha):
        return _ops().gemm8(a, a_kc, b, b_kc, out, beta, alpha_t, alpha, ph)
    return run


@pytest.mark.parametrize("ph", ["8", "4"])
@pytest.mark.parametrize("case", GEMM_CASES, ids=gemm_id)
def test_gemm8_integer_exact(gpu, case, ph, monkeypatch):
    monkeypatch.setenv("MXLLM_GEMM8_PH", ph)
    alpha = ALPHA_VARIANTS if case[1] == (512, 768) and case[2] in (192, 100) else []
    check_gemm(case, native_gemm8(int(ph)), gpu, VARIANTS + alpha)


@pytest.mark.parametrize("case", PERSIST_CASES, ids=gemm_id)
def test_gemm8_persistent_integer_exact(gpu, case, monkeypatch):
    """MXLLM_GEMM8_PERSIST=1: each workgroup walks several of the 272 tiles."""
    monkeypatch.setenv("MXLLM_GEMM8_PERSIST", "1")
    check_gemm(case, native_gemm8(4), gpu, VARIANTS)


TAIL_CASES = [(o, (512, 768), K) for o in ORDERS for K in (128, 704, 64)]  # K-tiles split 1+1, 5+6; K = 64


def check_gemm_tail(case, rows, run, dev):
    """``run(a, a_kc, b, b_kc, out, at, rows) -> bool``: exact where the launcher accepts, ``out``
    untouched where it declines (K = 64: fewer than two K-tiles to split)."""
    (a_kc, b_kc), (M, N), K = case
    c = gemm_case(case)
    a = view(c["a_buf"].to(dev), c["a_shape"])
    b = view(c["b_buf"].to(dev), c["b_shape"])
    ref, want = gemm_expected(c, False, 0.0, 1.0)
    if K >= 640:
        assert unrepresentable_share(ref) >= 0.10
    buf = out_buffer(c, M, N, False, 0.0, dev)
    before = buf.clone()
    name = f"tail {gemm_id(case)} {'rows' if rows else 'columns'}"
    if run(a, a_kc, b, b_kc, buf[:, :N], 256, rows):
        assert K >= 128, name
        assert_exact(buf[:, :N], want.to(dev), name)
        assert (buf[:, N:] == SENTINEL).all(), f"{name}: output pad columns written"
    else:
        assert K < 128, name
        assert torch.equal(bits(buf), bits(before)), f"{name}: declined but wrote"


@pytest.mark.parametrize("ph", [4, 8])
@pytest.mark.parametrize("rows", [False, True], ids=["columns", "rows"])
@pytest.mark.parametrize("case", TAIL_CASES, ids=gemm_id)
def test_gemm8_tail_integer_exact(gpu, case, rows, ph):
    check_gemm_tail(case, rows, lambda a, ak, b, bk, out, at, r: _ops().gemm8_tail(a, ak, b, bk, out, at, r, ph), gpu)


@pytest.mark.parametrize("case", [(o, mn, 192 if o[0] or o[1] else 100) for o in ORDERS for mn in GEMM_MN], ids=gemm_id)
def test_gemm8_sq_integer_exact(gpu, case):
    """gemm8_sq: the output exact (device alpha 0.5 x host alpha 4), the per-tile sums of squares of
    the stored values as before (allclose), nothing past the tiles."""
    (a_kc, b_kc), (M, N), K = case
    c = gemm_case(case)
    a = view(c["a_buf"].to(gpu), c["a_shape"])
    b = view(c["b_buf"].to(gpu), c["b_shape"])
    _, want = gemm_expected(c, False, 0.0, 2.0)
    buf = out_buffer(c, M, N, False, 0.0, gpu)
    nt = (M // 256) * (N // 256)
    sq = torch.full((nt + 3,), -1.0, device=gpu)
    assert _ops().gemm8_sq(a, a_kc, b, b_kc, buf[:, :N], sq, torch.tensor([0.5], device=gpu), 4.0)
    assert_exact(buf[:, :N], want.to(gpu), f"sq {gemm_id(case)}")
    assert (buf[:, N:] == SENTINEL).all()
    tiles = want.to(gpu).float().pow(2).view(M // 256, 256, N // 256, 256).sum(dim=(1, 3)).flatten()
    assert torch.allclose(sq[:nt], tiles, rtol=1e-5, atol=0), (sq[:nt] - tiles).abs().max().item()
    assert (sq[nt:] == -1.0).all()


# =========================================================================== lora_xwt
XWT_SHAPES = [(16, 128), (48, 384), (64, 192), (256, 512)]
XWT_PAD = 64  # the augmented GEMMs' spare columns: the adapter's rank columns live there


@functools.lru_cache(maxsize=2)
def xwt_case(T, K):
    """buf [T, K + 64 + 8]: x (0..3) | the 64 output columns | 8 sentinel columns; v [64, K] (-1..3)
    in a [64, K + 16] buffer -- all 64 rows non-zero, so a kernel told ``rows`` must not read past them."""
    g = _gen(300 + T + K)
    x, v = _ints(g, 0, 3, T, K), _ints(g, -1, 3, XWT_PAD, K)
    buf = torch.full((T, K + XWT_PAD + 8), SENTINEL, dtype=BF16)
    buf[:, :K] = x.to(BF16)
    assert float((x.abs().double() @ v.abs().double().t()).max()) * 2.0 < EXACT_LIMIT
    return buf, _padded(v, 16), 2.0 * (x.double() @ v.double().t())


def xwt_path(kern, T, K):
    """What mx_lora_xwt does with this call: the row-tiled kernel (adapter rows only, zeros in the
    rest of the pad), the 64-row kernels (all rows of v), or a refusal (they need T % 64)."""
    if kern == "tile" and K % 128 == 0:
        return "tile"
    return "rows64" if T % 64 == 0 else "refused"


def check_lora_xwt(T, K, kern, rows, run, dev):
    """``run(x, v, out, alpha, rows)``; alpha 2.0."""
    buf0, v_buf, ref = xwt_case(T, K)
    buf, v = buf0.to(dev), v_buf.to(dev)[:, :K]
    out = buf[:, K:K + XWT_PAD]
    name = f"lora_xwt {kern} T{T} K{K} rows{rows}"
    path = xwt_path(kern, T, K)
    if path == "refused":
        with pytest.raises(RuntimeError):
            run(buf[:, :K], v, out, 2.0, rows)
        assert torch.equal(buf, buf0.to(dev)), f"{name}: refused but wrote"
        return
    run(buf[:, :K], v, out, 2.0, rows)
    want = ref.to(F32).to(BF16)
    if path == "tile":
        want[:, rows:] = 0
    assert_exact(out, want.to(dev), name)
    assert torch.equal(buf[:, :K], buf0[:, :K].to(dev)) and (buf[:, K + XWT_PAD:] == SENTINEL).all(), \
        f"{name}: columns outside the 64-column pad written"


@pytest.mark.parametrize("rows", [16, 32, 48, 64])
@pytest.mark.parametrize("kern", ["lds", "reg", "tile"])
@pytest.mark.parametrize("T,K", XWT_SHAPES)
def test_lora_xwt_integer_exact(gpu, T, K, kern, rows, monkeypatch):
    monkeypatch.setenv("MXLLM_LORA_XWT", kern)
    check_lora_xwt(T, K, kern, rows, lambda x, v, out, alpha, r: _ops().lora_xwt(x, v, out, alpha, r), gpu)


# =========================================================================== lora_grads
GRADS_T = 256
GRADS_CONFIGS = [(512, (512, 128, 128), 16), (1024, (1024, 256, 256), 16), (256, (1024, 1024), 16),
                 (320, (192,), 16), (512, (512, 256, 256), 32)]  # (K, splits, r)


@functools.lru_cache(maxsize=2)
def grads_case(K, splits, r):
    """xa [T, K + pad] = x | st, dya [T, N + pad] = dy | g (the augmented layouts), integers -2..2 /
    -1..3; ga0 [R, K], gb0 [N, R] integers -8..8; the expected dA and diagonal dB blocks in fp64."""
    T, n, N = GRADS_T, len(splits), sum(splits)
    R = n * r
    pad = (R + 63) // 64 * 64
    g = _gen(400 + K + N + r)
    xa, dya = _ints(g, -2, 2, T, K + pad).to(BF16), _ints(g, -1, 3, T, N + pad).to(BF16)
    ga0, gb0 = _ints(g, -8, 8, R, K), _ints(g, -8, 8, N, R)
    x, st, dy, gg = xa[:, :K].double(), xa[:, K:].double(), dya[:, :N].double(), dya[:, N:].double()
    da = gg[:, :R].t() @ x
    db, off = [], 0
    for i, ni in enumerate(splits):
        db.append(dy[:, off:off + ni].t() @ st[:, i * r:(i + 1) * r])
        off += ni
    assert T * 2 * 3 + 8 < EXACT_LIMIT
    return xa, dya, ga0, gb0, da, db


def check_lora_grads(K, splits, r, acc, run, dev):
    """``run(x, dy, g, st, ga, gb, splits, r, accumulate)``."""
    xa, dya, ga0, gb0, da, db = grads_case(K, splits, r)
    N, R = sum(splits), len(splits) * r
    want_a = (da + (ga0.double() if acc else 0.0)).to(F32).to(BF16)
    want_b = gb0.clone().to(BF16)
    ga, gb = ga0.clone().to(BF16), gb0.clone().to(BF16)
    if not acc:
        ga[:] = float("nan")  # written fresh: must be ignored
    off = 0
    for i, ni in enumerate(splits):
        blk = (slice(off, off + ni), slice(i * r, (i + 1) * r))
        want_b[blk] = (db[i] + (gb0[blk].double() if acc else 0.0)).to(F32).to(BF16)
        if not acc:
            gb[blk] = float("nan")
        off += ni
    xa, dya, ga, gb = xa.to(dev), dya.to(dev), ga.to(dev), gb.to(dev)
    run(xa[:, :K], dya[:, :N], dya[:, N:], xa[:, K:], ga, gb, list(splits), r, acc)
    name = f"lora_grads K{K} splits{splits} r{r} acc{acc}"
    assert_exact(ga, want_a.to(dev), f"{name}: dA")
    assert_exact(gb, want_b.to(dev), f"{name}: dB (diagonal blocks exact, off-diagonal blocks untouched)")


@pytest.mark.parametrize("wt", ["0", "1"])
@pytest.mark.parametrize("fused", ["0", "1"])
@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("K,splits,r", GRADS_CONFIGS)
def test_lora_grads_integer_exact(gpu, K, splits, r, acc, fused, wt, monkeypatch):
    monkeypatch.setenv("MXLLM_LORA_FUSED_RED", fused)
    monkeypatch.setenv("MXLLM_LORA_XTG_WT", wt)
    monkeypatch.setenv("MXLLM_LORA_XTG_WT_MIN", "16")  # the one-tile-per-wave form takes these small shapes
    check_lora_grads(K, splits, r, acc, lambda *a: _ops().lora_grads(*a), gpu)


# =========================================================================== one-hot attention
ONEHOT_CASES = [c for c in ATTN_CASES if c[6]]
MIN_GAP_LOG2 = 300.0


def onehot_c(D):
    return 8.0 if D == 128 else 16.0


@functools.lru_cache(maxsize=4)
def onehot_case(case):
    """q, k (c * codes), pi [B,Hq,S] (the chosen key: <= i + Sk - S, the diagonal for every third
    query), integer v (-4..4), a real-valued v and integer dO (-2..2), on the CPU."""
    B, Hq, Hkv, S, Sk, D, causal = case
    assert causal
    G, c = Hq // Hkv, onehot_c(D)
    g = _gen(500 + 131 * S + 17 * Sk + D + Hq)
    codes = _ints(g, 0, 1, B, Hkv, Sk, D) * 2 - 1
    i = torch.arange(S).view(1, 1, S)
    pi = (torch.rand(B, Hq, S, generator=g) * (i + Sk - S + 1)).long().clamp_(max=Sk - 1)
    pi = torch.minimum(pi, i + Sk - S)
    pi = torch.where(i % 3 == 0, i + Sk - S, pi)
    kv_of = torch.arange(Hq) // G
    q = codes[torch.arange(B).view(B, 1, 1), kv_of.view(1, Hq, 1), pi]  # [B,Hq,S,D]
    v_int = _ints(g, -4, 4, B, Hkv, Sk, D).to(BF16)
    v_real = torch.randn(B, Hkv, Sk, D, generator=g).to(BF16)
    do = _ints(g, -2, 2, B, S, Hq * D).to(BF16)
    return (c * q).to(BF16), (c * codes).to(BF16), pi, v_int, v_real, do


def onehot_gap(case):
    """log2 units between the matching score and the best other key's, from the worst code correlation."""
    D = case[5]
    _, k, _, _, _, _ = onehot_case(case)
    codes = k.double() / onehot_c(D)
    corr = codes @ codes.transpose(-1, -2)
    Sk = corr.shape[-1]
    worst = corr.masked_fill(torch.eye(Sk, dtype=torch.bool), -D).max().item() if Sk > 1 else -D
    return onehot_c(D) ** 2 * (D - worst) / math.sqrt(D) * LOG2E


def onehot_expected(case, v):
    """O [B,S,Hq*D] = V[b, h / G, pi] and the lse (log2 domain) of a one-hot row: the matching score."""
    B, Hq, Hkv, S, Sk, D, _ = case
    pi = onehot_case(case)[2]
    kv_of = (torch.arange(Hq) // (Hq // Hkv)).view(1, Hq, 1)
    o = v[torch.arange(B).view(B, 1, 1), kv_of, pi]  # [B,Hq,S,D]
    lse = torch.full((B, Hq, S), onehot_c(D) ** 2 * D / math.sqrt(D) * LOG2E, dtype=torch.float64)
    return o.transpose(1, 2).reshape(B, S, Hq * D), lse


def onehot_dv(case):
    """fp64 scatter-add of the dO rows over the queries and the q-heads of the group that chose each key."""
    B, Hq, Hkv, S, Sk, D, _ = case
    _, _, pi, _, _, do = onehot_case(case)
    G = Hq // Hkv
    doh = do.double().view(B, S, Hkv, G, D).permute(0, 2, 3, 1, 4).reshape(B, Hkv, G * S, D)
    idx = pi.view(B, Hkv, G * S, 1).expand(-1, -1, -1, D)
    return torch.zeros(B, Hkv, Sk, D, dtype=torch.float64).scatter_add_(2, idx, doh)


def check_onehot(case, fwd, bwd, dev, modes=(1, 2, 3)):
    """``fwd`` / ``bwd`` as in tests/test_attention_strict_gpu.check_attention."""
    B, Hq, Hkv, S, Sk, D, causal = case
    scale = 1.0 / math.sqrt(D)
    assert onehot_gap(case) >= MIN_GAP_LOG2
    q, k, _, v_int, v_real, do = [t.to(dev) for t in onehot_case(case)]
    name = f"one-hot {case_id(case)}"
    for v in (v_real, v_int):
        want_o, want_lse = onehot_expected(case, v.cpu())
        o, lse = fwd(q, k, v, causal, scale)
        assert_exact(o, want_o.to(dev), f"{name}: O")
        assert_parity(lse, want_lse.to(dev), P.ATTN_LSE, scale="tensor", name=f"{name}: lse")
    ref_dv = onehot_dv(case)
    want_dv = ref_dv.to(F32)
    assert torch.equal(want_dv.double(), ref_dv)
    for mode in modes:
        dq, dkp, dvp = bwd(do, q, k, v_int, o, lse, causal, scale, mode)
        assert_exact(dq, torch.zeros(B, Hq, S, D, device=dev), f"{name}: dQ (mode {mode})")
        assert_exact(dkp, torch.zeros_like(dkp), f"{name}: dK partials (mode {mode})")
        dv = dvp.view(B, Hkv, -1, Sk, D).sum(2)  # integers: exact in fp32
        assert_exact(dv, want_dv.to(dev), f"{name}: dV (mode {mode})")


@pytest.mark.parametrize("case", ONEHOT_CASES, ids=case_id)
def test_attention_onehot_exact(gpu, case):
    from tests.test_attention_strict_gpu import native_bwd, native_fwd

    check_onehot(case, native_fwd, native_bwd, gpu)
