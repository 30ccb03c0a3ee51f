"""Exact and per-element tests of the decode GEMMs: csrc/kernels/skinny_gemm.hip, fp8_gemm.hip and the
fused prologues / epilogues of decode_fuse.h.

Permutation weights.  Every row of W holds a single 1.0, at column pi(n); the other products are exact
zeros, so skinny_linear(x, W)[m, n] = x[m, pi(n)] whatever the accumulation order (a -0.0 of x comes out
as +0.0: the accumulator starts at +0.0 and +0.0 + -0.0 = +0.0).  pi visits every position of a 64-k
chunk, every one of the eight wave K parts and every chunk of the unrolled and the tail loop: one device
for the k-permutation of the X / W fragments, the K split, the channel and token maps and the row clamp.
Behind a fused epilogue (SwiGLU, RoPE + KV append) or prologue (RMSNorm) the GEMM is then an exact
selection and the fused piece is checked per element against fp64, alone.

Integer operands.  x and W hold integers in -4..4, |sum| < 2^24: the output is the bf16 rounding of the
fp64 product (assert_exact); every k of every channel contributes.

FP8.  Every code the quantiser can emit decodes exactly; integer codes +-1..+-4 with power-of-two channel
scales give an exact w8_linear; quant_rows_e4m3 is bitwise the same fp32 expressions on the CPU.

NaN fills the pad columns of every strided operand and the rows past M.  Inputs are built on the CPU
from fixed seeds, expectations on the CPU in fp64 or by indexing.  ``tests/test_decode_inputs.py`` runs
the CPU references through the same checks.  ``python -m tests.test_skinny_exact_gpu`` prints the measured
constants of tests/_parity.py (no GPU); ``--nc 2|4`` runs the MXLLM_SKINNY_NC cases (GPU, fresh process).
"""
import functools
import os
import subprocess
import sys

import pytest
import torch

from tests import _parity as P
from tests import test_decode_exact_gpu as TD
from tests._parity import assert_exact, assert_parity

pytestmark = pytest.mark.gpu

BF16, F32, F64, I32 = torch.bfloat16, torch.float32, torch.float64, torch.int32
NAN = float("nan")
EXACT_LIMIT = 2 ** 24
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bits = TD.bits


def _ops():
    from mxllm.ops import native

    return native()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def padded(vals, pad, extra_rows=0, fill=NAN):
    """``vals`` [R, C] inside a [R + extra_rows, C + pad] buffer whose other elements hold ``fill``."""
    R, C = vals.shape
    buf = torch.full((R + extra_rows, C + pad), fill, dtype=vals.dtype)
    buf[:R, :C] = vals
    return buf


def strided(vals, pad, extra_rows, dev, fill=NAN):
    """The [R, C] row-strided view of such a buffer on ``dev``."""
    R, C = vals.shape
    return padded(vals, pad, extra_rows, fill).to(dev)[:R, :C]


# =========================================================================== operands
@functools.lru_cache(maxsize=4)
def perm_map(N, K):
    """pi [N]: a seeded permutation of the columns (N <= K) or a map with repeats that covers every column."""
    g = _gen(3000 + N + K)
    reps = (N + K - 1) // K
    return torch.cat([torch.randperm(K, generator=g) for _ in range(reps)])[:N]


@functools.lru_cache(maxsize=2)
def perm_weight(N, K):
    w = torch.zeros(N, K, dtype=BF16)
    w[torch.arange(N), perm_map(N, K)] = 1.0
    return w


@functools.lru_cache(maxsize=2)
def int_weight(N, K):
    return torch.randint(-4, 5, (N, K), generator=_gen(3100 + N + K)).to(BF16)


@functools.lru_cache(maxsize=2)
def gauss_weight(N, K):
    return (torch.randn(N, K, generator=_gen(3200 + N + K)) * 0.05).to(BF16)


BF16_MAX = 3.3895313892515355e38
BF16_TINY = 2.0 ** -126


def finite_x(M, K, seed, extremes=True):
    """Gaussian bf16 with some +-0 and, ``extremes``, the largest and the smallest normal bf16 of both signs."""
    g = _gen(seed)
    x = torch.randn(M, K, generator=g)
    sel = torch.rand(M, K, generator=g)
    x[sel < 0.02] = 0.0
    x[sel > 0.98] = -0.0
    if extremes:
        for i, v in enumerate((BF16_MAX, -BF16_MAX, BF16_TINY, -BF16_TINY)):
            x[(sel > 0.1 + 0.01 * i) & (sel < 0.105 + 0.01 * i)] = v
    return x.to(BF16)


def int_x(M, K, seed, lim=4):
    return torch.randint(-lim, lim + 1, (M, K), generator=_gen(seed)).to(BF16)


def gauss_x(M, K, seed):
    return torch.randn(M, K, generator=_gen(seed)).to(BF16)


def select(x, pi):
    """x[:, pi] with -0.0 read as +0.0 (see the module docstring), same dtype."""
    y = x[:, pi].clone()
    y[y == 0] = 0.0
    return y


# =========================================================================== skinny_linear
LIN_M = (1, 15, 16, 17, 31, 32)   # <1, .> up to 16 rows, <2, .> above; the clamp of rows >= M
LIN_K = (512, 4096, 4608)         # per wave: the tail loop only, one unrolled batch, a batch and a tail chunk
LIN_N = (16, 1040, 4096)
LIN_CASES = [(M, N, K) for N in LIN_N for K in LIN_K for M in LIN_M]
GAUSS_LIN_CASES = [(1, 1040, 512), (16, 4096, 4608), (17, 1040, 4096), (32, 16, 4608)]


def lin_expected(kind, M, N, K):
    """(x, w, the exact expected output or None, the fp64 reference)."""
    seed = 3300 + 64 * M + N + K
    if kind == "perm":
        x, w = finite_x(M, K, seed), perm_weight(N, K)
        want = select(x, perm_map(N, K))
        return x, w, want, want.double()
    if kind == "int":
        x, w = int_x(M, K, seed), int_weight(N, K)
        r64 = x.double() @ w.double().t()
        assert float((x.abs().double() @ w.abs().double().t()).max()) < EXACT_LIMIT
        return x, w, r64.to(F32).to(BF16), r64
    x, w = gauss_x(M, K, seed), gauss_weight(N, K)
    return x, w, None, x.double() @ w.double().t()


def check_linear(kind, M, N, K, run, dev, bound=None, xpad=24, wpad=8):
    """``run(x, w) -> y``.  x: a row-strided view with NaN pad columns and NaN rows after row M - 1;
    W row-strided with NaN pads."""
    x, w, want, r64 = lin_expected(kind, M, N, K)
    xd, wd = strided(x, xpad, 3, dev), strided(w, wpad, 0, dev)
    y = run(xd, wd).cpu()
    name = f"{kind} M{M} N{N} K{K}"
    if want is not None:
        assert_exact(bits(y), bits(want), name)
    else:
        assert_parity(y, r64, bound or P.SKINNY_Y, name=name)
    return y, r64


@pytest.mark.parametrize("kind", ["perm", "int"])
@pytest.mark.parametrize("M,N,K", LIN_CASES)
def test_skinny_linear_exact(gpu, M, N, K, kind):
    check_linear(kind, M, N, K, _ops().skinny_linear, gpu)


@pytest.mark.parametrize("M,N,K", GAUSS_LIN_CASES)
def test_skinny_linear_gaussian_parity(gpu, M, N, K):
    check_linear("gauss", M, N, K, _ops().skinny_linear, gpu)


def check_linear_refusals(run, dev):
    def go(M, N, K, xpad=24, wpad=8):
        x, w = gauss_x(M, K, 1), gauss_weight(N, K)
        with pytest.raises(RuntimeError):
            run(strided(x, xpad, 0, dev), strided(w, wpad, 0, dev))

    go(33, 16, 512)
    go(4, 24, 512)       # N % 16
    go(4, 16, 768)       # K % 512
    go(4, 16, 512, xpad=4)   # a row stride that is no multiple of 8
    go(4, 16, 512, wpad=12)


def test_skinny_linear_refusals(gpu):
    check_linear_refusals(_ops().skinny_linear, gpu)


# --------------------------------------------------------------------------- MXLLM_SKINNY_NC (latched per process)
NC_SHAPES = {2: 4096, 4: 8192}  # N % (16 nc) == 0 and N / (16 nc) >= 128: the kernel keeps the group count
NC_MK = [(5, 512), (20, 512), (5, 4608), (20, 4608)]


def run_nc_cases(nc, run, dev):
    for M, K in NC_MK:
        for kind in ("perm", "int"):
            check_linear(kind, M, NC_SHAPES[nc], K, run, dev)


@pytest.mark.parametrize("nc", [2, 4])
def test_skinny_linear_channel_groups(gpu, nc):
    """The two- and four-channel-group kernels, in a fresh process (the variable is read once)."""
    env = dict(os.environ, MXLLM_SKINNY_NC=str(nc))
    r = subprocess.run([sys.executable, "-m", "tests.test_skinny_exact_gpu", "--nc", str(nc)], env=env, cwd=ROOT,
                       timeout=120, capture_output=True, text=True)
    assert r.returncode == 0, f"MXLLM_SKINNY_NC={nc}:\n{r.stdout}\n{r.stderr}"
    assert f"nc {nc}: {2 * len(NC_MK)} cases exact" in r.stdout, r.stdout


# =========================================================================== SwiGLU epilogue
SWIGLU_CASES = [(M, F, K) for F in (8, 520, 1024) for K in (512, 4608) for M in (1, 16, 17, 32)]


def silu64(g):
    return g / (1.0 + torch.exp(-g))


def check_swiglu(M, F, K, run, dev, xpad=24, wpad=8):
    """g = x[m, pi(n)], u = x[m, pi(F + n)] exactly; y against fp64 silu(g) * u under SWIGLU_M."""
    x = finite_x(M, K, 3400 + 64 * M + F + K, extremes=False)
    pi = perm_map(2 * F, K)
    gu = select(x, pi).double()
    y = run(strided(x, xpad, 3, dev), strided(perm_weight(2 * F, K), wpad, 0, dev)).cpu()
    ref64 = silu64(gu[:, :F]) * gu[:, F:]
    assert_parity(y, ref64, P.SWIGLU_M, name=f"swiglu M{M} F{F} K{K}")
    return y, ref64


@pytest.mark.parametrize("M,F,K", SWIGLU_CASES)
def test_skinny_linear_swiglu_parity(gpu, M, F, K):
    check_swiglu(M, F, K, _ops().skinny_linear_swiglu, gpu)


# =========================================================================== RMSNorm prologue
NORM_N = 528
NORM_CASES = [(M, K, resid, sw) for K in (512, 2048, 2560, 8192) for M in (1, 2, 3, 4) for resid in (False, True)
              for sw in (False, True)]
EPS = 1e-5


def norm_inputs(M, K, resid):
    g = _gen(3500 + 64 * M + K + resid)
    h = (torch.randn(M, K, generator=g) * 2).to(BF16)
    d = torch.randn(M, K, generator=g).to(BF16) if resid else None
    gamma = (1.0 + 0.1 * torch.randn(K, generator=g)).to(BF16)
    hb = (h.float() + d.float()).to(BF16) if resid else h  # the new residual: one fp32 add, rounded
    xn64 = hb.double() * torch.rsqrt(hb.double().pow(2).mean(-1, keepdim=True) + EPS) * gamma.double()
    return h, d, gamma, hb, xn64


def check_norm_linear(M, K, resid, swiglu, run, dev, N=NORM_N, hpad=16, dpad=40, wpad=8):
    """``run(h, delta, gamma, eps, w, swiglu) -> (y, h_out)``.  y[m, n] is the normalised row element
    pi(n) (RMSNORM_Y against fp64), or silu(g) * u of two of them, each rounded to bf16 (SWIGLU_M)."""
    h, d, gamma, hb, xn64 = norm_inputs(M, K, resid)
    pi = perm_map(N, K)
    hd = strided(h, hpad, 2, dev)
    y, h_out = run(hd, strided(d, dpad, 1, dev) if resid else None, gamma.to(dev), EPS,
                   strided(perm_weight(N, K), wpad, 0, dev), swiglu)
    name = f"norm M{M} K{K} resid{resid} swiglu{swiglu}"
    if resid:
        assert_exact(bits(h_out.cpu()), bits(hb), f"{name}: h + delta")
    else:
        assert h_out.data_ptr() == hd.data_ptr()
    sel = xn64[:, pi]
    if swiglu:
        gu = sel.to(BF16).double()  # g and u are rounded to bf16 before the SwiGLU (skinny_gemm.hip SWO)
        F = N // 2
        assert_parity(y.cpu(), silu64(gu[:, :F]) * gu[:, F:], P.SWIGLU_M, name=name)
    else:
        assert_parity(y.cpu(), sel, P.RMSNORM_Y, name=name)


@pytest.mark.parametrize("M,K,resid,swiglu", NORM_CASES)
def test_skinny_norm_linear_parity(gpu, M, K, resid, swiglu):
    check_norm_linear(M, K, resid, swiglu, _ops().skinny_norm_linear, gpu)


def check_norm_refusals(run, dev):
    for M, K in ((5, 512), (4, 8704)):  # more than four rows; M * K > 32768
        h, gamma = gauss_x(M, K, 2), torch.ones(K, dtype=BF16)
        with pytest.raises(RuntimeError):
            run(h.to(dev), None, gamma.to(dev), EPS, perm_weight(16, K).to(dev), False)


def test_skinny_norm_linear_refusals(gpu):
    check_norm_refusals(_ops().skinny_norm_linear, gpu)


# =========================================================================== RoPE + KV-append epilogue
# (M, Hq, Hkv, K, norm, resid, paged, kind)
QKV_CASES = [(M, hq, hkv, 512, False, False, paged, "perm") for M in (1, 4, 5, 16) for hq, hkv in ((8, 2), (16, 1))
             for paged in (False, True)]
QKV_CASES += [(M, hq, hkv, 2560, True, resid, paged, "perm") for M in (1, 4) for hq, hkv in ((8, 2), (16, 1))
              for resid, paged in ((False, False), (True, True))]
QKV_CASES += [(5, 8, 2, 4608, False, False, True, "int"), (16, 16, 1, 4608, False, False, False, "perm")]
QKV_CASES += [(4, 8, 2, 8192, True, True, False, "perm"), (2, 16, 1, 4096, True, False, True, "perm")]  # nit >= UNR


def qkv_id(c):
    M, Hq, Hkv, K, norm, resid, paged, kind = c
    return f"M{M}-Hq{Hq}-Hkv{Hkv}-K{K}-{'norm' if norm else 'plain'}{'+resid' if resid else ''}-" \
           f"{'paged' if paged else 'contig'}-{kind}"


@functools.lru_cache(maxsize=4)
def small_layout(M, Hkv, paged):
    """The layout of the refusal tests: caches of 2 slots x 256 positions of random bits (the canary), rows on
    alternating slots at distinct positions (0 and 255 included); paged: the same pools as two blocks of 256."""
    g = _gen(3650 + 8 * M + Hkv + paged)
    mid = 1 + torch.randperm(254, generator=g)
    pos = torch.cat([torch.tensor([0]), mid[:max(M - 2, 0)], torch.tensor([255])])[:M].to(I32)
    shape = (2, Hkv, 256, 128)
    cos, sin = TD.ref.rope_tables(256, 128, TD.ROPE_THETA, None)
    return dict(kc=TD.random_bits_cache(g, shape), vc=TD.random_bits_cache(g, shape), pos=pos,
                slots=(torch.arange(M) % 2).to(I32), bt=torch.tensor([[1], [0]], dtype=I32) if paged else None,
                cos=cos, sin=sin)


def qkv_inputs(case, small=False):
    """(layout, h, delta, gamma, w, the bf16 projection the rotation starts from, h + delta)."""
    M, Hq, Hkv, K, norm, resid, paged, kind = case
    N = (Hq + 2 * Hkv) * 128
    g = _gen(3600 + 64 * M + Hq + K + paged)
    c = small_layout(M, Hkv, paged) if small else TD.append_layout(g, M, Hkv, 128, 300, paged, True)
    hb = None
    if norm:  # the projection selects from the bf16 rounding of the fp64 normalised row
        h, d, gamma, hb, xn64 = norm_inputs(M, K, resid)
        w = perm_weight(N, K)
        proj = xn64[:, perm_map(N, K)].to(BF16)
    elif kind == "int":
        h, d, gamma, w = int_x(M, K, 3601), None, None, int_weight(N, K)
        r64 = h.double() @ w.double().t()
        assert float((h.abs().double() @ w.abs().double().t()).max()) < EXACT_LIMIT
        proj = r64.to(F32).to(BF16)
    else:
        h, d, gamma, w = finite_x(M, K, 3602 + M, extremes=False), None, None, perm_weight(N, K)
        proj = select(h, perm_map(N, K))
    return c, h, d, gamma, w, proj, hb


def qkv_args(case, inp, dev, kc, vc, hpad=16, dpad=40, wpad=8):
    """The op's arguments by name, in its order, on ``dev``."""
    c, h, d, gamma, w = inp[:5]
    return dict(h=strided(h, hpad, 2, dev), delta=strided(d, dpad, 1, dev) if d is not None else None,
                gamma=TD._dev(gamma, dev), eps=EPS, w=strided(w, wpad, 0, dev), cos=c["cos"].to(dev),
                sin=c["sin"].to(dev), pos=c["pos"].to(dev), slots=c["slots"].to(dev), kc=kc, vc=vc, Hq=case[1],
                Hkv=case[2], bt=TD._dev(c["bt"], dev))


def check_qkv_rope(case, run, dev, small=False, **pads):
    """``run(h, delta, gamma, eps, w, cos, sin, pos, slots, kc, vc, Hq, Hkv, bt) -> (q, h_out)``."""
    M, Hq, Hkv, K, norm, resid, paged, kind = case
    inp = qkv_inputs(case, small)
    out = {}

    def go(kc, vc):
        q, out["h"] = run(*qkv_args(case, inp, dev, kc, vc, **pads).values())
        return q

    TD.check_append(qkv_id(case), inp[0], inp[5], Hq, Hkv, 128, go, dev)
    if norm and resid:
        assert_exact(bits(out["h"].cpu()), bits(inp[6]), f"{qkv_id(case)}: h + delta")


@pytest.mark.parametrize("case", QKV_CASES, ids=qkv_id)
def test_skinny_qkv_rope_whole_cache(gpu, case):
    check_qkv_rope(case, _ops().skinny_qkv_rope, gpu)


# =========================================================================== FP8 weights
def emittable_codes():
    """The 238 codes the quantiser can emit: exponent field != 0, without 0x7F / 0xFF (NaN)."""
    c = torch.arange(256)
    return c[((c & 0x78) != 0) & ((c & 0x7F) != 0x7F)].to(torch.uint8)


def decode_e4m3(q, scale):
    from mxllm.serve.quant import dequantize_e4m3

    return dequantize_e4m3(q, scale)


def check_w8_dequant(run, dev):
    """Every emittable code at every position of the 8-code group, scale 1 and power-of-two scales."""
    codes = emittable_codes()
    assert codes.numel() == 238
    row = torch.cat([codes, codes[:2]])  # 240 = 30 groups of 8
    q = torch.stack([row.roll(r) for r in range(8)] * 2).contiguous()
    for scale in (torch.ones(16), torch.exp2(torch.arange(16.0) - 8)):
        want = decode_e4m3(q, scale)
        assert torch.equal(want.to(BF16).float(), want)  # 4 significant bits times a power of two
        assert_exact(bits(run(q.to(dev), scale.to(dev)).cpu()), bits(want.to(BF16)), "w8_dequant")


def test_w8_dequant_every_code(gpu):
    check_w8_dequant(_ops().w8_dequant, gpu)


INT_CODES = torch.tensor([0x38, 0x40, 0x44, 0x48, 0xB8, 0xC0, 0xC4, 0xC8], dtype=torch.uint8)  # +-1, 2, 3, 4
# (M, N, K, MXLLM_W8_NC, the branch of mx_w8a16_gemm)
W8_CASES = [(1, 96, 512, "", "one group"), (16, 96, 4608, "", "one group"), (1, 1040, 4096, "", "one group"),
            (6, 8192, 512, "", "two groups (6..16 tokens)"), (4, 8192, 16384, "", "two groups (4 tokens, K >= 16384)"),
            (5, 4096, 4096, "2", "two groups forced"), (8, 8192, 512, "4", "four groups forced"),
            (16, 8192, 4608, "4", "four groups forced"), (17, 96, 512, "", "two token blocks"),
            (32, 1040, 4608, "", "two token blocks")]
W8_FALLBACK = [(5, 96, 768), (33, 96, 1024)]  # K % 512 != 0; more than 32 rows: dequantise + mm


def w8_id(c):
    return f"M{c[0]}-N{c[1]}-K{c[2]}-nc{c[3] or 'auto'}"


@functools.lru_cache(maxsize=1)
def w8_int_weight(N, K):
    q = INT_CODES[torch.randint(0, 8, (N, K), generator=_gen(3700 + N + K))]
    scale = torch.exp2((torch.arange(N) % 5 - 2).float())  # ties each output to its own scale element
    return q, scale


@functools.lru_cache(maxsize=1)
def w8_gauss_weight(N, K):
    """quantize_e4m3 of Gaussian rows (at most 1040 different ones, repeated down the channels: the
    integer case is the one that ties every output to its own channel)."""
    from mxllm.serve.quant import quantize_e4m3

    n = min(N, 1040)
    q, s = quantize_e4m3(torch.randn(n, K, generator=_gen(3800 + N + K)) * 0.02)
    reps = (N + n - 1) // n
    return q.repeat(reps, 1)[:N].contiguous(), s.repeat(reps)[:N].contiguous()


def w8_products(x, q, scale, chunk=1024, f32=True, f64=True):
    """(fp32, fp64) products of x with the reference-decoded weights, 1024 channels at a time."""
    y32, y64 = [], []
    for n0 in range(0, q.shape[0], chunk):
        wd = decode_e4m3(q[n0:n0 + chunk], scale[n0:n0 + chunk])
        if f32:
            y32.append(x.float() @ wd.t())
        if f64:
            y64.append(x.double() @ wd.double().t())
    return (torch.cat(y32, 1) if f32 else None), (torch.cat(y64, 1) if f64 else None)


def w8_case(kind, M, N, K):
    if kind == "int":
        q, scale = w8_int_weight(N, K)
        x = int_x(M, K, 3701 + M, lim=3)
        assert bool(((q & 0x7F) >= 0x38).all()) and bool(((q & 0x7F) <= 0x48).all())  # |code| in 1..4
        assert 4 * 3 * K * 4 < EXACT_LIMIT  # |w| <= 4, |x| <= 3, scale <= 4
    else:
        q, scale = w8_gauss_weight(N, K)
        x = gauss_x(M, K, 3801 + M)
    return x, q, scale


def check_w8_linear(kind, M, N, K, run, dev, xpad=24):
    """``run(x, q, scale) -> y``; x row-strided with NaN pads and NaN rows past M."""
    name = f"w8 {kind} M{M} N{N} K{K}"
    x, q, scale = w8_case(kind, M, N, K)
    if kind == "int":  # integers below 2^24 (asserted in w8_case): the fp32 product is the exact one
        r64 = w8_products(x, q, scale, f64=False)[0].double()
    else:
        r64 = w8_products(x, q, scale, f32=False)[1]
    y = run(strided(x, xpad, 3, dev), q.to(dev), scale.to(dev)).cpu()
    if kind == "int":
        assert_exact(bits(y), bits(r64.to(F32).to(BF16)), name)
    else:
        assert_parity(y, r64, P.W8_Y, name=name)
    return y, r64


def w8_fallback_products(x, q, scale):
    """The documented fallback: the weights dequantised to bf16 (one fp32 product code * scale, rounded),
    then a bf16 GEMM.  (fp32, fp64) products with those rounded weights."""
    wb = decode_e4m3(q, scale).to(BF16)
    return x.float() @ wb.float().t(), x.double() @ wb.double().t()


def check_w8_fallback(M, N, K, run, dequant, dev):
    """Shapes the decode kernel does not take: w8_dequant bitwise (any scale), then the bf16 GEMM of the
    ROUNDED weights per element -- against the unrounded ones the error is the weights' bf16 rounding
    (2^-9 each), far above W8_Y, and no defect."""
    x, q, scale = w8_case("gauss", M, N, K)
    assert M > 32 or K % 512
    assert_exact(bits(dequant(q.to(dev), scale.to(dev)).cpu()), bits(decode_e4m3(q, scale).to(BF16)), "w8_dequant")
    y = run(strided(x, 24, 3, dev), q.to(dev), scale.to(dev)).cpu()
    assert_parity(y, w8_fallback_products(x, q, scale)[1], P.W8_DEQ_Y, name=f"w8 fallback M{M} N{N} K{K}")
    return y


@pytest.mark.parametrize("kind", ["int", "gauss"])
@pytest.mark.parametrize("case", W8_CASES, ids=w8_id)
def test_w8_linear_every_branch(gpu, case, kind, monkeypatch):
    M, N, K, nc, _ = case
    monkeypatch.setenv("MXLLM_W8_NC", nc)
    check_w8_linear(kind, M, N, K, _ops().w8_linear, gpu)


@pytest.mark.parametrize("M,N,K", W8_FALLBACK)
def test_w8_linear_fallback_parity(gpu, M, N, K):
    check_w8_fallback(M, N, K, _ops().w8_linear, _ops().w8_dequant, gpu)


# --------------------------------------------------------------------------- quant_rows_e4m3
QUANT_K = (8, 2048, 2056)


def inv448_is_exact():
    """448 * fl(1 / 448) == 1 in fp32: then amax = 448 gives sc = 1, inv = 1 and the ties below are exact."""
    one = torch.tensor(448.0) * (torch.tensor(1.0) / torch.tensor(448.0))
    return one.item() == 1.0


def quant_rows_input(K):
    """Three rows: Gaussian with amax in the last column; all zero; e4m3 rounding ties with amax in the
    first column (x * inv exact: amax 448 when 448 * fl(1/448) == 1, else the amax whose inv is 2)."""
    g = _gen(3900 + K)
    x = (torch.randn(3, K, generator=g) * 3).to(BF16)
    x[0, K - 1] = 17.0
    x[1] = 0.0
    amax = 448.0 if inv448_is_exact() else 224.0
    ties = torch.tensor([1.0625, 1.1875, -1.0625, -1.1875, 17.0, 19.0, 0.001953125 * 1.5, 2.0 ** -10])
    x[2] = (ties[torch.randint(0, 8, (K,), generator=g)] * (amax / 448.0)).to(BF16)
    x[2, 0] = amax
    return x


def quant_rows_expected(x):
    """The kernel's fp32 expressions in PyTorch (fp32 division is correctly rounded on both sides)."""
    xf = x.float()
    sc = torch.maximum(xf.abs().amax(1, keepdim=True), torch.tensor(1e-12)) * (torch.tensor(1.0) / torch.tensor(448.0))
    inv = torch.tensor(1.0) / sc
    q = (xf * inv).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)  # RNE, saturating
    return q, sc


def check_quant_rows(K, run, dev):
    x = quant_rows_input(K)
    q, s = run(strided(x, 16, 1, dev, fill=3e38))  # fmaxf drops NaN: a finite giant shows a read past K
    want_q, want_s = quant_rows_expected(x)
    assert_exact(bits(s.cpu()), bits(want_s), f"quant_rows K{K}: scales")
    assert_exact(q.cpu(), want_q, f"quant_rows K{K}: codes")
    return want_q


@pytest.mark.parametrize("K", QUANT_K)
def test_quant_rows_e4m3_bitwise(gpu, K):
    check_quant_rows(K, _ops().quant_rows_e4m3, gpu)


# =========================================================================== the launchers' rules, one by one
# mx::sk_takes (csrc/kernels/skinny_args.h) through the six ops.  Per rule: one call just inside, which passes
# the op's exact check at that shape, and one just outside, which raises a RuntimeError naming the op
# (w8_linear: runs the documented dequantise + GEMM fallback) -- at the smallest shapes on either side: K 512
# against 768, N 16 against 24, the row limit against one more, (4, 8192) against (4, 8704) for the 64 KiB of
# LDS, a row pad of 8 against 4.  Then a valid call passes again.  Not reachable through an op: the rules
# on ldy (the op allocates y), rows shorter than K (a view's rows are as long as its width) and nsplit >= 1.
def run_sides(op, check, base, rules, run, dev):
    """Per (inside, outside) of ``rules``: ``check`` passes at the base with ``inside`` and raises, naming the op,
    with ``outside``; at the end the base passes again."""
    for inside, outside in rules:
        check(run=run, dev=dev, **dict(base, **inside))
        with pytest.raises(RuntimeError, match=op):
            check(run=run, dev=dev, **dict(base, **outside))
    check(run=run, dev=dev, **base)


PADS_XW = [(dict(xpad=8), dict(xpad=4)), (dict(wpad=8), dict(wpad=4))]


def check_rules_linear(run, dev):
    rules = [(dict(M=32), dict(M=33)), (dict(N=16), dict(N=24)), (dict(K=512), dict(K=768))] + PADS_XW
    run_sides("skinny_linear", check_linear, dict(kind="perm", M=4, N=16, K=512, xpad=8, wpad=8), rules, run, dev)


def check_rules_swiglu(run, dev):
    rules = [(dict(M=32), dict(M=33)), (dict(F=8), dict(F=12)), (dict(K=512), dict(K=768))] + PADS_XW
    run_sides("skinny_linear_swiglu", check_swiglu, dict(M=4, F=8, K=512, xpad=8, wpad=8), rules, run, dev)


PADS_HDW = [(dict(hpad=8), dict(hpad=4)), (dict(dpad=8), dict(dpad=4)), (dict(wpad=8), dict(wpad=4))]


def check_rules_norm(run, dev):
    rules = [(dict(M=4), dict(M=5)), (dict(K=8192), dict(K=8704)), (dict(N=16), dict(N=24)),
             (dict(N=16, swiglu=True), dict(N=24, swiglu=True)), (dict(K=512), dict(K=768))] + PADS_HDW
    base = dict(M=4, K=512, resid=True, swiglu=False, N=16, hpad=8, dpad=8, wpad=8)
    run_sides("skinny_norm_linear", check_norm_linear, base, rules, run, dev)


def check_qkv_refused(case, run, dev, match="skinny_qkv_rope", edit=None, **pads):
    """The call raises and leaves both caches -- random bits, the canary -- bitwise as they were."""
    inp = qkv_inputs(case, True)
    c = inp[0]
    kc, vc = c["kc"].to(dev, copy=True), c["vc"].to(dev, copy=True)
    a = qkv_args(case, inp, dev, kc, vc, **pads)
    if edit:
        edit(a)
    with pytest.raises(RuntimeError, match=match):
        run(*a.values())
    assert_exact(bits(kc.cpu()), bits(c["kc"]), f"{qkv_id(case)}: K cache after a refused call")
    assert_exact(bits(vc.cpu()), bits(c["vc"]), f"{qkv_id(case)}: V cache after a refused call")


def _qkv(M=4, K=512, norm=False, resid=False, paged=False):
    return (M, 2, 1, K, norm, resid, paged, "perm")  # Hq 2, Hkv 1


def check_rules_qkv(run, dev):
    pads = dict(hpad=8, dpad=8, wpad=8)
    nd = dict(norm=True, resid=True)
    for inside, outside, pin, pout in [
            (_qkv(M=16), _qkv(M=17), {}, {}),                                      # without the prologue
            (_qkv(M=4, **nd), _qkv(M=5, **nd), {}, {}),                            # with it
            (_qkv(K=8192, **nd), _qkv(K=8704, **nd), {}, {}),
            (_qkv(M=16, K=8704), None, {}, {}),                                    # no LDS bound without it
            (_qkv(K=512), _qkv(K=768), {}, {}), (_qkv(K=512, norm=True), _qkv(K=768, norm=True), {}, {}),
            (_qkv(), _qkv(), {}, dict(hpad=4)), (_qkv(), _qkv(), {}, dict(wpad=4)),
            (_qkv(**nd), _qkv(**nd), {}, dict(dpad=4))]:
        check_qkv_rope(inside, run, dev, small=True, **dict(pads, **pin))
        if outside is not None:
            check_qkv_refused(outside, run, dev, **dict(pads, **pout))
    # N = (Hq + 2 Hkv) * 128: the weight of two q-heads against Hq = 3
    check_qkv_refused(_qkv(), run, dev, edit=lambda a: a.update(Hq=3), **pads)
    check_qkv_rope(_qkv(**nd), run, dev, small=True, **pads)


def check_merge_rule(M, Hq, N, wpad, run, dev):
    """``run(ml, po, w) -> y``: the exact merge case of tests/test_decode_exact_gpu.py against the first N rows
    of the identity, y = the merged row's first N elements."""
    ml, po, ref64 = TD.merge_case(M, Hq, 1, True)
    w = torch.eye(N, Hq * 128, dtype=BF16)
    y = run(ml.to(dev), po.to(dev), strided(w, wpad, 0, dev)).cpu()
    assert_exact(bits(y), bits(ref64[:, :N].to(F32).to(BF16)), f"merge M{M} Hq{Hq} N{N} wpad{wpad}")


def check_rules_merge(run, dev):
    rules = [(dict(M=4), dict(M=5)), (dict(Hq=64), dict(Hq=68)), (dict(N=16), dict(N=24)), (dict(Hq=4), dict(Hq=6)),
             (dict(wpad=8), dict(wpad=4))]
    run_sides("skinny_merge_linear", check_merge_rule, dict(M=4, Hq=4, N=16, wpad=8), rules, run, dev)


def check_w8_outside(M, N, K, xpad, run, dev):
    """A call the fp8 kernel does not take: the fallback's GEMM of the bf16-rounded weights, per element."""
    x, q, scale = w8_case("gauss", M, N, K)
    y = run(strided(x, xpad, 3, dev), q.to(dev), scale.to(dev)).cpu()
    assert_parity(y, w8_fallback_products(x, q, scale)[1], P.W8_DEQ_Y, name=f"w8 fallback M{M} N{N} K{K} xpad{xpad}")


def check_rules_w8(run, dev):
    rules = [(dict(M=32), dict(M=33)), (dict(N=16), dict(N=24)), (dict(K=512), dict(K=768)), (dict(xpad=8), dict(xpad=4))]
    base = dict(M=4, N=16, K=512, xpad=8)
    for inside, outside in rules:
        check_w8_linear("int", run=run, dev=dev, **dict(base, **inside))
        check_w8_outside(run=run, dev=dev, **dict(base, **outside))
    check_w8_linear("int", run=run, dev=dev, **base)


RULE_CHECKS = dict(skinny_linear=check_rules_linear, skinny_linear_swiglu=check_rules_swiglu,
                   skinny_norm_linear=check_rules_norm, skinny_qkv_rope=check_rules_qkv,
                   skinny_merge_linear=check_rules_merge, w8_linear=check_rules_w8)


@pytest.mark.parametrize("op", RULE_CHECKS)
def test_refusals_by_rule(gpu, op):
    RULE_CHECKS[op](getattr(_ops(), op), gpu)


# --------------------------------------------------------------------------- skinny_qkv_rope's operands
def qkv_bad_operands(dev):
    """(case, the operand the message names, the edit of the valid arguments)."""
    other = torch.device("cpu") if dev.type == "cuda" else torch.device("meta")  # not the device of h

    def to(name, f):
        return lambda a: a.update({name: f(a[name])})

    return [("pos on another device", "pos", to("pos", lambda t: t.to(other))),
            ("pos int64", "pos", to("pos", lambda t: t.long())),
            ("pos a stride-2 view", "pos", to("pos", lambda t: torch.stack([t, t], 1)[:, 0])),
            ("pos of M + 1", "pos", to("pos", lambda t: torch.cat([t, t[:1]]))),
            ("slots on another device", "slots", to("slots", lambda t: t.to(other))),
            ("slots of M - 1", "slots", to("slots", lambda t: t[:-1])),
            ("cos on another device", "cos / sin", to("cos", lambda t: t.to(other))),
            ("cos of width 32", "cos / sin", to("cos", lambda t: t[:, :32].contiguous())),
            ("sin non-contiguous", "cos / sin", to("sin", lambda t: torch.cat([t, t], 1)[:, :64])),
            ("v_cache of another shape", "pools", to("vc", lambda t: torch.cat([t, t[:1]]))),
            ("k_cache 3-D", "pools", to("kc", lambda t: t[0])),
            ("head_dim 64", "pools", lambda a: a.update(kc=a["kc"][..., :64].contiguous(), vc=a["vc"][..., :64].contiguous())),
            ("block_table int64", "block_table", to("bt", lambda t: t.long())),
            ("gamma of K - 8", "gamma", to("gamma", lambda t: t[:-8])),
            ("delta of M + 1 rows", "delta", to("delta", lambda t: torch.cat([t, t[:1]])))]


def check_qkv_operands(run, dev):
    """Every operand check refuses before anything is written; then the valid call passes."""
    case = _qkv(norm=True, resid=True, paged=True)
    for name, match, edit in qkv_bad_operands(dev):
        check_qkv_refused(case, run, dev, match=match, edit=edit)
    check_qkv_rope(case, run, dev, small=True)


def test_skinny_qkv_rope_operand_checks(gpu):
    check_qkv_operands(_ops().skinny_qkv_rope, gpu)


# =========================================================================== yardstick
def measure():
    """fp32 ``x.float() @ w.float().t()`` against fp64 at the Gaussian inputs above: SKINNY_Y, W8_Y, W8_DEQ_Y."""
    from tests.test_rowwise_strict_gpu import _meas

    acc = {}
    for M, N, K in GAUSS_LIN_CASES:
        x, w, _, r64 = lin_expected("gauss", M, N, K)
        _meas(acc, "SKINNY_Y", x.float() @ w.float().t(), r64, BF16)
    for M, N, K in [c[:3] for c in W8_CASES]:
        x, q, scale = w8_case("gauss", M, N, K)
        _meas(acc, "W8_Y", *w8_products(x, q, scale), BF16)
    for M, N, K in W8_FALLBACK:
        x, q, scale = w8_case("gauss", M, N, K)
        _meas(acc, "W8_DEQ_Y", *w8_fallback_products(x, q, scale), BF16)
    return acc


def main(argv):
    if argv[:1] == ["--nc"]:
        nc = int(argv[1])
        assert os.environ.get("MXLLM_SKINNY_NC") == str(nc)
        try:
            run_nc_cases(nc, _ops().skinny_linear, torch.device("cuda", 0))
        except AssertionError as e:
            print(f"nc {nc}: {e}")
            return 1
        print(f"nc {nc}: {2 * len(NC_MK)} cases exact")
        return 0
    for name, (rel, ab) in sorted(measure().items()):
        print(f"{name}_MEASURED = ({rel:.3g}, {ab:.3g})")
    print(f"448 * fl(1 / 448) == 1 in fp32: {inv448_is_exact()}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
