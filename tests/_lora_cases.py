"""Cases, references and checks of the strict LoRA tests (tests/test_lora_strict_gpu.py on the GPU,
tests/test_lora_cases.py on the CPU).  Everything here is built on the CPU from fixed seeds; the check
functions take the tensors an implementation produced, so the CPU tests push reference implementations
(and deliberately corrupted tensors) through the very assertions the kernels meet.

A. ``swiglu_lora_kernel`` / ``swiglu_lora_reduce_kernel`` (csrc/kernels/lora.hip)
   The launcher picks the template arguments <BWD, NRB, RBW> and the split count CS from (bwd, nrb, T, F) and
   two environment variables; ``rbw_of`` / ``cs_of`` / ``split_ranges`` mirror it -- to choose and label
   cases only, no check reads them for a tolerance.  How TAIL_CASES was chosen:
     * base set: each of the 2 x 4 x 3 instantiations once at F = 640 (5 tiles) with 2 splits, so its two
       workgroups per row group run 2 and 3 trips (both LDS buffers, an uneven split, the prefetch of a
       next tile and the last trip's reload).  RBW 1 comes from T = 48 (request 4, three row blocks) or
       T = 16 (request 2), RBW 2 from T = 160 (request 4, ten row blocks) or T = 64 (request 2), RBW 4 from
       T = 64 (request 4); the pad alternates between 64 and 16 nrb.
     * extras, forward and backward: 1 tile; 3 tiles with the split count unset (clamped to 3 x 1 trip),
       1 (one workgroup, 3 trips), 2 (1 + 2); 5 tiles with 1 split (5 trips), 5 splits and unset; a
       request of 2 splits clamped to the single tile; requests 1 and 2 for RBW; two cases with gate
       values of magnitude 30..60 (the sigmoid saturated in both directions).
   Per case: the elementwise half bitwise the plain kernels', one-hot V rows (routing, exact), V rows with one
   non-zero per split (the reduce kernel adds every split once, exact), Gaussian V per element, twice the same bits.

B. The LoRA projection (FusedLinear -> lora_linear_aug -> _LoRAAugFn) and the LoRA MLP block
   (gate-up -> SwiGLU with tails -> down, as Llama._layer wires them) against plain fp64, with adapters
   at least as large as the base term (``term_rms``), so that a wrong adapter product cannot hide.
"""
from __future__ import annotations

import functools
import types
from collections import namedtuple

import torch
import torch.nn.functional as F_

from tests import _parity as P
from tests._parity import assert_exact, assert_parity

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
POISON = 64.0  # V rows past 16 nrb, V's columns past its width: any read of one shows
S_TAIL = 2.0   # a power of two: 2 x out is exact in bf16


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


# =========================================================================== A. launcher mirror
def rbw_of(T: int, req: int | None) -> int:
    """``swiglu_lora_rbw``: 16-row blocks per workgroup (default 2), clamped to divide T / 16."""
    rbw = 2 if req is None else req
    rbw = 4 if rbw >= 4 else (2 if rbw >= 2 else 1)
    while rbw > 1 and (T // 16) % rbw:
        rbw >>= 1
    return rbw


def cs_of(T: int, F: int, cs_req: int | None, rbw: int) -> int:
    """``swiglu_lora_splits``: the split count, clamped to the tile count (and 32)."""
    tiles, rbs = F // 128, T // (16 * rbw)
    cs = cs_req or 0
    if cs <= 0:
        cs = (512 + rbs - 1) // rbs
    return min(max(cs, 1), tiles, 32)


def split_ranges(tiles: int, cs: int):
    """[t0, t1) of every split, as the kernel computes them."""
    return [(sp * tiles // cs, (sp + 1) * tiles // cs) for sp in range(cs)]


TailCase = namedtuple("TailCase", "bwd nrb T F rbw_req cs_req pad sat")
# (T, requested row blocks) -> RBW after the launcher's clamp (three and ten row blocks fall back)
RBW_EXPECTED = {(16, 1): 1, (16, 2): 1, (16, 4): 1, (48, 1): 1, (48, 2): 1, (48, 4): 1,
                (64, 1): 1, (64, 2): 2, (64, 4): 4, (160, 1): 1, (160, 2): 2, (160, 4): 2}


def _tail_cases():
    cases = []
    for bwd in (False, True):
        for nrb in (1, 2, 3, 4):
            alt = (nrb + bwd) % 2
            for T, req in [((48, 4), (16, 2))[alt], ((160, 4), (64, 2))[alt], (64, 4)]:  # RBW 1, 2, 4
                cases.append(TailCase(bwd, nrb, T, 640, req, 2, 16 * nrb if alt else 64, False))
    for bwd in (False, True):
        cases += [TailCase(bwd, 1, 16, 128, 1, None, 64, False),
                  TailCase(bwd, 2, 48, 384, 2, None, 32, False),
                  TailCase(bwd, 3, 64, 384, 4, 1, 64, True),
                  TailCase(bwd, 4, 160, 384, 4, 2, 64, False),
                  TailCase(bwd, 2, 64, 640, 1, 1, 64, False),
                  TailCase(bwd, 3, 160, 640, 2, 5, 48, False),
                  TailCase(bwd, 4, 16, 640, None, None, 64, True),
                  TailCase(bwd, 1, 64, 128, 2, 2, 16, False)]
    return cases


TAIL_CASES = _tail_cases()


def tail_rbw(c):
    return rbw_of(c.T, c.rbw_req)


def tail_cs(c):
    return cs_of(c.T, c.F, c.cs_req, tail_rbw(c))


def tail_trips(c):
    """Trips of each workgroup of a row group."""
    return [t1 - t0 for t0, t1 in split_ranges(c.F // 128, tail_cs(c))]


def tail_id(c):
    cs = "x" if c.cs_req is None else c.cs_req
    return (f"{'bwd' if c.bwd else 'fwd'}-nrb{c.nrb}-rbw{tail_rbw(c)}-T{c.T}-F{c.F}-cs{cs}-pad{c.pad}"
            + ("-sat" if c.sat else ""))


def tail_env(c):
    """The two environment variables of the launcher (None: unset)."""
    return {"MXLLM_SWIGLU_LORA_RBW": None if c.rbw_req is None else str(c.rbw_req),
            "MXLLM_SWIGLU_LORA_CS": None if c.cs_req is None else str(c.cs_req)}


def tail_width(c):
    return 2 * c.F if c.bwd else c.F


@functools.lru_cache(maxsize=4)
def tail_inputs(c, kind="gauss"):
    """(gu [T, 2F], dm [T, F] or None) in bf16.  ``gauss``: N(0, 1.5) gates and ups (``sat``: every third
    gate column of magnitude 30..60, either sign); ``bounded``: gate in [1, 3], |up| and |dm| in [1, 2] --
    every |output| lies in 2^-1 .. 2^3, so a sum of a few of them is exact in fp32 in any order."""
    g = _gen(7000 + 977 * c.bwd + 131 * c.nrb + 7 * c.T + c.F + (0 if kind == "gauss" else 5))
    if kind == "gauss":
        gu = _randn(g, c.T, 2 * c.F, scale=1.5)
        if c.sat:
            big = (30.0 + 30.0 * torch.rand(c.T, (c.F + 2) // 3, generator=g))
            gu[:, 0:c.F:3] = big * (torch.randint(0, 2, big.shape, generator=g) * 2 - 1)
        dm = _randn(g, c.T, c.F)
    else:
        sign = lambda *s: (torch.randint(0, 2, s, generator=g) * 2 - 1).float()  # noqa: E731
        gate = 1.0 + 2.0 * torch.rand(c.T, c.F, generator=g)
        up = (1.0 + torch.rand(c.T, c.F, generator=g)) * sign(c.T, c.F)
        gu = torch.cat([gate, up], dim=1)
        dm = (1.0 + torch.rand(c.T, c.F, generator=g)) * sign(c.T, c.F)
    return gu.to(BF16), (dm.to(BF16) if c.bwd else None)


def _v_buffer(c, vals):
    """``vals`` [16 nrb, W] as the leading rows of a [16 nrb + 16, W + 24] buffer (padded row stride);
    the 16 further rows and the 24 further columns hold POISON."""
    R, W = vals.shape
    buf = torch.full((R + 16, W + 24), POISON, dtype=BF16)
    buf[:R, :W] = vals.to(BF16)
    return buf


@functools.lru_cache(maxsize=4)
def tail_v_gauss(c):
    """Gaussian V: every element of the buffer non-zero, the rows past 16 nrb included."""
    g = _gen(7100 + 31 * c.nrb + c.F + c.bwd)
    buf = _randn(g, 16 * c.nrb + 16, tail_width(c) + 24).to(BF16)
    assert bool((buf[16 * c.nrb:] != 0).all())
    return buf


NSHIFT = 3


def _route_offsets():
    """Start of every case's run of 8-column chunks: consecutive within the cases of one (bwd, F), so
    that together they visit every chunk of the width (asserted in tests/test_lora_cases.py)."""
    off, nxt = {}, {}
    for c in TAIL_CASES:
        key = (c.bwd, c.F)
        off[c] = nxt.get(key, 0)
        nxt[key] = off[c] + NSHIFT * 16 * c.nrb
    return off


ROUTE_OFFSET = _route_offsets()


def route_columns(c, k):
    """c_j of shift ``k``: row j selects column 8 q + (j + k) % 8 of chunk q = (offset + k R + j) mod W / 8.
    Chunk q is (tile q // 16, wave slice q % 16 // 4, lane group q % 4) of the dg half or, past F / 8, the
    du half."""
    R, nch = 16 * c.nrb, tail_width(c) // 8
    return [8 * ((ROUTE_OFFSET[c] + k * R + j) % nch) + (j + k) % 8 for j in range(R)]


def tail_v_onehot(c, k):
    cols = route_columns(c, k)
    vals = torch.zeros(len(cols), tail_width(c))
    vals[torch.arange(len(cols)), torch.tensor(cols)] = 1.0
    return _v_buffer(c, vals), cols


def tail_v_splits(c):
    """One non-zero (1, -1 or 2) of every V row in every split: row j, split sp -> a column of tile
    t0 + (j mod trips) of that split (backward: alternately of the dg and the du half).  Returns the buffer
    and the dense [16 nrb, W] values."""
    R, W = 16 * c.nrb, tail_width(c)
    vals = torch.zeros(R, W)
    for sp, (t0, t1) in enumerate(split_ranges(c.F // 128, tail_cs(c))):
        for j in range(R):
            col = 128 * (t0 + j % (t1 - t0)) + (37 * j + 11 * sp) % 128
            if c.bwd and (j + sp) % 2:
                col += c.F
            vals[j, col] = (1.0, -1.0, 2.0)[(j + sp) % 3]
    return _v_buffer(c, vals), vals


def exact_sum_ok(terms: torch.Tensor) -> bool:
    """Whether sum(terms, -1) is exact in fp32 in ANY order: every term is a multiple of the ulp (8-bit
    significand) of the smallest non-zero one, and sum |terms| stays below 2^24 of those ulps."""
    t = terms.double().abs()
    tmin = torch.where(t > 0, t, torch.full_like(t, float("inf"))).amin(-1)
    ulp = torch.exp2(torch.floor(torch.log2(tmin)) - 7)
    return bool((t.sum(-1) / ulp < 2.0 ** 24).all())


def swiglu_plain_ref(dm, gu):
    """The plain SwiGLU of mxllm/ops/reference.py in fp32 (forward, or its autograd), rounded to bf16."""
    F = gu.shape[1] // 2
    x = gu.float().requires_grad_(dm is not None)
    m = F_.silu(x[:, :F]) * x[:, F:]
    if dm is None:
        return m.detach().to(BF16)
    m.backward(dm.float())
    return x.grad.to(BF16)


def tail_takes(dm, gu, pad, v, nrb, dev) -> bool:
    """The operand contract of the ``swiglu_lora`` op (csrc/bindings.cpp), for the reference implementation."""
    ts = [gu, v] + ([dm] if dm is not None else [])
    if any(t.dtype != BF16 or t.device.type != torch.device(dev).type for t in ts):
        return False
    if gu.dim() != 2 or not gu.is_contiguous() or gu.shape[1] == 0 or gu.shape[1] % 256 or gu.shape[0] % 16:
        return False
    if v.dim() != 2 or v.stride(1) != 1 or v.stride(0) < v.shape[1] or v.stride(0) % 8:
        return False
    T, F = gu.shape[0], gu.shape[1] // 2
    if not 1 <= nrb <= 4 or pad < 16 * nrb or pad % 8:
        return False
    if v.shape[0] < 16 * nrb or v.shape[1] != (2 * F if dm is not None else F):
        return False
    return dm is None or (dm.is_contiguous() and dm.numel() == T * F)


def ref_swiglu_lora(dm, gu, pad, v, nrb, s):
    """The op's contract in plain PyTorch: the whole [T, W + pad] buffer, or RuntimeError."""
    if not tail_takes(dm, gu, pad, v, nrb, gu.device):
        raise RuntimeError("swiglu_lora: operands refused")
    out = swiglu_plain_ref(dm, gu)
    full = torch.zeros(out.shape[0], out.shape[1] + pad, dtype=BF16)
    full[:, :out.shape[1]] = out
    full[:, out.shape[1]:out.shape[1] + 16 * nrb] = (s * (out.float() @ v[:16 * nrb].float().t())).to(BF16)
    return full


# --------------------------------------------------------------------------- A. the checks
def check_tail_zero(tail, R, name):
    assert_exact(tail[:, R:], torch.zeros_like(tail[:, R:]), f"{name}: pad columns past 16 nrb")


def check_tail_routing(tail, out, cols, name):
    """One-hot V rows, s = 2: tail[t, j] == bf16(2 out[t, c_j]), whatever the summation order."""
    R = len(cols)
    want = (S_TAIL * out[:, torch.as_tensor(cols, device=out.device)].float()).to(BF16)
    assert_exact(tail[:, :R], want, f"{name}: one-hot routing")
    check_tail_zero(tail, R, name)


def check_tail_splits(tail, out, vals, name):
    """One non-zero per split: the fp32 sum is exact (asserted), so tail == bf16(2 sum) bit for bit."""
    R = vals.shape[0]
    v = vals.to(out.device).double()
    idx = v.abs().argsort(dim=1, descending=True)[:, :int((v != 0).sum(1).max())]  # the non-zero columns
    terms = out.double()[:, idx] * v.gather(1, idx)  # [T, R, n]
    assert exact_sum_ok(terms), f"{name}: the chosen sums are not exact in fp32"
    ref = S_TAIL * terms.sum(-1)
    want = ref.to(F32)
    assert torch.equal(want.double(), ref)
    assert_exact(tail[:, :R], want.to(BF16), f"{name}: one non-zero per split")
    check_tail_zero(tail, R, name)


def check_tail_parity(tail, out, v, R, name):
    """Gaussian V: every element against the fp64 product of the implementation's own bf16 output."""
    ref = S_TAIL * (out.double() @ v[:R].double().t())
    assert_parity(tail[:, :R], ref, P.SWIGLU_LORA_TAIL, scale="row", name=f"{name}: tail")
    check_tail_zero(tail, R, name)


def check_tail_case(c, run, plain, dev):
    """``run(dm, gu, pad, v, nrb, s)`` -> the whole [T, W + pad] buffer; ``plain(dm, gu)`` -> the plain
    SwiGLU kernels' [T, W] output."""
    name, W, R = tail_id(c), tail_width(c), 16 * c.nrb
    gu, dm = [None if t is None else t.to(dev) for t in tail_inputs(c)]
    vb = tail_v_gauss(c).to(dev)
    full = run(dm, gu, c.pad, vb[:, :W], c.nrb, S_TAIL)
    assert tuple(full.shape) == (c.T, W + c.pad), name
    out, tail = full[:, :W], full[:, W:]
    assert_exact(out, plain(dm, gu), f"{name}: elementwise half")
    check_tail_parity(tail, out, vb[:, :W], R, name)
    assert_exact(run(dm, gu, c.pad, vb[:, :W], c.nrb, S_TAIL), full, f"{name}: second call")
    for k in range(NSHIFT):
        vh, cols = tail_v_onehot(c, k)
        fk = run(dm, gu, c.pad, vh.to(dev)[:, :W], c.nrb, S_TAIL)
        assert_exact(fk[:, :W], out, f"{name}: elementwise half (shift {k})")
        check_tail_routing(fk[:, W:], out, cols, f"{name} shift {k}")
    gub, dmb = [None if t is None else t.to(dev) for t in tail_inputs(c, "bounded")]
    vs, vals = tail_v_splits(c)
    fs = run(dmb, gub, c.pad, vs.to(dev)[:, :W], c.nrb, S_TAIL)
    assert_exact(fs[:, :W], plain(dmb, gub), f"{name}: elementwise half (bounded inputs)")
    check_tail_splits(fs[:, W:], fs[:, :W], vals, name)
    assert torch.equal(vb, tail_v_gauss(c).to(dev)) and torch.equal(gu, tail_inputs(c)[0].to(dev)), \
        f"{name}: an operand was written"


# --------------------------------------------------------------------------- A. refusals
def _refusal_base(dev, bwd):
    T, F = 16, 128
    g = _gen(7300 + bwd)
    W = 2 * F if bwd else F
    return dict(dm=_randn(g, T, F).to(BF16).to(dev) if bwd else None, gu=_randn(g, T, 2 * F).to(BF16).to(dev),
                pad=64, v=_randn(g, 80, W + 24).to(BF16).to(dev)[:, :W], nrb=1)


def _bf(dev, *shape):
    return torch.ones(*shape, dtype=BF16, device=dev)


def _rows(dev, rows, width, stride=None):
    return _bf(dev, rows, stride or width + 24)[:, :width]


# id -> (backward?, the operands to replace); ``gpu_only``: the operand lives on the other device
REFUSALS = {
    "T-not-16": (False, lambda d: dict(gu=_bf(d, 24, 256))),
    "T-not-16-bwd": (True, lambda d: dict(gu=_bf(d, 24, 256), dm=_bf(d, 24, 128))),
    "F-not-128": (False, lambda d: dict(gu=_bf(d, 16, 128), v=_rows(d, 80, 64))),
    "F-not-128-bwd": (True, lambda d: dict(gu=_bf(d, 16, 384), dm=_bf(d, 16, 192), v=_rows(d, 80, 384))),
    "gu-odd-width": (False, lambda d: dict(gu=_bf(d, 16, 257))),
    "gu-odd-width-bwd": (True, lambda d: dict(gu=_bf(d, 16, 257), v=_rows(d, 80, 257))),
    "gu-odd-width-513": (False, lambda d: dict(gu=_bf(d, 16, 513), v=_rows(d, 80, 256))),
    "gu-zero-width": (False, lambda d: dict(gu=_bf(d, 16, 0), v=_rows(d, 80, 0))),
    "gu-3d": (False, lambda d: dict(gu=_bf(d, 1, 16, 256))),
    "gu-row-strided": (False, lambda d: dict(gu=_bf(d, 16, 264)[:, :256])),
    "nrb-0": (False, lambda d: dict(nrb=0)),
    "nrb-5": (False, lambda d: dict(nrb=5, pad=80)),
    "nrb-5-bwd": (True, lambda d: dict(nrb=5, pad=80)),
    "pad-below-16nrb": (False, lambda d: dict(nrb=2, pad=16)),
    "pad-not-8": (False, lambda d: dict(pad=20)),
    "pad-not-8-bwd": (True, lambda d: dict(pad=60, nrb=3)),
    "v-too-few-rows": (False, lambda d: dict(v=_rows(d, 8, 128))),
    "v-too-few-rows-nrb4": (True, lambda d: dict(v=_rows(d, 48, 256), nrb=4)),
    "v-wrong-width-fwd": (False, lambda d: dict(v=_rows(d, 80, 256))),
    "v-wrong-width-bwd": (True, lambda d: dict(v=_rows(d, 80, 128))),
    "v-row-stride-not-8": (False, lambda d: dict(v=_rows(d, 80, 128, 132))),
    "v-row-stride-not-8-bwd": (True, lambda d: dict(v=_rows(d, 80, 256, 260))),
    "v-1d": (False, lambda d: dict(v=_bf(d, 128 * 80))),
    "dm-wrong-size": (True, lambda d: dict(dm=_bf(d, 16, 120))),
    "dm-too-many-rows": (True, lambda d: dict(dm=_bf(d, 32, 128))),
    "gu-fp16": (False, lambda d: dict(gu=_bf(d, 16, 256).to(torch.float16))),
    "gu-fp32-bwd": (True, lambda d: dict(gu=_bf(d, 16, 256).float())),
    "v-fp32": (False, lambda d: dict(v=_rows(d, 80, 128).float())),
    "dm-fp32": (True, lambda d: dict(dm=_bf(d, 16, 128).float())),
    "gu-on-cpu": (False, lambda d: dict(gu=_bf("cpu", 16, 256))),
    "v-on-cpu": (False, lambda d: dict(v=_rows("cpu", 80, 128))),
    "dm-on-cpu": (True, lambda d: dict(dm=_bf("cpu", 16, 128))),
}
GPU_ONLY_REFUSALS = ("gu-on-cpu", "v-on-cpu", "dm-on-cpu")


def check_tail_refusal(rid, run, dev, raises):
    """The base operands are taken; with the operands of ``rid`` replaced the call raises and no operand
    changed.  (The op allocates its own output: there is no output to compare.)"""
    bwd, change = REFUSALS[rid]
    base = _refusal_base(dev, bwd)
    full = run(base["dm"], base["gu"], base["pad"], base["v"], base["nrb"], S_TAIL)
    assert tuple(full.shape) == (16, (256 if bwd else 128) + 64)
    args = dict(base, **change(dev))
    before = {k: t.clone() for k, t in args.items() if isinstance(t, torch.Tensor)}
    with raises(RuntimeError):
        run(args["dm"], args["gu"], args["pad"], args["v"], args["nrb"], S_TAIL)
    for k, t in before.items():
        assert torch.equal(args[k], t), f"{rid}: refused but {k} changed"


# =========================================================================== B. the projection
S_LORA = 2.0  # lora_alpha = 2 r: with the operand sizes below the adapter term has twice the base term's rms
ProjCase = namedtuple("ProjCase", "T K splits r wzero")
PROJ_CASES = [ProjCase(128, 256, (256, 128, 128), 16, False),  # R = 48 of a 64-column pad
              ProjCase(192, 256, (192,), 32, False),            # R = 32 of 64
              ProjCase(128, 256, (128, 128), 32, False),        # R = 64 = pad
              ProjCase(192, 256, (256,), 64, False),            # R = 64 = pad, one split
              ProjCase(48, 256, (128, 128), 32, False),         # T % 64: _lora_native declines, hipBLASLt products
              ProjCase(128, 256, (192,), 32, True)]             # W = 0: y and dx are the adapter terms alone
# (K, splits, r) of tests/test_mfma_exact_gpu.py ``grads_case`` whose last split's rank blocks end with the
# 64-column tail: lora_grads (csrc/bindings.cpp) launches them as one-block problems
GRADS_TAIL_END_CONFIGS = [(256, (128, 128), 32), (320, (192, 64), 32)]
LAYOUTS = ("row", "image", "tr")  # row-major (dX NN), row-major + dx_image (wxt, TN), transposed (wa, NN / TN)


def proj_id(c):
    return f"T{c.T}-K{c.K}-N{'+'.join(map(str, c.splits))}-r{c.r}" + ("-W0" if c.wzero else "")


def block_mask(splits, r):
    m = torch.zeros(sum(splits), len(splits) * r, dtype=torch.bool)
    off = 0
    for i, n in enumerate(splits):
        m[off:off + n, i * r:(i + 1) * r] = True
        off += n
    return m


def _adapters(g, K, splits, r):
    N, R = sum(splits), len(splits) * r
    a = _randn(g, R, K, scale=K ** -0.5).to(BF16)
    b = (_randn(g, N, R, scale=r ** -0.5) * block_mask(splits, r)).to(BF16)
    return a, b


@functools.lru_cache(maxsize=8)
def proj_case(c):
    """x, dy ~ N(0, 1); W, A ~ N(0, 1 / K), the diagonal blocks of B ~ N(0, 1 / r): x W^T, x A^T and
    (x A^T) B^T all have rms ~ 1, the adapter term s = 2 of it.  ``a1`` / ``b1``: the adapters after an update;
    ``ga0`` / ``gb0``: what the flat gradient buffers hold before an accumulating backward."""
    g = _gen(8000 + c.T + 3 * sum(c.splits) + 7 * c.r + c.wzero)
    N, R = sum(c.splits), len(c.splits) * c.r
    w = torch.zeros(N, c.K, dtype=BF16) if c.wzero else _randn(g, N, c.K, scale=c.K ** -0.5).to(BF16)
    a0, b0 = _adapters(g, c.K, c.splits, c.r)
    a1, b1 = _adapters(g, c.K, c.splits, c.r)
    return dict(x=_randn(g, c.T, c.K).to(BF16), dy=_randn(g, c.T, N).to(BF16), w=w, a0=a0, b0=b0, a1=a1, b1=b1,
                ga0=_randn(g, R, c.K, scale=4.0).to(BF16), gb0=_randn(g, N, R, scale=4.0).to(BF16))


def rms(t):
    return float(t.double().pow(2).mean().sqrt())


def term_rms(x, w, a, b, dy, s):
    """rms of (x W^T, s (x A^T) B^T, dy W, s (dy B) A) in fp64."""
    x, w, a, b, dy = [t.double() for t in (x, w, a, b, dy)]
    return rms(x @ w.t()), rms(s * (x @ a.t()) @ b.t()), rms(dy @ w), rms(s * (dy @ b) @ a)


def _blocks(splits, r):
    off = 0
    for i, n in enumerate(splits):
        yield slice(off, off + n), slice(i * r, (i + 1) * r)
        off += n


def proj_ref64(x, w, a, b, dy, s, splits, r):
    """Plain fp64, no intermediate rounding: y, dx, dA and the diagonal dB_i."""
    x, w, a, b, dy = [t.double() for t in (x, w, a, b, dy)]
    t, g = s * (x @ a.t()), s * (dy @ b)
    y = x @ w.t() + t @ b.t()
    dx = dy @ w + g @ a
    return y, dx, g.t() @ x, [dy[:, rows].t() @ t[:, cols] for rows, cols in _blocks(splits, r)]


def proj_fwd_model(x, w, a, b, s):
    """fp32 with the documented bf16 rounding of the stored tail t = s x A^T: (y before its rounding, t)."""
    t = (s * (x.float() @ a.float().t())).to(BF16)
    return torch.cat([x.float(), t.float()], 1) @ torch.cat([w.float(), b.float()], 1).t(), t


def proj_bwd_model(dy, x, t, w, a, b, s, splits, r, ga0=None, gb0=None):
    """fp32 with the documented bf16 rounding of g = s dy B: (dx, dA, [dB_i]) before their rounding."""
    g = (s * (dy.float() @ b.float())).to(BF16)
    dx = torch.cat([dy.float(), g.float()], 1) @ torch.cat([w.float(), a.float()], 0)
    da = g.float().t() @ x.float() + (0.0 if ga0 is None else ga0.float())
    db = [dy[:, rows].float().t() @ t[:, cols].float() + (0.0 if gb0 is None else gb0[rows, cols].float())
          for rows, cols in _blocks(splits, r)]
    return dx, da, db


def build_linear(K, splits, r, layout, dev, w, a, b):
    """A frozen-base LoRA FusedLinear in ``layout`` holding (w, a, b): the adapter copies and the images are
    made by the module's own ``sync_adapter_`` / ``refresh_images_``."""
    from mxllm.models.llama import FusedLinear

    lin = FusedLinear(K, list(splits), dtype=BF16, device=dev, lora_r=r, lora_alpha=S_LORA * r, train_base=False,
                      dx_image=layout == "image", transposed=layout == "tr")
    assert lin.scaling == S_LORA and lin.pad == (len(splits) * r + 63) // 64 * 64
    assert lin.transposed == (layout == "tr") and hasattr(lin, "wxt") == (layout == "image")
    with torch.no_grad():
        lin.weight.copy_(w.to(dev))
        set_adapters(lin, a, b)
        lin.refresh_images_()
    assert lin.augmented()
    return lin


def set_adapters(lin, a, b):
    """An optimizer step's effect: new adapter values, then the module's own sync."""
    with torch.no_grad():
        lin.lora_a.copy_(a.to(lin.lora_a.device))
        lin.lora_b.copy_(b.to(lin.lora_b.device))
    lin.sync_adapter_()


def attach_grads(lin, ga0, gb0):
    """Pre-attached flat gradient buffers (mxllm/parallel/grad_ready.py) and a ``mark_ready`` recorder."""
    dev, calls = lin.lora_a.device, []
    lin.lora_a.grad, lin.lora_b.grad = ga0.to(dev).clone(), gb0.to(dev).clone()
    for p in (lin.lora_a, lin.lora_b):
        p._mx_on_grad_ready = calls.append
    return calls


def run_projection(lin, x, dy, dev):
    """One forward and backward of the module: (y, dx, dA, dB) with dA / dB read from ``.grad``."""
    xg = x.to(dev).clone().requires_grad_(True)
    y = lin(xg)
    y.backward(dy.to(dev))
    return y.detach(), xg.grad, lin.lora_a.grad, lin.lora_b.grad


def check_proj_outputs(outs, ref, splits, r, name, gb0=None, ga0=None, bounds=None):
    """Every element of y, dx, dA and the diagonal dB_i against fp64 (``ref`` of proj_ref64, the start values
    of an accumulating backward added); the off-diagonal blocks of dB exactly zero or exactly ``gb0``."""
    y, dx, da, db = outs
    by, bdx, bda, bdb = bounds or (P.LORA_PROJ_Y, P.LORA_PROJ_DX, P.LORA_PROJ_DA, P.LORA_PROJ_DB)
    dev = y.device
    ry, rdx, rda, rdb = ref
    assert y.dtype == dx.dtype == da.dtype == db.dtype == BF16, name
    assert_parity(y, ry.to(dev), by, scale="row", name=f"{name}: y")
    assert_parity(dx, rdx.to(dev), bdx, scale="row", name=f"{name}: dx")
    assert_parity(da, (rda + (0.0 if ga0 is None else ga0.double())).to(dev), bda, scale="row", name=f"{name}: dA")
    for i, (rows, cols) in enumerate(_blocks(splits, r)):
        want = rdb[i] + (0.0 if gb0 is None else gb0[rows, cols].double())
        assert_parity(db[rows, cols], want.to(dev), bdb, scale="row", name=f"{name}: dB_{i}")
    off = ~block_mask(splits, r).to(dev)
    start = torch.zeros_like(db) if gb0 is None else gb0.to(dev)
    assert_exact(torch.where(off, db, torch.zeros_like(db)), torch.where(off, start, torch.zeros_like(db)),
                 f"{name}: off-diagonal blocks of dB ({'untouched' if gb0 is not None else 'zero'})")


def check_projection(c, layout, acc, dev, update=False):
    """FusedLinear in ``layout`` on ``dev``; ``acc``: gradients accumulated into pre-attached buffers holding
    ga0 / gb0, ``mark_ready`` once per adapter; ``update``: one step with (a0, b0), then the adapters
    change to (a1, b1), ``sync_adapter_()`` only, and the second step is the one compared."""
    d = proj_case(c)
    name = f"{proj_id(c)} {layout}{' acc' if acc else ''}{' after update' if update else ''}"
    lin = build_linear(c.K, c.splits, c.r, layout, dev, d["w"], d["a0"], d["b0"])
    a, b = d["a0"], d["b0"]
    if update:
        run_projection(lin, d["x"], d["dy"], dev)
        lin.lora_a.grad = lin.lora_b.grad = None
        a, b = d["a1"], d["b1"]
        set_adapters(lin, a, b)
    calls = attach_grads(lin, d["ga0"], d["gb0"]) if acc else None
    outs = run_projection(lin, d["x"], d["dy"], dev)
    ref = proj_ref64(d["x"], d["w"], a, b, d["dy"], S_LORA, c.splits, c.r)
    check_proj_outputs(outs, ref, c.splits, c.r, name, d["gb0"] if acc else None, d["ga0"] if acc else None)
    if acc:
        assert len(calls) == 2 and {id(p) for p in calls} == {id(lin.lora_a), id(lin.lora_b)}, \
            f"{name}: mark_ready fired {len(calls)} times"
    return lin


# =========================================================================== B. the MLP block
MlpCase = namedtuple("MlpCase", "T H F r")
MLP_CASES = [MlpCase(128, 256, 384, 16), MlpCase(192, 256, 128, 32)]  # R: gate-up 32 / down 16; 64 / 32


def mlp_id(c):
    return f"T{c.T}-H{c.H}-F{c.F}-r{c.r}"


@functools.lru_cache(maxsize=2)
def mlp_case(c):
    g = _gen(9000 + c.T + c.F + c.r)
    agu, bgu = _adapters(g, c.H, (c.F, c.F), c.r)
    ad, bd = _adapters(g, c.F, (c.H,), c.r)
    return dict(x=_randn(g, c.T, c.H).to(BF16), dy=_randn(g, c.T, c.H).to(BF16),
                wgu=_randn(g, 2 * c.F, c.H, scale=c.H ** -0.5).to(BF16), agu=agu, bgu=bgu,
                wd=_randn(g, c.H, c.F, scale=c.F ** -0.5).to(BF16), ad=ad, bd=bd)


def mlp_ref64(c):
    """fp64 autograd of the plain formula: y, dx, dA_gu, [dB_gu,i], dA_d, [dB_d]."""
    d = mlp_case(c)
    x, wgu, agu, bgu, wd, ad, bd, dy = [d[k].double() for k in ("x", "wgu", "agu", "bgu", "wd", "ad", "bd", "dy")]
    leaves = [t.requires_grad_(True) for t in (x, agu, bgu, ad, bd)]
    x, agu, bgu, ad, bd = leaves
    gu = x @ wgu.t() + S_LORA * (x @ agu.t()) @ bgu.t()
    m = F_.silu(gu[:, :c.F]) * gu[:, c.F:]
    y = m @ wd.t() + S_LORA * (m @ ad.t()) @ bd.t()
    dx, dagu, dbgu, dad, dbd = torch.autograd.grad(y, leaves, dy)
    return (y.detach(), dx, dagu, [dbgu[rows, cols] for rows, cols in _blocks((c.F, c.F), c.r)], dad,
            [dbd[rows, cols] for rows, cols in _blocks((c.H,), c.r)])


def swiglu_ref64(gu, dm):
    F = gu.shape[1] // 2
    g, u, d = gu[:, :F].double(), gu[:, F:].double(), dm.double()
    s = torch.sigmoid(g)
    return g * s * u, torch.cat([d * u * s * (1 + g * (1 - s)), d * g * s], dim=1)


def mlp_ref64_chained(c):
    """The same block from the closed forms (proj_ref64, swiglu_ref64): the independent formulation."""
    d = mlp_case(c)
    x, dy = d["x"].double(), d["dy"].double()
    gu = proj_ref64(x, d["wgu"], d["agu"], d["bgu"], torch.zeros(c.T, 2 * c.F), S_LORA, (c.F, c.F), c.r)[0]
    m = swiglu_ref64(gu, torch.zeros(c.T, c.F))[0]
    y, dm, dad, dbd = proj_ref64(m, d["wd"], d["ad"], d["bd"], dy, S_LORA, (c.H,), c.r)
    dgu = swiglu_ref64(gu, dm)[1]
    _, dx, dagu, dbgu = proj_ref64(x, d["wgu"], d["agu"], d["bgu"], dgu, S_LORA, (c.F, c.F), c.r)
    return y, dx, dagu, dbgu, dad, dbd


def mlp_model(c):
    """The fp32 model: the projection models above chained, every tensor that crosses an op boundary
    (gu, m, dm, dgu) rounded to bf16 as the ops store it.  Same tuple as mlp_ref64, before the output rounding."""
    d = mlp_case(c)
    gu32, tgu = proj_fwd_model(d["x"], d["wgu"], d["agu"], d["bgu"], S_LORA)
    gu = gu32.to(BF16)
    m = swiglu_plain_ref(None, gu)
    y32, td = proj_fwd_model(m, d["wd"], d["ad"], d["bd"], S_LORA)
    dm32, dad, dbd = proj_bwd_model(d["dy"], m, td, d["wd"], d["ad"], d["bd"], S_LORA, (c.H,), c.r)
    dgu = swiglu_plain_ref(dm32.to(BF16), gu)
    dx32, dagu, dbgu = proj_bwd_model(dgu, d["x"], tgu, d["wgu"], d["agu"], d["bgu"], S_LORA, (c.F, c.F), c.r)
    return y32, dx32, dagu, dbgu, dad, dbd


def run_mlp(c, dev):
    """gate-up -> SwiGLU -> down on ``dev`` exactly as Llama._layer wires them (its own ``_swiglu_tails``
    decides which tails the SwiGLU pass writes): ((y, dx, dA_gu, dB_gu, dA_d, dB_d), wrote the tails?)."""
    from mxllm import ops
    from mxllm.models.llama import Llama

    d = mlp_case(c)
    wgu = build_linear(c.H, (c.F, c.F), c.r, "row", dev, d["wgu"], d["agu"], d["bgu"])
    wd = build_linear(c.F, (c.H,), c.r, "image", dev, d["wd"], d["ad"], d["bd"])
    layer = types.SimpleNamespace(wgu=wgu, wd=wd)
    xg = d["x"].to(dev).clone().requires_grad_(True)
    tf, tb = Llama._swiglu_tails(types.SimpleNamespace(cfg=types.SimpleNamespace(ffn=c.F)), layer, xg)
    m = ops.swiglu(wgu(xg, dy_tail=tb is not None), out_pad=Llama._pad(wd), grad_pad=Llama._pad(wgu), tail_fwd=tf,
                   tail_bwd=tb)
    y = wd(m, x_tail=tf is not None)
    y.backward(d["dy"].to(dev))
    return (y.detach(), xg.grad, wgu.lora_a.grad, wgu.lora_b.grad, wd.lora_a.grad, wd.lora_b.grad), \
        (tf is not None, tb is not None)


def check_mlp_outputs(c, outs, name):
    y, dx, dagu, dbgu, dad, dbd = outs
    ry, rdx, rdagu, rdbgu, rdad, rdbd = mlp_ref64(c)
    dev = y.device
    assert_parity(y, ry.to(dev), P.LORA_MLP_Y, scale="row", name=f"{name}: y")
    assert_parity(dx, rdx.to(dev), P.LORA_MLP_DX, scale="row", name=f"{name}: dx")
    for tag, da, rda, db, rdb, splits in (("gate-up", dagu, rdagu, dbgu, rdbgu, (c.F, c.F)),
                                          ("down", dad, rdad, dbd, rdbd, (c.H,))):
        assert_parity(da, rda.to(dev), P.LORA_MLP_DA, scale="row", name=f"{name}: {tag} dA")
        for i, (rows, cols) in enumerate(_blocks(splits, c.r)):
            assert_parity(db[rows, cols], rdb[i].to(dev), P.LORA_MLP_DB, scale="row", name=f"{name}: {tag} dB_{i}")
        off = ~block_mask(splits, c.r).to(dev)
        assert_exact(torch.where(off, db, torch.zeros_like(db)), torch.zeros_like(db),
                     f"{name}: {tag} off-diagonal blocks of dB")


# =========================================================================== the measurements
def measure():
    """The ``*_MEASURED`` constants of tests/_parity.py for this file's outputs: the fp32 models above against
    the fp64 references at the inputs of the tests, on the CPU."""
    from tests.test_rowwise_strict_gpu import _meas

    acc = {}
    for c in TAIL_CASES:
        gu, dm = tail_inputs(c)
        out, v = swiglu_plain_ref(dm, gu), tail_v_gauss(c)[:16 * c.nrb, :tail_width(c)]
        _meas(acc, "SWIGLU_LORA_TAIL", S_TAIL * (out.float() @ v.float().t()),
              S_TAIL * (out.double() @ v.double().t()), BF16)
    for c in PROJ_CASES:
        d = proj_case(c)
        for a, b in ((d["a0"], d["b0"]), (d["a1"], d["b1"])):
            ry, rdx, rda, rdb = proj_ref64(d["x"], d["w"], a, b, d["dy"], S_LORA, c.splits, c.r)
            y32, t = proj_fwd_model(d["x"], d["w"], a, b, S_LORA)
            _meas(acc, "LORA_PROJ_Y", y32, ry, BF16)
            for ga0, gb0 in ((None, None), (d["ga0"], d["gb0"])):
                dx32, da32, db32 = proj_bwd_model(d["dy"], d["x"], t, d["w"], a, b, S_LORA, c.splits, c.r, ga0, gb0)
                _meas(acc, "LORA_PROJ_DX", dx32, rdx, BF16)
                _meas(acc, "LORA_PROJ_DA", da32, rda + (0.0 if ga0 is None else ga0.double()), BF16)
                for i, (rows, cols) in enumerate(_blocks(c.splits, c.r)):
                    _meas(acc, "LORA_PROJ_DB", db32[i], rdb[i] + (0.0 if gb0 is None else gb0[rows, cols].double()),
                          BF16)
    for c in MLP_CASES:
        y32, dx32, dagu, dbgu, dad, dbd = mlp_model(c)
        ry, rdx, rdagu, rdbgu, rdad, rdbd = mlp_ref64(c)
        _meas(acc, "LORA_MLP_Y", y32, ry, BF16)
        _meas(acc, "LORA_MLP_DX", dx32, rdx, BF16)
        for m32, r64 in ((dagu, rdagu), (dad, rdad)):
            _meas(acc, "LORA_MLP_DA", m32, r64, BF16)
        for m32, r64 in zip(dbgu + dbd, rdbgu + rdbd):
            _meas(acc, "LORA_MLP_DB", m32, r64, BF16)
    return acc
