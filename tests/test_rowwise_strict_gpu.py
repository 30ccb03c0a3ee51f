"""Per-element parity of the row and elementwise HIP kernels with fp64 references.

RMSNorm, SwiGLU, cross-entropy, AdamW, RoPE split / merge and the embedding: every compiled
template, every dispatch boundary (the ``iters_for(H)`` switch, ``rows_per_blk`` > 1 and its
partial last block, a second grid-stride pass), padded / strided outputs and the error paths
the host wrappers refuse.  Each output is compared element by element with an fp64 reference
computed from the same rounded inputs (``tests/_parity.py``: the bound and where its constants
come from).  The kernels are called through ``mxllm.ops.native()``: no Python fallback can stand
in for one.

Inputs are built on the CPU from fixed seeds, so ``measure()`` (``python -m
tests.test_rowwise_strict_gpu``, no GPU needed) reproduces the yardstick numbers recorded in
``tests/_parity.py`` at exactly the inputs the GPU tests use: the error of the plain fp32
PyTorch expression against the fp64 reference, per output, max over its cases.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from mxllm.ops import reference as ref
from tests import _parity as P
from tests._parity import assert_parity

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
EPS = 1e-5
SCALING = {"factor": 8.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0,
           "original_max_position_embeddings": 8192}


def _ops():
    from mxllm.ops import native

    return native()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape, dtype=torch.float32, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


# =========================================================================== RMSNorm
RMS_H = [8, 2048, 2056, 3072, 4096, 4104, 5120, 6144, 8192, 8200, 16384]


def _iters_for(H):
    chunks = (H // 8 + 255) // 256
    return 1 if chunks <= 1 else 2 if chunks <= 2 else 4 if chunks <= 4 else 8


def _rms_id(H):
    it = _iters_for(H)
    return f"H{H}-iters{it}-{'full' if H == it * 2048 else 'partial'}"


def _rpb(T, need_dw):
    return min(max(T // 512, 1), 32) if need_dw else 1


def rms_inputs(T, H, resid, seed=0):
    g = _gen(1000 + seed + 7 * T + H)
    x = _randn(g, T, H, dtype=BF16)
    r = _randn(g, T, H, dtype=BF16) if resid else None
    w = (1 + 0.1 * torch.randn(H, generator=g)).to(BF16)
    return x, r, w


def _rms_h(x, r):
    # the kernel normalises the rounded residual sum, as stored
    return x if r is None else (x.float() + r.float()).to(BF16)


def rms_fwd_ref64(x, r, w):
    h = _rms_h(x, r).double()
    rstd = torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + EPS)
    return h * rstd * w.double(), rstd.squeeze(-1)


def rms_fwd_fp32(x, r, w):  # reference.rms_norm's expression, before its output rounding
    h = _rms_h(x, r).float()
    rstd = torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + EPS)
    return h * rstd * w.float(), rstd.squeeze(-1)


def rms_bwd_inputs(T, H, seed=0):
    g = _gen(2000 + seed + 7 * T + H)
    x = _randn(g, T, H, dtype=BF16)
    w = (1 + 0.1 * torch.randn(H, generator=g)).to(BF16)
    dy = _randn(g, T, H, dtype=BF16)
    dres = _randn(g, T, H, dtype=BF16)
    # rstd is an input of the backward: the fp64 value rounded to the fp32 the kernel reads
    rstd = torch.rsqrt(x.double().pow(2).mean(-1) + EPS).float()
    return dy, x, w, rstd, dres


def _rms_bwd(dy, x, w, rstd, dres, dt):
    dy, x, w, rs = dy.to(dt), x.to(dt), w.to(dt), rstd.to(dt).unsqueeze(-1)
    gv = dy * w
    k = (gv * x).sum(-1, keepdim=True) * rs * rs * rs / x.shape[-1]
    dx = rs * gv - x * k
    if dres is not None:
        dx = dx + dres.to(dt)
    return dx, (dy * x * rs).sum(0)


def rms_bwd_ref64(dy, x, w, rstd, dres):
    return _rms_bwd(dy, x, w, rstd, dres, torch.float64)


def rms_bwd_fp32(dy, x, w, rstd, dres):
    return _rms_bwd(dy, x, w, rstd, dres, torch.float32)


@pytest.mark.parametrize("out_pad", [0, 64], ids=["pad0", "pad64"])
@pytest.mark.parametrize("resid", [False, True], ids=["plain", "resid"])
@pytest.mark.parametrize("T", [1, 3], ids=["T1", "T3"])
@pytest.mark.parametrize("H", RMS_H, ids=_rms_id)
def test_rmsnorm_fwd(gpu, H, T, resid, out_pad):
    x, r, w = rms_inputs(T, H, resid)
    xg, wg = x.to(gpu), w.to(gpu)
    rg = r.to(gpu) if resid else None
    y, rstd, h = _ops().rmsnorm_fwd(xg, rg, wg, EPS, out_pad)
    yr, rr = rms_fwd_ref64(xg, rg, wg)
    assert y.shape == (T, H) and y.stride() == (H + out_pad, 1)
    assert_parity(y, yr, P.RMSNORM_Y, name="y")
    assert_parity(rstd, rr, P.RMSNORM_RSTD, scale="tensor", name="rstd")
    if resid:
        assert torch.equal(h, (xg.float() + rg.float()).to(BF16))
    else:
        assert h.data_ptr() == xg.data_ptr()


def test_rmsnorm_fwd_too_wide_raises(gpu):
    x, _, w = rms_inputs(1, 16392, False)
    with pytest.raises(RuntimeError):
        _ops().rmsnorm_fwd(x.to(gpu), None, w.to(gpu), EPS, 0)


def _rms_bwd_check(gpu, T, H, dres_mode, need_dw, out_pad=0):
    dy, x, w, rstd, dres = [t.to(gpu) for t in rms_bwd_inputs(T, H)]
    if dres_mode == "strided":
        buf = torch.full((T, H + 64), float("nan"), device=gpu, dtype=BF16)
        buf[:, :H] = dres
        dres_in = buf[:, :H]
        assert not dres_in.is_contiguous()
    else:
        dres_in = dres if dres_mode else None
    dx, dw = _ops().rmsnorm_bwd(dy, x, w, rstd, dres_in, need_dw, out_pad)
    dxr, dwr = rms_bwd_ref64(dy, x, w, rstd, dres if dres_mode else None)
    assert dx.shape == (T, H) and dx.stride() == (H + out_pad, 1)
    assert_parity(dx, dxr, P.RMSNORM_DX, name="dx")
    if need_dw:
        assert_parity(dw, dwr, P.RMSNORM_DW, scale="tensor", name="dw")
    else:
        assert dw is None or dw.numel() == 0


@pytest.mark.parametrize("need_dw", [False, True], ids=["dw0", "dw1"])
@pytest.mark.parametrize("dres", [False, True], ids=["dres0", "dres1"])
@pytest.mark.parametrize("H", [2056, 3072, 8200], ids=lambda h: "rpb1-T5-" + _rms_id(h))
def test_rmsnorm_bwd_templates(gpu, H, dres, need_dw):
    """All four <DRES, DW> templates at widths with a partial last iteration; T = 5: rpb1."""
    _rms_bwd_check(gpu, 5, H, dres, need_dw)


@pytest.mark.parametrize("dres", [False, True], ids=["dres0", "dres1"])
@pytest.mark.parametrize("case", ["rpb3-T1537-H64", "rpb2-T1030-H3072", "rpb32-T16389-H64"])
def test_rmsnorm_bwd_multirow(gpu, case, dres):
    """rows_per_blk > 1 (need_dw): (1537, 64) rpb 3, 513 blocks, 1 row in the last; (1030, 3072)
    rpb 2, 515 blocks; (16389, 64) rpb capped at 32, 5 rows in the last block.  colsum_kernel sums
    block counts (513, 515, 513) that are no multiple of its 4 row slices."""
    rpb, T, H = [int(s.lstrip("rpbTH")) for s in case.split("-")]
    assert _rpb(T, True) == rpb
    assert (T, rpb, -(-T // rpb)) in [(1537, 3, 513), (1030, 2, 515), (16389, 32, 513)]
    _rms_bwd_check(gpu, T, H, dres, True)


@pytest.mark.parametrize("mode", ["dres-strided", "out-pad64", "dres-strided-out-pad64"])
def test_rmsnorm_bwd_strides(gpu, mode):
    """dres as a [T, H] view of a [T, H + 64] buffer (NaN in the pad) and dx into a padded buffer."""
    _rms_bwd_check(gpu, 5, 2056, "strided" if "dres-strided" in mode else True, True,
                   64 if "out-pad64" in mode else 0)


# =========================================================================== SwiGLU
SWIGLU_SHAPES = [(1, 8), (3, 24), (129, 1032)]
GATE_EDGES = [0.0, -0.0, 1e-3, -1e-3, 20.0, -20.0, 88.0, -88.0]


def swiglu_inputs(T, F_):
    g = _gen(3000 + T + F_)
    gu = _randn(g, T, 2 * F_, scale=2.0)
    gu[0, :8] = torch.tensor(GATE_EDGES)  # both sigmoid tails, __expf(-x) near overflow
    gu[T - 1, F_ - 8:F_] = torch.tensor(GATE_EDGES[::-1])
    return gu.to(BF16), _randn(g, T, F_, dtype=BF16)


def swiglu_ref64(gu, dm):
    F_ = gu.shape[-1] // 2
    g, u, d = gu[:, :F_].double(), gu[:, F_:].double(), dm.double()
    s = torch.sigmoid(g)
    return g * s * u, torch.cat([d * u * s * (1 + g * (1 - s)), d * g * s], dim=1)


def swiglu_fp32(gu, dm):  # reference.swiglu's expression and its autograd
    F_ = gu.shape[-1] // 2
    x = gu.float().requires_grad_(True)
    m = F.silu(x[:, :F_]) * x[:, F_:]
    m.backward(dm.float())
    return m.detach(), x.grad


@pytest.mark.parametrize("out_pad", [0, 64], ids=["pad0", "pad64"])
@pytest.mark.parametrize("T,F_", SWIGLU_SHAPES, ids=[f"T{t}-F{f}" for t, f in SWIGLU_SHAPES])
def test_swiglu(gpu, T, F_, out_pad):
    gu, dm = [t.to(gpu) for t in swiglu_inputs(T, F_)]
    mr, dgur = swiglu_ref64(gu, dm)
    m = _ops().swiglu_fwd(gu, out_pad)
    assert m.shape == (T, F_) and m.stride() == (F_ + out_pad, 1)
    assert_parity(m, mr, P.SWIGLU_M, name="m")
    dgu = _ops().swiglu_bwd(dm, gu, out_pad)
    assert dgu.shape == (T, 2 * F_) and dgu.stride() == (2 * F_ + out_pad, 1)
    # dg and du are separate outputs laid side by side: each half has its own row scale
    assert_parity(dgu[:, :F_], dgur[:, :F_], P.SWIGLU_DGU, name="dg")
    assert_parity(dgu[:, F_:], dgur[:, F_:], P.SWIGLU_DGU, name="du")
    if out_pad == 0:
        dgu2, m2 = _ops().swiglu_bwd_m(dm, gu)
        assert_parity(m2, mr, P.SWIGLU_M, name="m (bwd_m)")
        assert_parity(dgu2[:, :F_], dgur[:, :F_], P.SWIGLU_DGU, name="dg (bwd_m)")
        assert_parity(dgu2[:, F_:], dgur[:, F_:], P.SWIGLU_DGU, name="du (bwd_m)")


# =========================================================================== cross-entropy
CE_ENTRIES = ["ce_fwd_bwd", "ce_chunk", "ce_chunk_f32"]
CE_T = 7


def ce_inputs(V, entry, mag=None):
    """logits as fp32 values already rounded to what the entry point reads, and labels with the
    target at column 0, at column V - 1, and one ignored row."""
    g = _gen(4000 + V)
    lg = 3 * torch.randn(CE_T, V, generator=g)
    labels = torch.randint(0, V, (CE_T,), generator=g)
    labels[0], labels[1], labels[2] = 0, V - 1, -100
    if mag is not None:  # large magnitudes: every row spans [-mag, mag], the targets at both ends
        lg = (lg * (mag / 9)).clamp(-mag, mag)
        lg[:, 1], lg[:, V - 2] = mag, -mag
        lg[0, 0], lg[1, V - 1] = -mag, mag
    if entry != "ce_chunk_f32":
        lg = lg.to(BF16).float()
    return lg, labels


def ce_ref(lg, labels, ignore, dt=torch.float64):
    """losses [T], d(mean)/d(logits) [T, V], mean -- torch.nn.functional.cross_entropy in ``dt``.
    A label outside [0, V) counts as ignored.  No valid row: all zero (F.cross_entropy's own
    mean would be 0 / 0)."""
    V = lg.shape[1]
    valid = (labels != ignore) & (labels >= 0) & (labels < V)
    lab = torch.where(valid, labels, torch.full_like(labels, -100))
    x = lg.detach().to(dt).clone().requires_grad_(True)
    losses = F.cross_entropy(x, lab, ignore_index=-100, reduction="none")
    n = int(valid.sum())
    mean = losses.sum() * (1.0 / n if n else 0.0)
    mean.backward()
    return losses.detach(), x.grad, mean.detach()


def _ce_run(gpu, entry, lg, labels, ignore=-100):
    V = lg.shape[1]
    lab = labels.to(gpu)
    if entry == "ce_fwd_bwd":
        grad = lg.to(gpu, BF16)
        mean, losses = _ops().ce_fwd_bwd(grad, lab, ignore)
        return losses, grad, mean
    inv = _ops().ce_inv_count(lab, ignore, V)
    if entry == "ce_chunk":
        grad = lg.to(gpu, BF16)
        losses = _ops().ce_chunk(grad, lab, ignore, inv)
    else:
        grad = torch.empty(lg.shape, device=gpu, dtype=BF16)
        losses = _ops().ce_chunk_f32(lg.to(gpu), grad, lab, ignore, inv)
    return losses, grad, losses.sum() * inv[0]  # the caller's reduction (mxllm/ops/loss.py)


def _ce_check(gpu, entry, lg, labels, ref_labels=None, ignore=-100):
    losses, grad, mean = _ce_run(gpu, entry, lg, labels, ignore)
    lr, gr, mr = ce_ref(lg.to(gpu), (labels if ref_labels is None else ref_labels).to(gpu), ignore)
    print(f"{entry}: losses {losses.tolist()} mean {mean.item()} (fp64 {mr.item()}) "
          f"non-finite gradient elements {int((~torch.isfinite(grad.float())).sum())}")
    assert_parity(losses, lr, P.CE_LOSSES, scale="tensor", name="losses")
    assert_parity(grad, gr, P.CE_GRAD, name="dlogits")
    assert_parity(mean.reshape(1), mr.reshape(1), P.CE_MEAN, scale="tensor", name="mean loss")
    return losses, grad, mean


@pytest.mark.parametrize("V", [8, 1000, 2048, 2056], ids=lambda v: f"V{v}")
@pytest.mark.parametrize("entry", CE_ENTRIES)
def test_ce(gpu, entry, V):
    """V = 8: one lane holds data; 2048 / 2056: a lane's second chunk begins; targets at column 0
    and V - 1; one ignored row (zero loss, zero gradient row)."""
    lg, labels = ce_inputs(V, entry)
    losses, grad, _ = _ce_check(gpu, entry, lg, labels)
    assert losses[2].item() == 0.0 and not grad[2].any()


@pytest.mark.parametrize("entry", CE_ENTRIES)
def test_ce_all_ignored(gpu, entry):
    lg, _ = ce_inputs(1000, entry)
    labels = torch.full((CE_T,), -100)
    losses, grad, mean = _ce_run(gpu, entry, lg, labels)
    assert mean.item() == 0.0 and not losses.any() and not grad.any()
    assert torch.isfinite(grad.float()).all() and torch.isfinite(losses).all()


@pytest.mark.parametrize("V", [1000, 2056], ids=lambda v: f"V{v}")
@pytest.mark.parametrize("entry", CE_ENTRIES)
def test_ce_large_magnitude(gpu, entry, V):
    lg, labels = ce_inputs(V, entry, mag=80.0)
    losses, _, mean = _ce_check(gpu, entry, lg, labels)
    assert torch.isfinite(losses).all() and math.isfinite(mean.item())


@pytest.mark.parametrize("entry", CE_ENTRIES)
def test_ce_out_of_range_label_counts_as_ignored(gpu, entry):
    """A label outside [0, V) that is not the ignore index gets loss 0 and a zero gradient row in
    the row kernels; the valid-row count must leave it out too, or every other row's gradient and
    the mean are divided by a count that includes it."""
    V = 1000
    lg, labels = ce_inputs(V, entry)
    labels[3] = V + 3
    same = labels.clone()
    same[3] = -100
    losses, grad, _ = _ce_check(gpu, entry, lg, labels, ref_labels=same)
    assert losses[3].item() == 0.0 and not grad[3].any()


@pytest.mark.parametrize("V", [1000, 2056], ids=lambda v: f"V{v}")
@pytest.mark.parametrize("entry", CE_ENTRIES)
def test_ce_minus_inf_chunk(gpu, entry, V):
    """Columns 0-15 of one row are -inf (a masked vocabulary range): lanes 0 and 1 start on a
    chunk of eight -inf.  torch.nn.functional.cross_entropy gives a finite loss; so must the kernels."""
    lg, labels = ce_inputs(V, entry)
    lg[4, :16] = float("-inf")
    labels[4] = 500
    losses, grad, mean = _ce_check(gpu, entry, lg, labels)
    assert torch.isfinite(losses).all() and torch.isfinite(grad.float()).all() and math.isfinite(mean.item())
    assert not grad[4, :16].any()


# =========================================================================== AdamW
# every hyper-parameter (and 1 - beta^step for steps 1, 2) is exactly representable in fp32, so
# the launcher's double -> float conversion of them is not part of what is measured
ADAM = dict(lr=2.0 ** -10, beta1=0.875, beta2=0.9375, eps=2.0 ** -27, weight_decay=0.125)
ADAM_GS = 0.5
ADAM_FULL_PASS = 1024 * 256 * 4  # elements of one grid pass (1,024 workgroups x 256 lanes x 4)


def adamw_inputs(n, gdt):
    g = _gen(5000 + n)
    p = _randn(g, n)
    m = _randn(g, n).abs() * 0.1
    v = _randn(g, n).abs() * 0.1
    return p, m, v, _randn(g, n, dtype=gdt), _randn(g, n, dtype=gdt)


def adamw_ref64(p, g, m, v, step):
    b1, b2 = ADAM["beta1"], ADAM["beta2"]
    gd = g.double() * ADAM_GS
    m = b1 * m.double() + (1 - b1) * gd
    v = b2 * v.double() + (1 - b2) * gd * gd
    den = (v / (1 - b2 ** step)).sqrt() + ADAM["eps"]
    p = p.double() * (1 - ADAM["lr"] * ADAM["weight_decay"]) - (ADAM["lr"] / (1 - b1 ** step)) * m / den
    return p, m, v


def adamw_fp32(p, g, m, v, step):
    p, m, v = p.clone(), m.clone(), v.clone()
    ref.adamw_(p, g, m, v, step=step, grad_scale=ADAM_GS, **ADAM)
    return p, m, v


def _split(x):  # fp32 -> (hi bf16, lo int16): hi = (bits + 0x8000) >> 16, lo = bits - (hi << 16)
    b = x.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    h = ((b + 0x8000) >> 16) & 0xFFFF
    lo = b - (h << 16)
    lo = torch.where(lo >= 2 ** 31, lo - 2 ** 32, lo)
    hi = torch.where(h >= 2 ** 15, h - 2 ** 16, h).to(torch.int16).view(BF16)
    return hi, lo.to(torch.int16)


def _join(hi, lo):
    b = (((hi.view(torch.int16).to(torch.int64) & 0xFFFF) << 16) + lo.to(torch.int64)) & 0xFFFFFFFF
    return torch.where(b >= 2 ** 31, b - 2 ** 32, b).to(torch.int32).view(torch.float32)


@pytest.mark.parametrize("n", [ADAM_FULL_PASS + 4, 4], ids=["n1048580-2passes", "n4"])
@pytest.mark.parametrize("zero", [False, True], ids=["keepgrad", "zerograd"])
@pytest.mark.parametrize("mode", ["nolowp", "lowp", "splitmaster"])
@pytest.mark.parametrize("gdt", [torch.float32, BF16], ids=["gradf32", "gradbf16"])
def test_adamw(gpu, gdt, mode, zero, n):
    """Each launched <GRAD_BF16, LOWP, ZERO, SPLIT> variant, two steps (grad_scale as a float, then
    as a device tensor), every step checked against an fp64 AdamW from the state it started from.
    n = 2^20 + 4 is one 4-element group past a full grid pass."""
    p0, m0, v0, g1, g2 = [t.to(gpu) for t in adamw_inputs(n, gdt)]
    p, m, v = p0.clone(), m0.clone(), v0.clone()
    lowp = lo = None
    if mode == "lowp":
        lowp = torch.zeros(n, device=gpu, dtype=BF16)
    elif mode == "splitmaster":
        lowp, lo = _split(p0)
        assert torch.equal(_join(lowp, lo), p0)
    for step, (gsrc, scale) in enumerate([(g1, ADAM_GS), (g2, torch.tensor([ADAM_GS], device=gpu))], start=1):
        start = (p.clone() if lo is None else _join(lowp, lo)), m.clone(), v.clone()
        grad = gsrc.clone()
        st, sf = (scale, 1.0) if isinstance(scale, torch.Tensor) else (None, scale)
        args = (grad, m, v, lowp, lo, ADAM["lr"], ADAM["beta1"], ADAM["beta2"], ADAM["eps"], ADAM["weight_decay"],
                1.0 - ADAM["beta1"] ** step, 1.0 - ADAM["beta2"] ** step, st, sf, zero)
        _ops().adamw_step(None if lo is not None else p, *args)
        pr, mr, vr = adamw_ref64(start[0], gsrc, start[1], start[2], step)
        if lo is not None:
            got = torch.empty(n, device=gpu)
            _ops().join_master(lowp, lo, got)
            assert torch.equal(got, _join(lowp, lo))
            # the fp32-master kernel from the same state: the split form stores exactly its result,
            # and its high half is that result rounded half-up on its bit pattern
            pp, mm, vv = start[0].clone(), start[1].clone(), start[2].clone()
            _ops().adamw_step(pp, gsrc.clone(), mm, vv, None, None, *args[5:-1], False)
            assert torch.equal(got, pp)
            bits = pp.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
            assert torch.equal(lowp.view(torch.int16).to(torch.int64) & 0xFFFF, ((bits + 0x8000) >> 16) & 0xFFFF)
        else:
            got = p
        assert_parity(got, pr, P.ADAMW_P, scale="tensor", name=f"p step {step}")
        assert_parity(m, mr, P.ADAMW_M, scale="tensor", name=f"m step {step}")
        assert_parity(v, vr, P.ADAMW_V, scale="tensor", name=f"v step {step}")
        if mode == "lowp":
            assert torch.equal(lowp, p.to(BF16))
        assert (not grad.any()) if zero else torch.equal(grad, gsrc)
        # the elements past the first grid pass were updated (n = 4: the only group)
        assert (got[-4:] != start[0][-4:]).all() and (m[-4:] != start[1][-4:]).all()
        assert (v[-4:] != start[2][-4:]).all()


def test_adamw_n_not_multiple_of_4_raises(gpu):
    t = [torch.zeros(6, device=gpu) for _ in range(4)]
    with pytest.raises(RuntimeError):
        _ops().adamw_step(t[0], t[1], t[2], t[3], None, None, 1e-3, 0.9, 0.95, 1e-8, 0.1, 0.1, 0.05, None, 1.0, False)
    assert not t[0].any()


# =========================================================================== RoPE
ROPE_ODD = (2, 70, 8, 2)
ROPE_BIG = (2, 4096, 32, 8)  # B S NH D / 16 work items: more than one 4,096-workgroup grid pass


def rope_tables(S, D):
    return ref.rope_tables(S, D, 500000.0, SCALING)


def rope_split_inputs(B, S, Hq, Hkv, D):
    return _randn(_gen(6000 + S + D), B * S, (Hq + 2 * Hkv) * D, dtype=BF16)


def _rope_split(qkv, cos, sin, B, S, Hq, Hkv, D, pos, dt):
    x = qkv.to(dt).view(B, S, Hq + 2 * Hkv, D)
    idx = torch.arange(S, device=qkv.device).repeat(B) if pos is None else pos.long()
    c = cos.to(dt)[idx].view(B, S, 1, D // 2)
    s = sin.to(dt)[idx].view(B, S, 1, D // 2)
    x1, x2 = x[:, :, :Hq + Hkv, :D // 2], x[:, :, :Hq + Hkv, D // 2:]
    rot = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1).transpose(1, 2)  # reference.apply_rope's pairing
    return rot[:, :Hq].contiguous(), rot[:, Hq:].contiguous()


def rope_merge_inputs(B, S, Hq, Hkv, D, kvin):
    g = _gen(7000 + S + D + kvin)
    return _randn(g, B, Hq, S, D), _randn(g, B, kvin, S, D), _randn(g, B, kvin, S, D)


def _rope_merge(dq, dkp, dvp, cos, sin, B, S, Hq, Hkv, D, dt):
    c = cos.to(dt)[:S].view(1, 1, S, D // 2)
    s = sin.to(dt)[:S].view(1, 1, S, D // 2)
    dk = dkp.to(dt).view(B, Hkv, -1, S, D).sum(2)
    dv = dvp.to(dt).view(B, Hkv, -1, S, D).sum(2)

    def unrot(a):
        a1, a2 = a[..., :D // 2], a[..., D // 2:]
        return torch.cat([a1 * c + a2 * s, a2 * c - a1 * s], dim=-1)

    out = torch.cat([unrot(dq.to(dt)), unrot(dk), dv], dim=1)  # [B, NH, S, D]
    return out.transpose(1, 2).reshape(B * S, -1)


ROPE_CASES = [(d,) + ROPE_ODD for d in (32, 64, 128)] + [(128,) + ROPE_BIG]
ROPE_IDS = [f"D{c[0]}-B{c[1]}-S{c[2]}-Hq{c[3]}-Hkv{c[4]}" + ("-2gridpasses" if c[2] > 1000 else "")
            for c in ROPE_CASES]


@pytest.mark.parametrize("D,B,S,Hq,Hkv", ROPE_CASES, ids=ROPE_IDS)
def test_rope_split(gpu, D, B, S, Hq, Hkv):
    cos, sin = [t.to(gpu) for t in rope_tables(S + 3, D)]
    qkv = rope_split_inputs(B, S, Hq, Hkv, D).to(gpu)
    q, k, v = _ops().rope_split(qkv, cos, sin, B, S, Hq, Hkv, D)
    qr, kr = _rope_split(qkv, cos, sin, B, S, Hq, Hkv, D, None, torch.float64)
    assert_parity(q, qr, P.ROPE_QK, name="q")
    assert_parity(k, kr, P.ROPE_QK, name="k")
    assert torch.equal(v, qkv.view(B, S, -1, D)[:, :, Hq + Hkv:].transpose(1, 2).contiguous())


@pytest.mark.parametrize("D", [32, 64, 128], ids=lambda d: f"D{d}")
def test_rope_split_positions(gpu, D):
    B, S, Hq, Hkv = ROPE_ODD
    cos, sin = [t.to(gpu) for t in rope_tables(S, D)]
    qkv = rope_split_inputs(B, S, Hq, Hkv, D).to(gpu)
    g = _gen(61)
    pos = torch.cat([torch.randperm(S, generator=g) for _ in range(B)]).to(gpu, torch.int32)
    q, k, v = _ops().rope_split(qkv, cos, sin, B, S, Hq, Hkv, D, pos)
    qr, kr = _rope_split(qkv, cos, sin, B, S, Hq, Hkv, D, pos, torch.float64)
    assert_parity(q, qr, P.ROPE_QK, name="q (permuted positions)")
    assert_parity(k, kr, P.ROPE_QK, name="k (permuted positions)")
    none = _ops().rope_split(qkv, cos, sin, B, S, Hq, Hkv, D)
    assert torch.equal(v, none[2])
    ar = torch.arange(S, dtype=torch.int32, device=gpu).repeat(B)
    for a, b in zip(_ops().rope_split(qkv, cos, sin, B, S, Hq, Hkv, D, ar), none):
        assert torch.equal(a, b)


MERGE_CASES = ([(d,) + ROPE_ODD + (part, pad) for d in (32, 64, 128)
                for part, pad in (("perqhead", 0), ("presummed", 0), ("perqhead", 64), ("presummed", 64))]
               + [(128,) + ROPE_BIG + ("perqhead", 0)])
MERGE_IDS = [f"D{c[0]}-S{c[2]}-Hq{c[3]}-Hkv{c[4]}-{c[5]}-pad{c[6]}" + ("-2gridpasses" if c[2] > 1000 else "")
             for c in MERGE_CASES]


@pytest.mark.parametrize("D,B,S,Hq,Hkv,part,out_pad", MERGE_CASES, ids=MERGE_IDS)
def test_rope_merge_bwd(gpu, D, B, S, Hq, Hkv, part, out_pad):
    kvin = Hq if part == "perqhead" else Hkv
    cos, sin = [t.to(gpu) for t in rope_tables(S + 3, D)]
    dq, dkp, dvp = [t.to(gpu) for t in rope_merge_inputs(B, S, Hq, Hkv, D, kvin)]
    out = _ops().rope_merge_bwd(dq, dkp, dvp, cos, sin, B, S, Hq, Hkv, D, out_pad)
    NHD = (Hq + 2 * Hkv) * D
    assert out.shape == (B * S, NHD) and out.stride() == (NHD + out_pad, 1)
    want = _rope_merge(dq, dkp, dvp, cos, sin, B, S, Hq, Hkv, D, torch.float64)
    # one bound per head: a token row holds Hq + 2 Hkv separately produced heads
    assert_parity(out.reshape(B * S, -1, D), want.view(B * S, -1, D), P.ROPE_DQKV, name="dqkv")


# =========================================================================== embedding
EMB_V, EMB_T = 50, 64


def emb_inputs(H):
    g = _gen(8000 + H)
    w = _randn(g, EMB_V, H, dtype=BF16)
    ids = torch.randint(0, EMB_V, (EMB_T,), generator=g)
    ids[0], ids[1] = 0, EMB_V - 1
    ids[EMB_T // 2:] = 17  # one id repeated for half the tokens
    return w, ids, _randn(g, EMB_T, H, dtype=BF16)


def emb_bwd(dy, ids, dt):
    return torch.zeros(EMB_V, dy.shape[1], dtype=dt, device=dy.device).index_add_(0, ids, dy.to(dt))


@pytest.mark.parametrize("H", [8, 2056, 8192], ids=lambda h: f"H{h}")
def test_embedding(gpu, H):
    w, ids, dy = [t.to(gpu) for t in emb_inputs(H)]
    assert torch.equal(_ops().embedding_fwd(ids, w), w[ids])
    dw = _ops().embedding_bwd(dy, ids, EMB_V)
    assert_parity(dw, emb_bwd(dy, ids, torch.float64), P.EMBEDDING_DW, name="dW")


# =========================================================================== yardstick
def _meas(acc, name, y32, r64, out_dtype, scale="row"):
    """rel: the rounding of the fp32 result to the output dtype; abs: the fp32 arithmetic against
    fp64, relative to the row's / tensor's max |ref| (tests/_parity.py)."""
    y, r = y32.double(), r64.double()
    s = r.abs().amax(-1, keepdim=True) if scale == "row" else r.abs().max()
    ok = torch.isfinite(r) & (s > 0)
    ab = ((y - r).abs() / s)[ok.expand_as(r)].max().item() if ok.any() else 0.0
    rounded = y32.to(out_dtype).double()
    nz = y.abs() >= torch.finfo(out_dtype).tiny  # below it the output dtype is subnormal: the abs term's
    rel = ((rounded - y).abs()[nz] / y.abs()[nz]).max().item() if nz.any() else 0.0
    cur = acc.get(name, (0.0, 0.0))
    acc[name] = (max(cur[0], rel), max(cur[1], ab))


def measure():
    """Error of the plain fp32 PyTorch expressions against the fp64 references at the inputs of
    the tests above, on the CPU: the ``*_MEASURED`` constants of tests/_parity.py."""
    acc = {}
    f32 = torch.float32
    for H in RMS_H:
        for T in (1, 3):
            for resid in (False, True):
                x, r, w = rms_inputs(T, H, resid)
                (y, rs), (yr, rr) = rms_fwd_fp32(x, r, w), rms_fwd_ref64(x, r, w)
                _meas(acc, "RMSNORM_Y", y, yr, BF16)
                _meas(acc, "RMSNORM_RSTD", rs, rr, f32, "tensor")
    for T, H in [(5, 2056), (5, 3072), (5, 8200), (1537, 64), (1030, 3072), (16389, 64)]:
        dy, x, w, rstd, dres = rms_bwd_inputs(T, H)
        for d in (None, dres):
            (dx, dw), (dxr, dwr) = rms_bwd_fp32(dy, x, w, rstd, d), rms_bwd_ref64(dy, x, w, rstd, d)
            _meas(acc, "RMSNORM_DX", dx, dxr, BF16)
            _meas(acc, "RMSNORM_DW", dw, dwr, f32, "tensor")
    for T, F_ in SWIGLU_SHAPES:
        gu, dm = swiglu_inputs(T, F_)
        (m, dgu), (mr, dgur) = swiglu_fp32(gu, dm), swiglu_ref64(gu, dm)
        _meas(acc, "SWIGLU_M", m, mr, BF16)
        _meas(acc, "SWIGLU_DGU", dgu[:, :F_], dgur[:, :F_], BF16)
        _meas(acc, "SWIGLU_DGU", dgu[:, F_:], dgur[:, F_:], BF16)
    for entry in CE_ENTRIES:
        cases = [ce_inputs(V, entry) for V in (8, 1000, 2048, 2056)]
        cases += [ce_inputs(V, entry, mag=80.0) for V in (1000, 2056)]
        for V in (1000, 2056):
            lg, labels = ce_inputs(V, entry)
            lg[4, :16] = float("-inf")
            labels[4] = 500
            cases.append((lg, labels))
        for lg, labels in cases:
            (l, g, mn), (lr, gr, mr) = ce_ref(lg, labels, -100, f32), ce_ref(lg, labels, -100)
            _meas(acc, "CE_LOSSES", l, lr, f32, "tensor")
            _meas(acc, "CE_GRAD", g, gr, BF16)
            _meas(acc, "CE_MEAN", mn.reshape(1), mr.reshape(1), f32, "tensor")
    for gdt in (f32, BF16):
        for n in (ADAM_FULL_PASS + 4, 4):
            p, m, v, g1, g2 = adamw_inputs(n, gdt)
            for step, g in ((1, g1), (2, g2)):
                got, want = adamw_fp32(p, g, m, v, step), adamw_ref64(p, g, m, v, step)
                for nm, a, b in zip(("ADAMW_P", "ADAMW_M", "ADAMW_V"), got, want):
                    _meas(acc, nm, a, b, f32, "tensor")
                p, m, v = got
    for D, B, S, Hq, Hkv in ROPE_CASES:
        cos, sin = rope_tables(S + 3, D)
        qkv = rope_split_inputs(B, S, Hq, Hkv, D)
        pos = None
        for _ in range(2 if S < 1000 else 1):
            got = _rope_split(qkv, cos, sin, B, S, Hq, Hkv, D, pos, f32)
            want = _rope_split(qkv, cos, sin, B, S, Hq, Hkv, D, pos, torch.float64)
            for a, b in zip(got, want):
                _meas(acc, "ROPE_QK", a, b, BF16)
            pos = torch.cat([torch.randperm(S, generator=_gen(61)) for _ in range(B)])
    for D, B, S, Hq, Hkv, part, _pad in MERGE_CASES:
        if _pad:
            continue
        kvin = Hq if part == "perqhead" else Hkv
        cos, sin = rope_tables(S + 3, D)
        dq, dkp, dvp = rope_merge_inputs(B, S, Hq, Hkv, D, kvin)
        a = _rope_merge(dq, dkp, dvp, cos, sin, B, S, Hq, Hkv, D, f32)
        b = _rope_merge(dq, dkp, dvp, cos, sin, B, S, Hq, Hkv, D, torch.float64)
        _meas(acc, "ROPE_DQKV", a.view(B * S, -1, D), b.view(B * S, -1, D), BF16)
    for H in (8, 2056, 8192):
        _w, ids, dy = emb_inputs(H)
        _meas(acc, "EMBEDDING_DW", emb_bwd(dy, ids, f32), emb_bwd(dy, ids, torch.float64), f32)
    for name, (rel, ab) in acc.items():
        print(f"{name}_MEASURED = ({rel:.3g}, {ab:.3g})")
    return acc


if __name__ == "__main__":
    measure()
