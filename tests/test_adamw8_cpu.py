"""fp8 AdamW moments on the CPU reference; tests/test_adamw8_gpu.py applies the same cases to ``adamw8_kernel``."""
import math

import pytest
import torch

from mxllm import ops
from mxllm.ops import reference as ref
from tests._parity import ULP_F32, assert_parity

ADAM = dict(lr=2.0 ** -10, beta1=0.875, beta2=0.9375, eps=2.0 ** -27, weight_decay=0.125, step=1)
GS = 0.5
# p of ``reference.adamw8_`` against fp64 from the same decoded state, max |err| / max |p| over SIZES x gradient dtypes
ADAMW8_P_MEASURED = (0, 7.6e-08)
ADAMW8_P = (ULP_F32, 1.52e-07)  # 2 x 0 < one ulp; 2 x 7.6e-08
SIZES = [64, 320, (1 << 20) + 64]  # one block; 5 blocks; a full grid pass of 1,024 x 256 x 4 plus one block


def make_case(n, gdt, dev="cpu"):
    """(p, g, m, v), block magnitudes 2^-20 .. 2^20; from 5 blocks on: block 0 zero, block 1 a 2^30 gradient spike."""
    gen = torch.Generator().manual_seed(7000 + n)
    sc = torch.exp2(torch.randint(-20, 21, (n // 64, 1), generator=gen).float()).expand(-1, 64).reshape(-1)
    p, m0, s0, g = [torch.randn(n, generator=gen) for _ in range(4)]
    m0, s0, g = m0 * sc, s0.abs() * sc, g * sc
    if n >= 320:
        m0[:128], s0[:128], g[:64] = 0, 0, 0
        g[64:128] = torch.randn(64, generator=gen) * 2.0 ** -10
        g[70] = 2.0 ** 20
    m, v = ops.QuantMoment.zeros(n, seed=3), ops.QuantMoment.zeros(n, seed=3, sqrt=True)
    for q, x in ((m, m0), (v, s0 * s0)):
        q.copy_(x)
        q.codes, q.exps = q.codes.to(dev), q.exps.to(dev)
    return p.to(dev), g.to(gdt).to(dev), m, v


def _nbr(y, up):  # the e4m3 value at or below (up: at or above) y >= 0 (fp64): spacing 2^(max(floor(log2 y), -6) - 3)
    sp = torch.ldexp(torch.ones_like(y), (torch.frexp(y)[1] - 1).clamp(min=-6) - 3)
    return (torch.ceil(y / sp) if up else torch.floor(y / sp)) * sp


def _rule_e(amax):  # the smallest e with amax / 2^e <= 448, by frexp in fp64: amax = f 2^ex, 448 = 0.875 x 2^9
    f, ex = torch.frexp(amax)
    return torch.where(amax > 0, (ex - 9 + (f > 0.875)).clamp(min=-100), 0)


def check_moment(q, x64, tol, positive=None):
    """The rule's block exponent; every decoded value a representable neighbour of the fp64 one (``tol`` allowed)."""
    a, tol, e = x64.abs().view(-1, 64), tol.view(-1, 64), q.exps.to(torch.int32)[:, None]
    assert bool(((_rule_e((a - tol).amax(1, True)) <= e) & (e <= _rule_e((a + tol).amax(1, True)))).all()), "exponent"
    d = ref.q8_decode(q.codes, q.exps).double().view(-1, 64)
    y, lo, hi = [torch.ldexp(t, -e) for t in (d.abs(), (a - tol).clamp(min=0), a + tol)]
    ok = (_nbr(lo, False) <= y) & (y <= _nbr(hi, True))
    ok &= (d == 0) | (a <= tol) | (torch.signbit(d) == torch.signbit(x64.view(-1, 64)))
    assert bool(ok.all()), f"{int((~ok).sum())} values are no neighbour, first {(~ok).nonzero()[0].tolist()}"
    if positive is not None:  # a positive sqrt(v) is stored at the smallest subnormal at least
        assert bool((y.reshape(-1)[positive] >= 2.0 ** -9).all()), "a positive sqrt(v) was flushed to zero"


def check_step(p0, g, m0, s0, p, m, v, special):
    """One step from ``p0`` and the decoded old state ``m0`` / ``s0``: p, m, sqrt(v) against fp64 (on the CPU)."""
    p0, g, m0, s0, p = [t.cpu().double() for t in (p0, g, m0, s0, p)]
    m, v = [ops.QuantMoment(q.codes.cpu(), q.exps.cpu(), sqrt=q.sqrt) for q in (m, v)]
    b1, b2, gd = ADAM["beta1"], ADAM["beta2"], g * GS
    m64, v64 = b1 * m0 + (1 - b1) * gd, b2 * s0 ** 2 + (1 - b2) * gd * gd
    den = (v64 / (1 - b2)).sqrt() + ADAM["eps"]
    p64 = p0 * (1 - ADAM["lr"] * ADAM["weight_decay"]) - ADAM["lr"] / (1 - b1) * m64 / den
    assert_parity(p.float(), p64, ADAMW8_P, scale="tensor", name="p")
    check_moment(m, m64, ULP_F32 * (b1 * m0.abs() + (1 - b1) * gd.abs()))
    check_moment(v, v64.sqrt(), ULP_F32 * v64.sqrt(), positive=v64 > 0)
    if special:  # the zero block; the spike survives and the rest of its block is the smallest subnormal
        assert not m.codes[:64].any() and not v.codes[:64].any() and not m.exps[0] and not v.exps[0]
        s = ref.q8_decode(v.codes, v.exps)[64:128]
        assert s[6] > 2.0 ** 16 and bool((s[torch.arange(64) != 6] == 2.0 ** (int(v.exps[1]) - 9)).all())


@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16], ids=["gradf32", "gradbf16"])
@pytest.mark.parametrize("n", SIZES[:2])
def test_reference_step(n, gdt):
    p, g, m, v = make_case(n, gdt)
    p0, m0, s0 = p.clone(), m.float(), ref.q8_decode(v.codes, v.exps)
    ops.adamw_step_(p, g, m, v, None, grad_scale=GS, **ADAM)
    check_step(p0, g, m0, s0, p, m, v, n >= 320)


def run_exact_halving(dev="cpu"):
    """beta1 = 1/2, beta2 = 1/4, zero gradient: m / 2 and s / 2 are representable, so they are kept exactly."""
    p, g, m, v = make_case(320, torch.float32, dev)
    m0, s0 = m.float(), ref.q8_decode(v.codes, v.exps)
    ops.adamw_step_(p, torch.zeros_like(g), m, v, None, **dict(ADAM, beta1=0.5, beta2=0.25))
    assert torch.equal(m.float(), 0.5 * m0) and torch.equal(ref.q8_decode(v.codes, v.exps), 0.5 * s0)


def run_decay(dev="cpu"):
    """s = 1, zero gradients, K steps until beta2^(K/2) has crossed three e4m3 steps (1 -> 13/16).  The mean decays to
    beta2^(K/2) within four standard errors; a rounding of x between lo and hi adds (x - lo)(hi - x) of variance."""
    n, b2, K = 4096, 0.999, math.ceil(2 * math.log(13 / 16) / math.log(0.999))
    p, g = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    m, v = ops.QuantMoment.zeros(n, dev), ops.QuantMoment.zeros(n, dev, sqrt=True)
    v.copy_(torch.ones(n))
    var = 0.0
    for k in range(1, K + 1):
        x = math.sqrt(b2) * ref.q8_decode(v.codes, v.exps).double().cpu()
        var = b2 * var + float(((x - _nbr(x, False)) * (_nbr(x, True) - x)).mean()) / n
        ops.adamw_step_(p, g, m, v, None, **dict(ADAM, beta2=b2, step=k))
    mean, want, se = float(ref.q8_decode(v.codes, v.exps).double().mean()), b2 ** (K / 2), math.sqrt(var)
    assert want <= 13 / 16 < 1 - 4 * se and abs(mean - want) <= 4 * se, (mean, want, se)
    return v


def run_chunked(dev="cpu"):
    """One launch over the buffer and the same buffer stepped in three block-aligned chunks: identical bits."""
    out = []
    for cuts in ([0, 320], [0, 64, 192, 320]):
        p, g, m, v = make_case(320, torch.bfloat16, dev)
        for lo, hi in zip(cuts, cuts[1:]):
            ops.adamw_step_(p[lo:hi], g[lo:hi], m[lo:hi], v[lo:hi], None, grad_scale=GS, **ADAM)
        out.append((p, m.codes, m.exps, v.codes, v.exps))
    assert all(torch.equal(a, b) for a, b in zip(*out))
    with pytest.raises(ValueError):
        m[32:96]  # not on block boundaries


@pytest.mark.parametrize("run", [run_exact_halving, run_decay, run_chunked])
def test_reference_rules(run):
    run()


def _trainer(state, kind="ddp", steps=0, seed=0, lr=1e-3):
    """A ``tiny`` trainer stepped over 4 cycled batches of 4 x 32 synthetic tokens: (trainer, losses)."""
    from mxllm.data import SyntheticTokens
    from mxllm.models import Llama, get_config
    from mxllm.parallel.runtime import DistEnv
    from mxllm.parallel.zero3 import Zero3Trainer
    from mxllm.train.trainer import OptimConfig, Trainer

    if kind == "zero3":
        tr = Zero3Trainer(get_config("tiny"), DistEnv(), OptimConfig(lr=lr), seed=5, optim_state=state)
    else:
        tr = Trainer(Llama(get_config("tiny"), seed=5), DistEnv(), OptimConfig(lr=lr), optim_state=state)
    data = SyntheticTokens(512, 4, 32, "cpu", seed=seed)
    tr.pool = [data.next() for _ in range(4)]
    return tr, [float(tr.train_step([tr.pool[k % 4]])) for k in range(steps)]


def test_convergence_within_seed_spread():
    """200 steps at lr 5e-4: on the same data the fp8-state final loss is no further from the fp32-state one than the
    fp32-state runs spread over data seeds 0, 1, 2.  Measured: fp32 0.0062 / 0.0030 / 0.0030, fp8 0.0058 (seed 0)."""
    f32 = [sum(_trainer("fp32", steps=200, seed=s, lr=5e-4)[1][-4:]) / 4 for s in range(3)]
    f8 = sum(_trainer("fp8", steps=200, lr=5e-4)[1][-4:]) / 4
    assert max(f32) < 0.6 and abs(f8 - f32[0]) <= max(f32) - min(f32), (f32, f8)


@pytest.mark.parametrize("kind", ["ddp", "zero3"])
@pytest.mark.parametrize("saved", ["fp8", "fp32"])
def test_checkpoint_into_fp8_state(tmp_path, saved, kind):
    """fp8 -> fp8: save, load and step equals step, bitwise.  fp32 -> fp8: the moments rounded to nearest."""
    from mxllm.train import checkpoint

    a, b = _trainer(saved, kind, steps=2)[0], _trainer("fp8", kind)[0]
    checkpoint.save(str(tmp_path), a, 2)
    checkpoint.load(str(tmp_path), b)
    if saved == "fp32":
        q = ops.QuantMoment.zeros(a.v.numel(), sqrt=True)
        q.copy_(a.v)
        assert torch.equal(q.codes, b.v.codes) and torch.equal(q.exps, b.v.exps) and b.m.codes.any()
        return
    got = []
    for t in (a, b):
        t.train_step([a.pool[2]])
        got.append((t.m.codes, t.m.exps, t.v.codes, t.v.exps, t.state_dict()["master"].float()))
    assert all(torch.equal(x, y) for x, y in zip(*got))
