"""Cases, the fp64 reference and the checks of the strict training-step tests (tests/test_step_strict_gpu.py on
the GPU, tests/test_step_cases.py on the CPU).

Unit under test: three optimizer steps of ``mxllm.train.trainer.Trainer`` (``compute_grads`` + ``_optimizer_step``
over ``mxllm/parallel/flat.py``) and of ``mxllm.parallel.zero3.Zero3Trainer.train_step``, in one process, on the
whole-model case of tests/_layer_cases.py (tiny-d128, 2 layers, V = H = 512, F = 1024, ids [2, 256]).

The reference is plain PyTorch in fp64 and calls nothing of ``mxllm.ops`` / ``mxllm.train``:
  * ``ref_loss_grads``: the loss of a step is the mean over the micro-batches of each micro-batch's mean over its
    own valid tokens (a micro-batch with no valid token: loss 0, gradient 0), its gradient that of
    ``_layer_cases.model_math(..., F64, model=False)`` at the bf16 values the trainer computes with;
  * ``adamw64``: from the state before the step and the gradient buffer G the trainer holds,
    gnorm = ||G|| scale, coef = min(1, clip / (gnorm + 1e-6)), gscale = coef scale (no clip: scale), decoupled
    weight decay AdamW with ``lr_ref(step)`` (linear warm-up to ``warmup_steps``, then half a cosine to
    ``total_steps``, written out here) and the bias corrections 1 - beta^step.
Every step is checked from the trainer's OWN state before the step and its OWN gradient buffer (teacher forcing):
no sign flip of a first AdamW step has to be tolerated, and each step's check stands alone.

``check_step`` holds one step's record to: (1) the loss, (2) every element of the gradient buffer (row scale,
pads exactly zero, all finite), (3) the clip norm, (4) master / m / v after the step (tensor scale per slot, pads
exactly zero), (5) the stored bf16 parameters = the master's high half by the split rule
(hi = (bits + 0x8000) >> 16), LoRA: every adapter copy equal, every frozen weight untouched.  ``run_case`` adds
(6) continuity (the state before step s + 1 is bitwise the state after step s), (7) an unobserved rerun through
plain ``train_step`` with bitwise the same losses and final state, and the spies of each case's path.

``simulate`` is the reference written as a trainer (fp64 gradients rounded into the buffer's dtype, fp64 AdamW
rounded to fp32) over a layout WITH alignment pads; ``DEFECTS`` are planted in it and every one must be
rejected by ``check_step`` (tests/test_step_cases.py).  ``measure()`` (``python -m tests._step_cases``, no GPU)
prints the ``STEP_*_MEASURED`` constants of tests/_parity.py: the fp32 model of the step (``model_math(..., F32,
model=True)``, accumulation in the buffer's dtype with one rounding per added micro-batch,
``mxllm/ops/reference.py`` ``adamw_`` in fp32 with an fp32 norm) against the fp64 reference along the fp64
reference trajectory of every case.
"""
from __future__ import annotations

import functools
import math
import sys
from collections import namedtuple
from types import SimpleNamespace

import torch

from tests import _layer_cases as LY
from tests import _parity as P
from tests._parity import assert_exact, assert_parity

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
IGNORE = LY.IGNORE
STEPS = 3
LORA_R = LY.LORA_256.lora
# lr 5e-4, 1e-3, 5e-4 at steps 1, 2, 3: a stale step number or learning rate shows at both transitions
OPT = dict(lr=1e-3, beta1=0.9, beta2=0.95, eps=1e-8, weight_decay=0.01, warmup_steps=2, total_steps=4)
# case 1: between the smallest and the largest clip norm of its fp64 reference trajectory (``measure`` prints
# them: 2.38, 2.84, 2.25 -- on the CPU path of the trainer the same to three digits): the coefficient is exactly 1 at
# steps 1 and 3 and 0.88 at step 2
CLIP_1 = 2.5

# plan: per step, the micro-batches: A the batch of ``model_inputs``, B its rows swapped with half the labels
# ignored (the valid counts differ: a mean of means is not the token mean), Z every label ignored
_P1 = (("A",), ("B",), ("A",))
_P2 = (("A", "B"), ("B", "A"), ("A", "B"))
_P3 = (("A", "Z", "B"), ("Z", "A", "B"), ("B", "A", "Z"))

StepCase = namedtuple("StepCase", "num name zero3 tied lora gdt ckpt env clip overlap world plan")


def _c(num, name, plan, zero3=False, tied=False, lora=0, gdt=None, ckpt=False, env=(), clip=1.0, overlap=None, world=1):
    return StepCase(num, name, zero3, tied, lora, gdt, ckpt, tuple(env), clip, overlap, world, plan)


_G8 = (("MXLLM_GEMM8", "all"),)
CASES = (
    _c(1, "full-gemm8-fusednorm-1mb", _P1, env=_G8, clip=CLIP_1),
    _c(2, "full-gemm8-3mb-ignored", _P3, env=_G8),
    _c(3, "full-fp32grads-2mb", _P2, gdt=F32),
    _c(4, "tied-2mb", _P2, tied=True),
    _c(5, "ckpt1-2mb", _P2, ckpt=1),
    _c(6, "deterministic-1mb", _P1, env=(("MXLLM_DETERMINISTIC", "1"),)),
    _c(7, "noclip-onelaunch-2mb", _P2, clip=0.0, overlap=False),
    _c(8, "lora-1mb", _P1, lora=LORA_R),
    _c(8, "lora-2mb", _P2, lora=LORA_R),
    _c(9, "lora-overlap-2mb", _P2, lora=LORA_R, env=(("MXLLM_LORA_OVERLAP_ADAMW", "1"),)),
    _c(10, "zero3-w1-fp32-2mb", _P2, zero3=True, gdt=F32),
    _c(11, "zero3-w1-ckpt1-3mb-ignored", _P3, zero3=True, gdt=F32, ckpt=1),
    _c(12, "zero3-w1-bf16grads-2mb", _P2, zero3=True, gdt=BF16),
    _c(13, "zero3-emulated4-ckpt-2mb", _P2, zero3=True, gdt=F32, ckpt=True, world=4),
)
CPU_CASES = tuple(c for c in CASES if c.num not in (6, 9))  # (the two GPU-only switches)
ZERO3_SEED = 13


def case_id(c):
    return f"{c.num}-{c.name}"


def by_name(name):
    return next(c for c in CASES if c.name == name)


# =========================================================================== inputs
@functools.lru_cache(maxsize=None)
def micro_batch(tied, letter):
    ids, labels = LY.model_inputs(tied)[:2]
    if letter == "A":
        return ids, labels
    if letter == "Z":
        return ids, torch.full_like(labels, IGNORE)
    assert letter == "B"
    drop = torch.rand(labels.shape, generator=LY._gen(LY._seed(LY.MODEL_CASE) + 777)) < 0.5
    return ids.flip(0).contiguous(), labels.flip(0).masked_fill(drop, IGNORE)


def batches(c, step, dev="cpu"):
    return [tuple(t.to(dev) for t in micro_batch(c.tied, k)) for k in c.plan[step - 1]]


def lr_ref(step, o=OPT):
    """Linear warm-up to ``warmup_steps``, then half a cosine to ``total_steps``, constant afterwards."""
    w, t = o["warmup_steps"], o["total_steps"]
    if w and step <= w:
        return o["lr"] * step / w
    if t and step > w:
        return o["lr"] * 0.5 * (1.0 + math.cos(math.pi * min(1.0, (step - w) / max(1, t - w))))
    return o["lr"]


# =========================================================================== layouts
# A flat state vector (master, m, v, the gradient buffer) is a row of units; a unit holds ``full_numel`` elements
# of named slots (name, offset, numel, shape) and pads, of which the rank stores ``shard_numel``: all of them at
# world 1 and for a replicated unit, else the sum (gradients) or the first (parameters) of ``world`` slices.
Unit = namedtuple("Unit", "off shard_numel full_numel replicated slots")


def layout_of_flat(flat):
    return SimpleNamespace(world=1, numel=flat.numel, units=[Unit(0, flat.numel, flat.numel, True, [
        (s.name, s.offset, s.numel, tuple(s.shape)) for s in flat.slots])])


def layout_of_zero3(z):
    units, off = [], 0
    for u in z.units:
        units.append(Unit(off, u.shard_numel, u.full_numel, u.replicated,
                          list(zip(u.names, u.offsets, u.numels, u.shapes))))
        off += u.shard_numel
    return SimpleNamespace(world=z.world, numel=off, units=units)


def sim_layout(c, shapes):
    """The layout of ``simulate``: the trainer's rule (slots aligned to 64; ZeRO-3: norms | emb | layers | head,
    units rounded to 64 x world) with a pad after EVERY slot, which the shapes of the tests never need."""
    world, pad = c.world, 64

    def unit(off, names, replicated):
        slots, o = [], 0
        for n in names:
            slots.append((n, o, math.prod(shapes[n]), tuple(shapes[n])))
            o += math.prod(shapes[n]) + pad
        wsz = 1 if replicated else world
        full = (o + 64 * wsz - 1) // (64 * wsz) * (64 * wsz)
        return Unit(off, full // wsz, full, replicated, slots)

    if not c.zero3:
        u = unit(0, list(shapes), True)
        return SimpleNamespace(world=1, numel=u.full_numel, units=[u])
    groups = [[n for n in shapes if n.endswith("norm")], ["tok_emb"]]
    groups += [[f"layers.{i}.{p}.weight" for p in LY.PROJS] for i in (0, 1)] + [["lm_head"]]
    units, off = [], 0
    for k, names in enumerate(groups):
        units.append(unit(off, names, k == 0))
        off += units[-1].shard_numel
    return SimpleNamespace(world=world, numel=off, units=units)


def pad_mask(lay, dev):
    """True where a flat element belongs to no slot (world > 1: to no slot in any of the folded slices)."""
    mask = torch.ones(lay.numel, dtype=torch.bool, device=dev)
    for u in lay.units:
        used = torch.zeros(u.full_numel, dtype=torch.bool, device=dev)
        for _, o, n, _ in u.slots:
            used[o:o + n] = True
        if u.full_numel != u.shard_numel:
            used = used.view(lay.world, -1).any(0)
        mask[u.off:u.off + u.shard_numel] = ~used
    return mask


def named_values(lay, flat):
    """{name: tensor} of a flat PARAMETER vector (a sharded unit of world > 1: its shard tiled, as the emulated
    all-gather builds it)."""
    out = {}
    for u in lay.units:
        full = flat[u.off:u.off + u.shard_numel]
        if u.full_numel != u.shard_numel:
            full = full.repeat(lay.world)
        for name, o, n, shape in u.slots:
            out[name] = full[o:o + n].view(shape)
    return out


def flat_values(lay, named, dtype, dev):
    """The flat parameter vector of {name: tensor} (pads 0; world > 1: the first slice of each sharded unit)."""
    flat = torch.zeros(lay.numel, dtype=dtype, device=dev)
    for u in lay.units:
        full = torch.zeros(u.full_numel, dtype=dtype, device=dev)
        for name, o, n, _ in u.slots:
            full[o:o + n] = named[name].reshape(-1).to(dtype)
        flat[u.off:u.off + u.shard_numel] = full[:u.shard_numel]
    return flat


# =========================================================================== the reference
def grad_bound_name(c, name, gdt):
    key = LY.param_key(name).split(".")[-1].upper()
    if c.lora:
        key = "LORA_" + key
    if key == "DEMB" and c.tied:
        key = "DEMB_TIED"
    if c.zero3:  # its own weights (N(0, 0.02), gamma 1): constants of their own, the trainer's are not widened
        key = "Z3_" + key
    return key + ("_F32" if gdt == F32 else "")


def grad_bound(c, name, gdt):
    """(bound, its name): STEP_<kind> where the step's measurement exceeded the whole-model constant (or there
    is none), else MODEL_<kind>."""
    key = grad_bound_name(c, name, gdt)
    for n in ("STEP_" + key, "MODEL_" + key):
        if hasattr(P, n):
            return getattr(P, n), n
    raise AssertionError(f"no bound for {key}")


def accum_dtype(c):
    """The dtype gradients are formed and accumulated in (the ZeRO-3 buffer itself is always fp32: with bf16
    gradients it adds bf16-rounded micro-batch gradients)."""
    return c.gdt or BF16


def ref_loss_grads(c, params, mbs, dt=F64, model=False, loss_scale=None):
    """(loss of the step [1], {name: gradient of that loss}, per micro-batch outputs) at ``params`` {name: value}."""
    n = len(mbs)
    outs = [LY.model_math(c.tied, dt, model, params=params, batch=mb, lora=c.lora,
                          loss_scale=1.0 / n if loss_scale is None else loss_scale) for mb in mbs]
    loss = sum(o["loss"] for o in outs) / n
    grads = {name: sum(o[LY.param_key(name)] for o in outs) for name in params if LY.trainable(name, c.lora)}
    return loss, grads, outs


def gmul(c, n):
    """What the gradient buffer holds, in units of the gradient of the step's loss: the trainer runs every
    backward on loss / n (scale 1 / world), ZeRO-3 adds the micro-batches' own gradients (scale 1 / (world n);
    the emulated world's factor is in the fold of ``expected_buffer``)."""
    return float(n) if c.zero3 else 1.0


def expected_buffer(c, lay, grads, n, dev, bounds=True):
    """The fp64 gradient buffer and, per element, the two magnitudes of its bound: (G, |terms|, row maxima per
    bound constant): a sharded unit of world W > 1 is the sum of its W slices (the emulated reduce-scatter), a
    replicated unit W times its gradient (the emulated all-reduce); the bound of a sum is the sum of the bounds."""
    G = torch.zeros(lay.numel, dtype=F64, device=dev)
    lim = torch.zeros(lay.numel, dtype=F64, device=dev)
    gdt = accum_dtype(c)
    for u in lay.units:
        full = torch.zeros(u.full_numel, dtype=F64, device=dev)
        fl = torch.zeros(u.full_numel, dtype=F64, device=dev)
        for name, o, k, shape in u.slots:
            if name not in grads:
                continue
            g = (grads[name].to(dev) * gmul(c, n)).view(shape)
            (c_rel, c_abs), _ = grad_bound(c, name, gdt) if bounds else ((0.0, 0.0), None)
            full[o:o + k] = g.reshape(-1)
            fl[o:o + k] = (c_rel * g.abs() + c_abs * g.abs().amax(-1, keepdim=True)).reshape(-1)
        if u.full_numel != u.shard_numel:
            full, fl = full.view(lay.world, -1).sum(0), fl.view(lay.world, -1).sum(0)
        elif lay.world > 1:
            full, fl = full * lay.world, fl * lay.world
        G[u.off:u.off + u.shard_numel], lim[u.off:u.off + u.shard_numel] = full, fl
    return G, lim


def adamw64(c, step, state, G, scale, defect=None, lay=None):
    """fp64: (gnorm, coef, (master, m, v) after) from (master, m, v) before and the buffer ``G``."""
    o = OPT
    p, m, v = [t.double() for t in state]
    g = G.double()
    sq = g.pow(2).sum()
    if defect == "norm-skips-embedding":
        u, (_, off, k, _) = next((u, s) for u in lay.units for s in u.slots if s[0] == "tok_emb")
        sq = sq - g[u.off + off:u.off + off + k].pow(2).sum()
    if defect == "zero3-replicated-unit-counted-world-times":
        sq = sq + (lay.world - 1) * g[:lay.units[0].shard_numel].pow(2).sum()
    gnorm = sq.sqrt() * (1.0 if defect == "norm-of-unscaled-sum" else scale)
    coef = 1.0
    if c.clip > 0:
        coef = c.clip / (float(gnorm) + 1e-6)
        if defect != "coef-not-clamped":
            coef = min(1.0, coef)
    gs = g * (coef * scale)
    b1, b2 = o["beta1"], o["beta2"]
    lr = lr_ref(step - 1 if defect == "lr-of-previous-step" else step)
    bstep = step - 1 if defect == "bias-correction-step-minus-one" else step
    bc1, bc2 = max(1 - b1 ** bstep, 1e-30), max(1 - b2 ** bstep, 1e-30)
    if defect == "weight-decay-as-l2":
        gs = gs + o["weight_decay"] * p
    m = b1 * m + (1 - b1) * gs
    v = b2 * v + (1 - b2) * gs * gs
    if defect != "weight-decay-as-l2":
        p = p * (1 - lr * o["weight_decay"])
    p = p - (lr / bc1) * m / ((v / bc2).sqrt() + o["eps"])
    return gnorm, coef, (p, m, v)


def split_hi(master):
    """The bf16 high half of an fp32 master by the split rule: hi = (bits + 0x8000) >> 16."""
    b = master.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    h = ((b + 0x8000) >> 16) & 0xFFFF
    return torch.where(h >= 2 ** 15, h - 2 ** 16, h).to(torch.int16).view(BF16)


def is_tie(master):
    """Masters the split rule rounds up and round-to-nearest-even down: low half exactly 0x8000, high half even."""
    b = master.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return ((b & 0xFFFF) == 0x8000) & (((b >> 16) & 1) == 0)


# =========================================================================== the check of one step
def _segments(lay):
    """(name, lo, hi) per slot at world 1, per unit where slices fold."""
    for k, u in enumerate(lay.units):
        if lay.world == 1:
            for name, o, n, _ in u.slots:
                yield name, u.off + o, u.off + o + n
        else:
            yield f"unit{k}", u.off, u.off + u.shard_numel


def check_step(c, lay, rec, name=""):
    """One step's record against the fp64 reference (module doc, checks 1-5).  ``rec``: step, mbs, params
    {name: the bf16 values the forward read}, loss, G (the flat gradient buffer), scale, gnorm (None without
    clipping), before / after = (master, m, v) fp32, stored (the flat bf16 parameters after the step, None: the
    parameters are fp32), split (whether the master is split), copies [(adapter, its copy)], frozen
    [(name, before step 1, now)].  Returns (gnorm, coef) of the reference."""
    step, n, dev = rec.step, len(rec.mbs), rec.G.device
    tag = f"{name or case_id(c)} step {step}"
    loss64, grads, _ = ref_loss_grads(c, rec.params, rec.mbs)
    # 1
    assert rec.loss.dtype == F32 and bool(torch.isfinite(rec.loss).all()), f"{tag}: loss {rec.loss}"
    assert_parity(rec.loss.reshape(1), loss64.reshape(1).to(dev), P.STEP_LOSS, scale="row",
                  name=f"{tag}: loss (STEP_LOSS)")
    # 2
    gdt = accum_dtype(c)
    assert rec.G.dtype == (F32 if c.zero3 else gdt), f"{tag}: gradient buffer is {rec.G.dtype}"
    assert bool(torch.isfinite(rec.G).all()), f"{tag}: non-finite gradient"
    pads = pad_mask(lay, dev)
    assert not bool(rec.G[pads].any()), f"{tag}: gradient pad not zero"
    want, lim = expected_buffer(c, lay, grads, n, dev)
    if lay.world == 1:
        for u in lay.units:
            for pname, o, k, shape in u.slots:
                if pname in grads:
                    bound, bname = grad_bound(c, pname, gdt)
                    assert_parity(rec.G[u.off + o:u.off + o + k].view(shape), want[u.off + o:u.off + o + k].view(shape),
                                  bound, scale="row", name=f"{tag}: gradient of {pname} ({bname})")
    else:
        err = (rec.G.double() - want).abs()
        for sname, lo, hi in _segments(lay):
            bad = ~(err[lo:hi] <= lim[lo:hi])
            assert not bool(bad.any()), (f"{tag}: gradient of {sname}: {int(bad.sum())} of {hi - lo} elements exceed "
                                         f"the folded bound, worst |diff| {float(err[lo:hi][bad].max()):.3g}")
    # 3
    scale = 1.0 / (lay.world * n) if c.zero3 else 1.0  # the contract: 1 / world, ZeRO-3 1 / (world n)
    if not c.zero3:
        assert rec.scale == scale, f"{tag}: compute_grads returned the scale {rec.scale}"
    gnorm, coef, after = adamw64(c, step, rec.before, rec.G, scale)
    if c.clip > 0:
        assert rec.gnorm is not None and abs(float(rec.gnorm) - float(gnorm)) <= 1e-6 * float(gnorm), \
            f"{tag}: clip norm {float(rec.gnorm):.9g}, of the buffer {float(gnorm):.9g}"
    else:
        assert rec.gnorm is None, f"{tag}: a clip norm without clipping"
    # 4
    bounds = (P.STEP_ADAMW_P, P.STEP_ADAMW_M, P.STEP_ADAMW_V)
    for what, got, ref, bound in zip(("master", "m", "v"), rec.after, after, bounds):
        assert got.dtype == F32, f"{tag}: {what} is {got.dtype}"
        assert not bool(got[pads].any()), f"{tag}: {what} pad not zero"
        for sname, lo, hi in _segments(lay):
            assert_parity(got[lo:hi], ref[lo:hi], bound, scale="tensor", name=f"{tag}: {what} of {sname}")
    # 5
    if rec.stored is not None:
        hi = split_hi(rec.after[0]) if rec.split else rec.after[0].to(BF16)
        assert_exact(rec.stored, hi, f"{tag}: stored bf16 parameters against the master's "
                     + ("high half (split rule)" if rec.split else "rounding"))
    for k, (src, dst) in enumerate(rec.copies):
        assert_exact(dst, src, f"{tag}: adapter copy {k}")
    for pname, was, now in rec.frozen:
        assert_exact(now, was, f"{tag}: frozen {pname}")
    return float(gnorm), coef


# =========================================================================== the reference as a trainer
DEFECTS = ("accum-divided-twice", "second-microbatch-overwrites", "stale-slot", "ignored-microbatch-counted",
           "norm-skips-embedding", "norm-of-unscaled-sum", "coef-not-clamped", "bias-correction-step-minus-one",
           "lr-of-previous-step", "weight-decay-as-l2", "pad-not-zero", "params-rne-not-split-rule",
           "adapter-buffer-stale", "zero3-scale-without-n", "zero3-replicated-unit-counted-world-times")
STALE_SLOT = "layers.1.wo.weight"


def start_params(c, dev="cpu"):
    """The bf16 values a case starts from: ``model_params``; ZeRO-3 seeds its own (``simulate`` / ``measure`` start
    from the same rule's values), each sharded unit's first slice tiled over an emulated world."""
    if c.zero3:  # what Zero3Trainer seeds (N(0, 0.02), every norm weight 1; the values of a CPU generator)
        from mxllm.parallel.zero3 import init_full_state

        named = init_full_state(LY.config(LY.MODEL_CASE), ZERO3_SEED, torch.device(dev))
    else:
        named = {k: v.to(dev) for k, v in LY.model_params(c.tied, c.lora).items()}
    if c.zero3 and c.world > 1:
        lay = sim_layout(c, {k: tuple(v.shape) for k, v in named.items()})
        named = {k: v.clone() for k, v in named_values(lay, flat_values(lay, named, BF16, dev)).items()}
    return named


@functools.lru_cache(maxsize=None)
def simulate(c, defect=None):
    """Three steps of the reference as a trainer: ([records], layout).  ``defect``: one of DEFECTS planted."""
    named = start_params(c)
    lay = sim_layout(c, {k: tuple(v.shape) for k, v in named.items()})
    gdt, world = accum_dtype(c), lay.world
    train = [k for k in named if LY.trainable(k, c.lora)]
    tlay = lay if not c.lora else sim_layout(c, {k: tuple(named[k].shape) for k in train})
    frozen0 = {k: v.clone() for k, v in named.items() if k not in train}
    state = (flat_values(tlay, named, F32, "cpu"), torch.zeros(tlay.numel), torch.zeros(tlay.numel))
    stored, recs, prevG = None, [], None
    pads = pad_mask(tlay, "cpu")
    for step in range(1, STEPS + 1):
        mbs = batches(c, step)
        n = len(mbs)
        _, _, outs = ref_loss_grads(c, named, mbs, loss_scale=1.0)
        per_mb = 1.0 if c.zero3 else 1.0 / n
        if defect == "accum-divided-twice":
            per_mb = per_mb / n
        G = torch.zeros(tlay.numel, dtype=F32 if c.zero3 else gdt)
        for k, o in enumerate(outs):
            g, _ = expected_buffer(c, tlay, {name: o[LY.param_key(name)] * per_mb for name in train}, 1, "cpu", False)
            if k == 0 or (defect == "second-microbatch-overwrites" and k == 1):
                G = g.to(gdt).to(G.dtype)
            elif c.zero3:  # the unit's gradient in its dtype, added into the fp32 shard
                G = (G.double() + g.to(gdt).double()).float()
            else:  # one rounding per added micro-batch
                G = (G.double() + g).to(gdt)
        if defect == "stale-slot" and prevG is not None:
            u, (_, off, k, _) = next((u, s) for u in tlay.units for s in u.slots if s[0] == STALE_SLOT)
            G[u.off + off:u.off + off + k] += prevG[u.off + off:u.off + off + k]
        if defect == "pad-not-zero":
            G[pads.nonzero()[3]] = 2.0 ** -20
        counted = [o for o in outs if o["losses"].numel()] if defect == "ignored-microbatch-counted" else outs
        loss = (sum(o["loss"] for o in outs) / len(counted)).float()
        scale = 1.0 / (world * (1 if defect == "zero3-scale-without-n" else n)) if c.zero3 else 1.0
        gnorm, _, after = adamw64(c, step, state, G, scale, defect, tlay)
        after = tuple(t.float() for t in after)
        stored = after[0].to(BF16) if defect == "params-rne-not-split-rule" else split_hi(after[0])
        # the next step starts from the state without the defect: every step's record shows the defect alone
        clean = tuple(t.float() for t in adamw64(c, step, state, G, 1.0 / (world * n) if c.zero3 else 1.0)[2])
        new = dict(named, **{k: v.clone() for k, v in named_values(tlay, split_hi(clean[0])).items()})
        copies = [(new[k], (named if defect == "adapter-buffer-stale" else new)[k]) for k in train] if c.lora else []
        recs.append(SimpleNamespace(step=step, mbs=mbs, params=named, loss=loss, G=G, scale=scale,
                                    gnorm=gnorm.float() if c.clip > 0 else None, before=state, after=after,
                                    stored=stored, split=True, copies=copies,
                                    frozen=[(k, v, new[k]) for k, v in frozen0.items()]))
        named, state, prevG = new, clean, G
    return recs, tlay


# =========================================================================== the trainers under test
def _spy(mp, obj, name, log, label):
    real = getattr(obj, name)
    mp.setattr(obj, name, lambda *a, _r=real, **k: (log.append((label, None)), _r(*a, **k))[1])


class _Run:
    """One trainer of case ``c`` on ``dev``: the same few reads for both trainer classes."""

    def __init__(self, c, dev, mp):
        from mxllm.models import Llama
        from mxllm.parallel import zero3
        from mxllm.parallel.runtime import DistEnv
        from mxllm.train.trainer import OptimConfig, Trainer

        self.c, self.dev, self.log = c, torch.device(dev), LY.apply_route(mp, "default", LY.MODEL_CASE, dev)
        for k in ("MXLLM_LORA_OVERLAP_ADAMW", "MXLLM_OVERLAP_ADAMW", "MXLLM_FRESH_GRADS", "MXLLM_FUSED_GRAD_NORM",
                  "MXLLM_NORM_OVERLAP", "MXLLM_SPLIT_MASTER", "MXLLM_ADAMW_LAG", "MXLLM_ADAMW_CUS",
                  "MXLLM_STEP_PRIORITY",
                  "MXLLM_Z3_ADAMW_OVERLAP", "MXLLM_Z3_RS_WIRE", "MXLLM_Z3_EMUL_ASYNC", "MXLLM_CE_FP32_LOGITS"):
            mp.delenv(k, raising=False)
        for k, v in c.env:
            mp.setenv(k, v)
        _spy(mp, LY._mod("mxllm.models.llama").ckpt, "checkpoint", self.log, "ckpt")
        _spy(mp, zero3._CkptLayer, "apply", self.log, "z3ckpt")
        opt = OptimConfig(grad_clip=c.clip, **OPT)
        env = DistEnv(device=self.dev, backend="nccl" if self.dev.type == "cuda" else "gloo")
        cfg = LY.config(LY.MODEL_CASE).replace(tie_embeddings=c.tied)
        if c.zero3:
            self.tr = zero3.Zero3Trainer(cfg, env, opt, seed=ZERO3_SEED, activation_checkpointing=c.ckpt,
                                         emulate_world=c.world if c.world > 1 else 0, grad_dtype=c.gdt)
            self.lay, self.model = layout_of_zero3(self.tr), self.tr.model
        else:
            m = Llama(cfg, device=self.dev, init=False, activation_checkpointing=c.ckpt, lora_r=c.lora,
                      lora_alpha=LY.S_LORA * c.lora if c.lora else 16.0)
            vals = LY.model_params(c.tied, c.lora)
            with torch.no_grad():
                for n, p in m.named_parameters():
                    p.copy_(vals[n])
                m.sync_adapters_()
                m.refresh_images_()
            self.model = m.train()
            self.tr = Trainer(m, env, opt, overlap_optimizer=c.overlap, grad_dtype=c.gdt)
            self.lay = layout_of_flat(self.tr.flat)
        self.frozen0 = {n: p.detach().clone() for n, p in self.model.named_parameters() if not p.requires_grad}
        self.check_path()

    # ---- the path the case is named for
    def check_path(self):
        c, tr, gpu = self.c, self.tr, self.dev.type == "cuda"
        self.path = {"overlap": tr.overlap_optimizer}  # what the spies saw, for the record
        if c.zero3:
            self.path.update(local=[u.local for u in tr.units], emulated=tr.emulated)
            assert tr.emulated == (c.world > 1) and tr.world == c.world
            assert all(u.local == (c.world == 1 or u.resident) for u in tr.units)
            assert tr.overlap_optimizer == gpu and tr.grad_dtype == (c.gdt or F32) and tr.split_master
            return
        # fresh gradients, the fused norm and the side streams are GPU-only
        assert tr.fresh_grads == (gpu and not c.lora and not c.tied), tr.fresh_grads
        lora_overlap = dict(c.env).get("MXLLM_LORA_OVERLAP_ADAMW") == "1"
        want_overlap = gpu and (c.overlap is not False) and (not c.lora or lora_overlap)
        assert tr.overlap_optimizer == want_overlap, tr.overlap_optimizer
        assert (getattr(tr, "_side", None) is not None) == want_overlap
        assert bool(tr._sq_params) == (tr.fresh_grads and c.clip > 0)
        assert (tr._chunk_copies is not None) == (want_overlap and bool(c.lora))
        assert tr.grad_dtype == accum_dtype(c) and isinstance(tr.flat.master, LY._mod("mxllm.ops").SplitMaster)
        self.path.update(fresh=tr.fresh_grads, sq_params=len(tr._sq_params), chunk_copies=tr._chunk_copies is not None)

    def check_step_path(self, n):
        """After the backwards of a step with ``n`` micro-batches."""
        c, tr, log = self.c, self.tr, self.log
        nck = 2 if c.ckpt is True else int(c.ckpt)
        got = (LY.count(log, "ckpt"), LY.count(log, "z3ckpt"))
        assert got == ((0, nck * n) if c.zero3 else (nck * n, 0)), (got, nck, n)
        self.path.setdefault("checkpoints", []).append(max(got))
        if c.zero3:
            return
        assert tr._sq_armed == (bool(tr._sq_params) and n == 1), tr._sq_armed
        self.path.setdefault("sq_armed", []).append(tr._sq_armed)
        self.path.setdefault("sq_done", []).append(
            sum(getattr(p, "_mx_sq_done", None) is True for p in self.model.parameters()))
        if tr._sq_armed and c.num == 1:  # MXLLM_GEMM8=all: the armed dW GEMMs took the fused path
            done = [k for k, p in self.model.named_parameters() if getattr(p, "_mx_sq_done", None) is True]
            assert any("wgu" in k for k in done) and any("wd" in k for k in done), done
            assert "tok_emb" not in done and tr._fused_sq() is not None, done

    # ---- reads
    def state(self):
        tr = self.tr
        tr.params_ready()
        master = tr.master if self.c.zero3 else tr.flat.master
        return master.float().clone(), tr.m.clone(), tr.v.clone()

    def stored(self):
        self.tr.params_ready()
        return (self.tr.shard_params if self.c.zero3 else self.tr.flat.params).clone()

    def params(self):
        """The bf16 values the next forward reads, by name (frozen weights included)."""
        if self.c.zero3:
            return {k: v.clone() for k, v in named_values(self.lay, self.stored()).items()}
        self.tr.params_ready()
        return {n: p.detach().clone() for n, p in self.model.named_parameters()}

    def copies(self):
        from mxllm.models.llama import FusedLinear

        self.tr.params_ready()
        return [pair for mod in self.model.modules() if isinstance(mod, FusedLinear) and mod.augmented()
                for pair in mod.adapter_copies()]

    def observed_step(self, step):
        """One step read from outside: the record ``check_step`` takes."""
        c, tr = self.c, self.tr
        mbs = batches(c, step, self.dev)
        n = len(mbs)
        params, before = self.params(), self.state()
        del self.log[:]
        if c.zero3:
            loss = tr.train_step(mbs)
            self.check_step_path(n)
            G, scale = tr.grads.clone(), 1.0 / (tr.world * n)  # kept: zero_grad=False
        else:
            total, scale = tr.compute_grads(mbs)
            self.check_step_path(n)
            tr.step_num += 1
            G = tr.flat.grads.clone()  # (fresh_grads off: AdamW clears the buffer)
            tr._optimizer_step(scale)
            loss = total / n
        assert tr.step_num == step
        gnorm = tr.last_grad_norm.clone() if c.clip > 0 else tr.last_grad_norm
        now = dict(self.model.named_parameters())
        return SimpleNamespace(step=step, mbs=mbs, params=params, loss=loss.detach().float().reshape(1), G=G,
                               scale=scale, gnorm=gnorm, before=before, after=self.state(), stored=self.stored(),
                               split=True, copies=self.copies(),
                               frozen=[(k, v, now[k].detach()) for k, v in self.frozen0.items()])


def run_case(c, dev, mp):
    """A case on ``dev``: three observed steps through ``check_step``, continuity between them, the case's own
    assertions, then the unobserved rerun.  Returns {"seen": the reference's [(gnorm, coef)] per step, "path": what
    the spies recorded}."""
    run = _Run(c, dev, mp)
    seen, losses, last = [], [], None
    for step in range(1, STEPS + 1):
        rec = run.observed_step(step)
        if last is not None:  # 6: nothing writes master / m / v between two steps
            for what, a, b in zip(("master", "m", "v"), last, rec.before):
                assert_exact(b, a, f"{case_id(c)}: {what} before step {step} against after step {step - 1}")
        seen.append(check_step(c, run.lay, rec))
        losses.append(rec.loss)
        last = rec.after
    if c.lora:
        assert run.copies() and all(not p.requires_grad for n, p in run.model.named_parameters() if "lora_" not in n)
    if c.num == 1:  # the clip coefficient below 1 at one step and exactly 1 at another
        assert min(co for _, co in seen) < 1.0 and max(co for _, co in seen) == 1.0, seen
    if any("Z" in p for p in c.plan):  # an all-ignored micro-batch: a finite loss, the others' mean over n
        assert all(bool(torch.isfinite(x).all()) for x in losses)
    # 7: the same three steps through plain train_step, nothing read in between
    again = _Run(c, dev, mp)
    plain = [again.tr.train_step(batches(c, step, dev)) for step in range(1, STEPS + 1)]
    for step, (a, b) in enumerate(zip(plain, losses), start=1):
        assert_exact(a.detach().float().reshape(1), b, f"{case_id(c)}: loss of step {step}, unobserved rerun")
    for what, a, b in zip(("master", "m", "v"), again.state(), last):
        assert_exact(a, b, f"{case_id(c)}: final {what}, unobserved rerun")
    return {"seen": seen, "path": run.path}


# =========================================================================== the measurements
def measure(cases=CASES, verbose=False):
    """The ``STEP_*_MEASURED`` constants (module doc).  STEP_LOSS by the standard-error rule of
    ``_layer_cases.measure_model``: three standard errors of the mean of means, relative to the loss."""
    from mxllm.ops import reference as ref_ops
    from tests.test_rowwise_strict_gpu import _meas

    acc, done = {}, set()
    for c in cases:
        key = (c.zero3, c.tied, c.lora, c.gdt, c.plan, c.clip, c.world)  # what the arithmetic depends on
        if key in done:
            continue
        done.add(key)
        recs, lay = simulate(c)
        gdt = accum_dtype(c)
        train = [k for k in recs[0].params if LY.trainable(k, c.lora)]
        for rec in recs:
            n = len(rec.mbs)
            _, grads64, outs64 = ref_loss_grads(c, rec.params, rec.mbs)
            _, _, outs32 = ref_loss_grads(c, rec.params, rec.mbs, F32, True, loss_scale=1.0 if c.zero3 else 1.0 / n)
            # the loss: per-token errors of every micro-batch, the mean of means' standard error
            var = sum(float((a["losses"].double() - b["losses"]).pow(2).mean()) / b["losses"].numel()
                      for a, b in zip(outs32, outs64) if b["losses"].numel())
            se = var ** 0.5 / n
            loss64 = float(sum(o["loss"] for o in outs64) / n)
            assert abs(float(sum(o["loss"] for o in outs32).double() / n) - loss64) < 3 * se
            acc["STEP_LOSS"] = (0.0, max(acc.get("STEP_LOSS", (0.0, 0.0))[1], 3 * se / loss64))
            # the buffer: one rounding per added micro-batch in the accumulation dtype
            for name in train:
                a32 = None
                for k, o in enumerate(outs32):
                    g = o[LY.param_key(name)]
                    if c.zero3 and gdt == BF16:  # bf16 unit gradients added into the fp32 shard
                        a32 = g.to(BF16).float() if a32 is None else a32 + g.to(BF16).float()
                    else:
                        a32 = g if a32 is None else a32.to(gdt).float() + g
                # (an emulated world: per parameter before the fold, whose bound is the sum of its slices' bounds)
                _meas(acc, "STEP_" + grad_bound_name(c, name, gdt), a32, grads64[name] * gmul(c, n), gdt)
            # AdamW: reference.adamw_ in fp32 with an fp32 norm against fp64 from the same state and buffer.  The
            # clip coefficient is ONE number per step, shared by every element: its fp32 error here is one draw, and
            # twice one draw bounds no other order of the same operations.  Six roundings of half an ulp lie between
            # the gradient and a clipped gscale (the sum of squares' own, the square root, the scale, + 1e-6, the
            # division, the scale again): the model is evaluated at gscale (1 +- 6 x 2^-24) as well.
            G, o = rec.G, OPT
            gn64, coef, want = adamw64(c, rec.step, rec.before, G, rec.scale)
            gs, wiggle = rec.scale, (1.0,)
            if c.clip > 0:
                gn = G.float().pow(2).sum().sqrt() * rec.scale
                gs = torch.clamp(c.clip / (gn + 1e-6), max=1.0) * rec.scale
                wiggle = (1.0, 1.0 + 6 * 2.0 ** -24, 1.0 - 6 * 2.0 ** -24) if coef < 1.0 else wiggle
            if verbose:
                print(f"# {case_id(c)} step {rec.step}: loss {loss64:.6f} clip norm {float(gn64):.4f} coef {coef:.4f}")
            for f in wiggle:
                p, m, v = [t.clone() for t in rec.before]
                ref_ops.adamw_(p, G, m, v, lr=lr_ref(rec.step), beta1=o["beta1"], beta2=o["beta2"], eps=o["eps"],
                               weight_decay=o["weight_decay"], step=rec.step, grad_scale=gs * f)
                for nm, got, w in zip("PMV", (p, m, v), want):
                    for _, lo, hi in _segments(lay):
                        _meas(acc, "STEP_ADAMW_" + nm, got[lo:hi], w[lo:hi], F32, "tensor")
    return acc


def new_constants(acc):
    """The measured constants that tests/_parity.py must hold: every STEP_* one but the gradient constants that came
    out no larger than the MODEL_* constant of the same kind (which is then the bound)."""
    out = {}
    for name, (rel, ab) in acc.items():
        old = getattr(P, "MODEL_" + name[5:] + "_MEASURED", None)
        if old is not None and name != "STEP_LOSS" and float(f"{ab:.3g}") <= old[1] and float(f"{rel:.3g}") <= old[0]:
            continue
        out[name] = (rel, ab)
    return out


def main():
    acc = measure(verbose=True)
    keep = new_constants(acc)
    for name, (rel, ab) in sorted(acc.items()):
        print(f"{name}_MEASURED = ({rel:.3g}, {ab:.3g})" + ("" if name in keep else f"  # <= MODEL_{name[5:]}: reused"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
