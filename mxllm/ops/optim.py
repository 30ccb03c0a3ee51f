"""Fused AdamW over flat parameter buffers.

mxllm keeps every trainable parameter as a view into ONE flat fp32 master
buffer (and, for full fine-tuning, one flat bf16 compute buffer); gradients
land in one flat buffer too.  The optimizer step is therefore a single
vectorised HIP kernel launch per weight-decay group, streaming
(master, m, v, grad[, bf16 copy]) once: 16-28 B/param, HBM-bound.  With the
moments in fp8 (:class:`QuantMoment`, ``adamw8_kernel``): 14-16 B/param.
"""
from __future__ import annotations

import torch

from . import reference as ref
from ._ext import native, use_native


class SplitMaster:
    """fp32 master weights stored as two 16-bit halves of their bit pattern:
    ``hi`` — the bf16 COMPUTE weights themselves (the master rounded half-up on its
    bits) — and ``lo`` (int16) = master bits - (hi << 16), which always fits.  The
    fp32 value is reconstructed exactly, so the optimizer arithmetic is that of an
    fp32 master; the separate bf16 copy disappears: 2 B/param less optimizer state
    (8B full fine-tune: 16 GB; a 70B ZeRO-3 rank at world 8: 17.6 GB) and 2 B/param
    less AdamW traffic.  Only exact ties round differently from round-to-nearest-even.

    Behaves like a 1-D fp32 tensor where the framework needs one: slicing (views of
    both halves), ``copy_`` (split), ``zero_``, and ``float()`` / ``detach()`` /
    ``contiguous()`` / ``cpu()`` / ``clone()`` / ``view()`` (a materialised fp32
    copy, for checkpoints, tests and export)."""

    dtype = torch.float32

    def __init__(self, hi: torch.Tensor, lo: torch.Tensor | None = None):
        self.hi = hi
        self.lo = lo if lo is not None else torch.zeros(hi.shape, dtype=torch.int16, device=hi.device)

    @property
    def device(self):
        return self.hi.device

    @property
    def shape(self):
        return self.hi.shape

    @property
    def is_cuda(self):
        return self.hi.is_cuda

    def numel(self) -> int:
        return self.hi.numel()

    def element_size(self) -> int:
        return 4

    def storage_offset(self) -> int:
        return self.hi.storage_offset()

    def __getitem__(self, sl):
        return SplitMaster(self.hi[sl], self.lo[sl])

    def float(self) -> torch.Tensor:
        out = torch.empty(self.hi.shape, dtype=torch.float32, device=self.hi.device)
        if use_native(self.hi) and self.hi.is_contiguous() and self.lo.is_contiguous():
            native().join_master(self.hi, self.lo, out)
            return out
        b = (self.hi.view(torch.int16).to(torch.int64) & 0xFFFF) << 16
        b = (b + self.lo.to(torch.int64)) & 0xFFFFFFFF
        b = torch.where(b >= 2 ** 31, b - 2 ** 32, b)
        out.copy_(b.to(torch.int32).view(torch.float32))
        return out

    def detach(self):
        return self.float()

    contiguous = clone = detach

    def cpu(self):
        return self.float().cpu()

    def view(self, *shape):
        return self.float().view(*shape)

    def zero_(self):
        self.hi.zero_()
        self.lo.zero_()
        return self

    def copy_(self, src: torch.Tensor):
        x = src.to(device=self.hi.device, dtype=torch.float32).reshape(self.hi.shape).contiguous()
        if use_native(self.hi) and self.hi.is_contiguous() and self.lo.is_contiguous():
            native().split_master(x, self.hi, self.lo)
            return self
        b = x.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
        h = ((b + 0x8000) >> 16) & 0xFFFF
        lo = b - (h << 16)
        lo = torch.where(lo >= 2 ** 31, lo - 2 ** 32, lo)  # h << 16 wrapped past 2^32 (negative numbers)
        self.lo.copy_(lo.to(torch.int16))
        self.hi.view(torch.int16).copy_(torch.where(h >= 2 ** 15, h - 2 ** 16, h).to(torch.int16))
        return self


class QuantMoment:
    """One AdamW moment of a flat buffer in 8 bits (2 + 1/32 B/param for both moments instead of 8).

    Format (``mxllm/ops/reference.py`` ``q8_*`` define it, ``adamw8_kernel`` implements it): a block is 64
    consecutive elements of the FLAT buffer; ``codes`` uint8 [n] are OCP e4m3 codes and ``exps`` int8 [n / 64]
    one power-of-two exponent per block, value = e4m3(code) 2^e, e the smallest with amax / 2^e <= 448 (at least
    -100; 0 for an all-zero block).  ``sqrt=True`` (the second moment): the stored quantity is s = sqrt(v) --
    e4m3 spans 2^18 inside a block, which as v would leave the denominators a range of 500 -- and a positive s
    is stored no smaller than the smallest subnormal, so an update never divides by a flushed zero.  The
    optimizer step rounds STOCHASTICALLY (to-nearest would return sqrt(v) to its old code every step: a 0.1 %
    change against a 6 % spacing) with bits hashed from (``seed``, step, moment, global element index
    ``base`` + i), so the result does not depend on the grid, the chunking or the rank that holds the element.

    Where the trainers need it, it stands in for a 1-D fp32 tensor: slicing on block boundaries (views; ``base``
    follows), ``numel``, ``zero_``, ``float()`` (the decoded fp32 moment: v = s^2 when ``sqrt``) and ``copy_``
    (from a QuantMoment: codes and exponents as they are; from fp32: round to NEAREST, so a loaded checkpoint is
    deterministic).  Accuracy on real checkpoints has not been measured."""

    BLOCK = ref.Q8_BLOCK
    dtype = torch.float32

    def __init__(self, codes: torch.Tensor, exps: torch.Tensor | None = None, *, sqrt: bool = False, seed: int = 0,
                 base: int = 0):
        if codes.dtype != torch.uint8 or codes.dim() != 1 or codes.numel() % self.BLOCK or base % self.BLOCK:
            raise ValueError("QuantMoment: uint8 codes of whole 64-element blocks starting on a block boundary")
        self.codes = codes
        self.exps = exps if exps is not None else torch.zeros(codes.numel() // self.BLOCK, dtype=torch.int8,
                                                              device=codes.device)
        if self.exps.dtype != torch.int8 or self.exps.numel() != codes.numel() // self.BLOCK:
            raise ValueError("QuantMoment: one int8 exponent per 64 codes")
        self.sqrt, self.seed, self.base = sqrt, int(seed), int(base)

    @classmethod
    def zeros(cls, n: int, device=None, **kw):
        return cls(torch.zeros(n, dtype=torch.uint8, device=device), **kw)

    @property
    def device(self):
        return self.codes.device

    @property
    def shape(self):
        return self.codes.shape

    @property
    def is_cuda(self):
        return self.codes.is_cuda

    def numel(self) -> int:
        return self.codes.numel()

    def __getitem__(self, sl):
        if not isinstance(sl, slice) or sl.step not in (None, 1):
            raise ValueError("QuantMoment: contiguous slices only")
        lo, hi, _ = sl.indices(self.numel())
        if lo % self.BLOCK or hi % self.BLOCK:
            raise ValueError(f"QuantMoment: slice [{lo}, {hi}) does not lie on 64-element block boundaries")
        return QuantMoment(self.codes[lo:hi], self.exps[lo // self.BLOCK:hi // self.BLOCK], sqrt=self.sqrt,
                           seed=self.seed, base=self.base + lo)

    def at(self, base: int):
        """The same storage as the elements [base, base + n) of the flat buffer (a rank's compact shard)."""
        return QuantMoment(self.codes, self.exps, sqrt=self.sqrt, seed=self.seed, base=base)

    def float(self) -> torch.Tensor:
        x = ref.q8_decode(self.codes, self.exps)
        return x * x if self.sqrt else x

    def zero_(self):
        self.codes.zero_()
        self.exps.zero_()
        return self

    def copy_(self, src):
        if isinstance(src, QuantMoment):
            if src.sqrt != self.sqrt:
                raise ValueError("QuantMoment.copy_: one holds sqrt(v), the other does not")
            self.codes.copy_(src.codes)
            self.exps.copy_(src.exps)
            return self
        x = src.to(device=self.codes.device, dtype=torch.float32).reshape(self.codes.shape)
        ref.q8_encode_(self.codes, self.exps, x.sqrt() if self.sqrt else x, floor_min=(x > 0) if self.sqrt else None)
        return self


def copy_moment_(dst, src) -> None:
    """``dst.copy_(src)`` for any pairing of fp32 and fp8 optimizer state (checkpoints written with the other
    setting): fp8 -> fp32 decodes, fp32 -> fp8 rounds to nearest, fp8 -> fp8 copies codes and exponents."""
    dst.copy_(src.float() if isinstance(src, QuantMoment) and not isinstance(dst, QuantMoment) else src)


def adamw_step_(master, grad: torch.Tensor, m, v, lowp: torch.Tensor | None, *, lr: float, beta1: float,
                beta2: float, eps: float, weight_decay: float, step: int, grad_scale=1.0,
                zero_grad: bool = False) -> None:
    """In-place AdamW on flat 1-D tensors (``grad`` fp32 or bf16).

    ``master``: an fp32 tensor (``lowp``: optional bf16 copy to refresh) or a
    :class:`SplitMaster` (its ``hi`` half IS the bf16 copy; ``lowp`` ignored).
    ``m`` / ``v``: fp32 tensors, or two :class:`QuantMoment` (``v`` with ``sqrt=True``): fp8 state.
    ``grad_scale`` is a float or a 1-element f32 device tensor (e.g. the
    grad-clip coefficient x 1/world computed on device: no host sync).
    ``zero_grad``: clear ``grad`` in the same pass (GPU: fused into the kernel)."""
    split = isinstance(master, SplitMaster)
    quant = isinstance(m, QuantMoment)
    if quant != isinstance(v, QuantMoment) or (quant and (m.sqrt or not v.sqrt or m.numel() != v.numel()
                                                          or m.base != v.base or m.seed != v.seed)):
        raise ValueError("adamw_step_: fp8 state needs m = QuantMoment and v = QuantMoment(sqrt=True) of one range")
    if quant and use_native(m.codes):
        if isinstance(grad_scale, torch.Tensor):
            st, sf = grad_scale.reshape(1).float().contiguous(), 1.0
        else:
            st, sf = None, float(grad_scale)
        native().adamw8_step(None if split else master, grad, m.codes, m.exps, v.codes, v.exps,
                             master.hi if split else lowp, master.lo if split else None, lr, beta1, beta2, eps,
                             weight_decay, 1.0 - beta1 ** step, 1.0 - beta2 ** step, st, sf, bool(zero_grad),
                             ref.q8_key(m.seed, step), m.base)
        return
    if quant:
        p = master.float() if split else master
        ref.adamw8_(p, grad, m.codes, m.exps, v.codes, v.exps, lr=lr, beta1=beta1, beta2=beta2, eps=eps,
                    weight_decay=weight_decay, step=step, grad_scale=grad_scale, p_lowp=None if split else lowp,
                    seed=m.seed, base=m.base)
        if split:
            master.copy_(p)
        if zero_grad:
            grad.zero_()
        return
    if use_native(m):
        bc1 = 1.0 - beta1 ** step
        bc2 = 1.0 - beta2 ** step
        if isinstance(grad_scale, torch.Tensor):
            st, sf = grad_scale.reshape(1).float().contiguous(), 1.0
        else:
            st, sf = None, float(grad_scale)
        if split:
            native().adamw_step(None, grad, m, v, master.hi, master.lo, lr, beta1, beta2, eps, weight_decay, bc1,
                                bc2, st, sf, bool(zero_grad))
        else:
            native().adamw_step(master, grad, m, v, lowp, None, lr, beta1, beta2, eps, weight_decay, bc1, bc2, st,
                                sf, bool(zero_grad))
        return
    p = master.float() if split else master
    ref.adamw_(p, grad, m, v, lr=lr, beta1=beta1, beta2=beta2, eps=eps, weight_decay=weight_decay,
               step=step, grad_scale=grad_scale, p_lowp=None if split else lowp)
    if split:
        master.copy_(p)
    if zero_grad:
        grad.zero_()


def sq_norm(x: torch.Tensor) -> torch.Tensor:
    """sum(x^2) as a 1-element fp32 tensor (no host sync).  GPU: one read of x
    (f32 or bf16) with a fixed-order reduction, so every DDP replica computes the
    bitwise-same clip coefficient."""
    if use_native(x) and x.dtype in (torch.float32, torch.bfloat16) and x.is_contiguous():
        return native().sqnorm(x)
    return x.float().pow(2).sum().reshape(1)
