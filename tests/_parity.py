"""Per-element parity check for kernel outputs against an fp64 reference.

One global norm ratio (``|a - b| / |b| < 1e-2`` on Gaussian data) cannot see a wrong 8-column
chunk, a wrong row of a partially filled last block or one element missed by a second grid pass:
each moves the ratio by a fraction of itself.  ``assert_parity`` bounds every element instead:

    |out - ref| <= c_rel * |ref| + c_abs * scale

``scale`` is the max |ref| of the element's row (last dimension) or of the whole tensor.  The
absolute term is there because some outputs cancel (RMSNorm dx, the cross-entropy gradient p - 1,
the RoPE rotation): their error is relative to the operands, not to the result.

How the constants below were chosen (none comes from a kernel):

  * On the CPU, at the inputs the GPU tests use (``tests/test_rowwise_strict_gpu.py`` builds them
    on the CPU from a fixed seed), the plain fp32 PyTorch expression of the operation
    (``mxllm/ops/reference.py`` and the ``*_fp32`` functions of the test module) is compared with
    the fp64 reference computed from the same rounded inputs:
        abs = max |y32 - ref| / scale               the fp32 arithmetic, before the output rounding
        rel = max |round(y32) - y32| / |y32|        the rounding to the output dtype
    (max over every case of that output, rel over the elements that are normal numbers in the
    output dtype; ``python -m tests.test_rowwise_strict_gpu`` prints them again, no GPU needed.)
  * The bound allows twice each: a different but equally valid fp32 operation order, fused
    multiply-adds and the hardware rcp / exp2 / rsq approximations move a result by about as much
    as the fp32 expression itself is off, and may flip the output rounding of an element.
  * c_rel never falls below one ulp of the output dtype (2^-7 bf16, 2^-23 fp32).

Each output has ``<NAME>_MEASURED = (rel, abs)`` and ``<NAME> = (c_rel, c_abs)`` side by side.
"""
from __future__ import annotations

import torch

ULP_BF16 = 2.0 ** -7
ULP_F32 = 2.0 ** -23


# --------------------------------------------------------------------------- constants
# <NAME>_MEASURED = (rel, abs), measured on the CPU as described above;
# <NAME> = (c_rel, c_abs) = (max(2 rel, one ulp), 2 abs): the bound of the GPU tests.
RMSNORM_Y_MEASURED = (0.00389, 1.74e-07)
RMSNORM_Y = (ULP_BF16, 3.48e-07)  # 2 x 0.00389 < one ulp; 2 x 1.74e-07
RMSNORM_RSTD_MEASURED = (0, 1.23e-07)
RMSNORM_RSTD = (ULP_F32, 2.46e-07)  # 2 x 0 < one ulp; 2 x 1.23e-07
RMSNORM_DX_MEASURED = (0.00389, 1.3e-07)
RMSNORM_DX = (ULP_BF16, 2.6e-07)  # 2 x 0.00389 < one ulp; 2 x 1.3e-07
RMSNORM_DW_MEASURED = (0, 1.71e-07)
RMSNORM_DW = (ULP_F32, 3.42e-07)  # 2 x 0 < one ulp; 2 x 1.71e-07
SWIGLU_M_MEASURED = (0.00387, 1.21e-07)
SWIGLU_M = (ULP_BF16, 2.42e-07)  # 2 x 0.00387 < one ulp; 2 x 1.21e-07
SWIGLU_DGU_MEASURED = (0.00389, 3.8e-07)
SWIGLU_DGU = (ULP_BF16, 7.6e-07)  # 2 x 0.00389 < one ulp; 2 x 3.8e-07
CE_LOSSES_MEASURED = (0, 7.01e-08)
CE_LOSSES = (ULP_F32, 1.4e-07)  # 2 x 0 < one ulp; 2 x 7.01e-08
CE_GRAD_MEASURED = (0.00389, 2.31e-07)
CE_GRAD = (ULP_BF16, 4.62e-07)  # 2 x 0.00389 < one ulp; 2 x 2.31e-07
CE_MEAN_MEASURED = (0, 1.63e-07)
CE_MEAN = (ULP_F32, 3.26e-07)  # 2 x 0 < one ulp; 2 x 1.63e-07
ADAMW_P_MEASURED = (0, 9.16e-08)
ADAMW_P = (ULP_F32, 1.83e-07)  # 2 x 0 < one ulp; 2 x 9.16e-08
ADAMW_M_MEASURED = (0, 7.3e-08)
ADAMW_M = (ULP_F32, 1.46e-07)  # 2 x 0 < one ulp; 2 x 7.3e-08
ADAMW_V_MEASURED = (0, 6.75e-08)
ADAMW_V = (ULP_F32, 1.35e-07)  # 2 x 0 < one ulp; 2 x 6.75e-08
ROPE_QK_MEASURED = (0.00389, 1.18e-07)
ROPE_QK = (ULP_BF16, 2.36e-07)  # 2 x 0.00389 < one ulp; 2 x 1.18e-07
ROPE_DQKV_MEASURED = (0.00389, 2.08e-07)
ROPE_DQKV = (ULP_BF16, 4.16e-07)  # 2 x 0.00389 < one ulp; 2 x 2.08e-07
EMBEDDING_DW_MEASURED = (0, 5.12e-08)
EMBEDDING_DW = (ULP_F32, 1.02e-07)  # 2 x 0 < one ulp; 2 x 5.12e-08


def assert_parity(out: torch.Tensor, ref: torch.Tensor, bound, *, scale: str = "row", name: str = "") -> None:
    """Assert ``|out - ref| <= c_rel |ref| + c_abs scale`` for every element.

    ``out``: the kernel's output (any float dtype).  ``ref``: the fp64 reference, same shape, same
    device.  ``bound``: ``(c_rel, c_abs)``.  ``scale``: ``"row"`` (max |ref| over the last dimension)
    or ``"tensor"``.  A non-finite ``out`` element fails.  On failure the message names the worst
    element (largest excess over its bound), both values there, and how many elements exceed the
    bound -- which localizes a wrong chunk, row or block."""
    c_rel, c_abs = bound
    assert ref.dtype == torch.float64, "the reference must be fp64"
    assert tuple(out.shape) == tuple(ref.shape), f"{name}: shape {tuple(out.shape)} vs reference {tuple(ref.shape)}"
    if ref.numel() == 0:
        return
    o = out.detach().to(torch.float64)
    r = ref.detach()
    if scale == "row":
        s = r.abs().amax(dim=-1, keepdim=True)
    elif scale == "tensor":
        s = r.abs().max()
    else:
        raise ValueError(scale)
    err = (o - r).abs()
    lim = c_rel * r.abs() + c_abs * s
    bad = ~(err <= lim)  # NaN compares false: counted
    nbad = int(bad.sum())
    if nbad == 0:
        return
    excess = torch.where(torch.isfinite(err), err - lim, torch.full_like(err, float("inf")))
    flat = int(excess.reshape(-1).argmax())
    idx = []
    for d in reversed(o.shape):
        idx.append(flat % d)
        flat //= d
    idx = tuple(reversed(idx))
    first = tuple(int(i) for i in bad.nonzero()[0])
    raise AssertionError(
        f"{name or 'output'}: {nbad} of {o.numel()} elements exceed |out - ref| <= {c_rel:.3g} |ref| + "
        f"{c_abs:.3g} {scale}-max; worst at {idx}: out {o[idx].item():.9g}, ref {r[idx].item():.9g}, "
        f"|diff| {err[idx].item():.3g} > bound {lim.expand_as(err)[idx].item():.3g}; first at {first}")

