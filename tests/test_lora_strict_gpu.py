"""Strict tests of the LoRA training path on the GPU (cases, references and checks: tests/_lora_cases.py).

A. ``swiglu_lora`` (csrc/kernels/lora.hip swiglu_lora_kernel + swiglu_lora_reduce_kernel), every
   <BWD, NRB, RBW> instantiation with several trips per workgroup and uneven splits: the elementwise half
   bitwise the plain SwiGLU kernels', one-hot and one-per-split V rows exact, Gaussian V per element against
   fp64, bit-reproducible; and every operand refusal of the op.
B. The LoRA projection as a layer (FusedLinear in its three layouts -> _LoRAAugFn / _lora_aug_backward, HIP
   rank-r kernels and hipBLASLt fallback products, gradients to autograd and into pre-attached buffers,
   after an adapter update) and the LoRA MLP block with and without producer-written tails, every element
   of y, dx, dA and the diagonal dB_i against plain fp64.

``python -m tests.test_lora_strict_gpu`` prints the CPU measurements behind the bounds of tests/_parity.py
(no GPU needed); tests/test_lora_cases.py runs the same checks on the CPU.
"""
import importlib
import sys

import pytest
import torch

from tests import _lora_cases as LC

pytestmark = pytest.mark.gpu


def _ops():
    from mxllm.ops import native

    return native()


def native_tail(dm, gu, pad, v, nrb, s):
    """The op's [T, W] result widened to its whole [T, W + pad] buffer."""
    from mxllm.ops.linear import _padded_rows

    out = _ops().swiglu_lora(dm, gu, pad, v, nrb, s)
    full = _padded_rows(out, pad)
    assert full is not None, "swiglu_lora: the result is not the left part of a [T, W + pad] buffer"
    return full


def native_plain(dm, gu):
    return _ops().swiglu_fwd(gu, 0) if dm is None else _ops().swiglu_bwd(dm, gu, 0)


def set_env(monkeypatch, env):
    for k, v in env.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)


# =========================================================================== A
@pytest.mark.parametrize("case", LC.TAIL_CASES, ids=LC.tail_id)
def test_swiglu_lora_strict(gpu, case, monkeypatch):
    set_env(monkeypatch, LC.tail_env(case))  # read by the launcher at every call
    LC.check_tail_case(case, native_tail, native_plain, gpu)


@pytest.mark.parametrize("rid", list(LC.REFUSALS))
def test_swiglu_lora_refusals(gpu, rid):
    LC.check_tail_refusal(rid, native_tail, gpu, pytest.raises)


# =========================================================================== B
def _lin_module():
    return importlib.import_module("mxllm.ops.linear")  # (the mxllm.ops attributes are the functions)


class XwtSpy:
    """torch.ops.mxllm with a counter of lora_xwt look-ups (one per call)."""

    def __init__(self, real):
        self.real, self.xwt, self.grads = real, 0, 0

    def __getattr__(self, k):
        if k == "lora_xwt":
            self.xwt += 1
        if k == "lora_grads":
            self.grads += 1
        return getattr(self.real, k)


def spy_on(monkeypatch):
    Lin = _lin_module()
    spy = XwtSpy(Lin.native())
    monkeypatch.setattr(Lin, "native", lambda: spy)
    return spy


@pytest.mark.parametrize("wt", ["0", "1"])
@pytest.mark.parametrize("fused", ["0", "1"])
@pytest.mark.parametrize("acc", [False, True], ids=["fresh", "accumulate"])
@pytest.mark.parametrize("K,splits,r", LC.GRADS_TAIL_END_CONFIGS)
def test_lora_grads_rank_blocks_at_the_tail_end_exact(gpu, K, splits, r, acc, fused, wt, monkeypatch):
    """Splits whose rank blocks end with the 64-column tail (two splits of r = 32: the second split's blocks
    are columns 32..63, so a 64-column window from its first block would leave the tail): integer operands,
    exact, as tests/test_mfma_exact_gpu.py ``test_lora_grads_integer_exact``.  ``lora_grads`` refused this
    layout before the projection tests below reached it."""
    from tests import test_mfma_exact_gpu as TE

    monkeypatch.setenv("MXLLM_LORA_FUSED_RED", fused)
    monkeypatch.setenv("MXLLM_LORA_XTG_WT", wt)
    monkeypatch.setenv("MXLLM_LORA_XTG_WT_MIN", "4")
    TE.check_lora_grads(K, splits, r, acc, lambda *a: _ops().lora_grads(*a), gpu)


@pytest.mark.parametrize("acc", [False, True], ids=["autograd", "accumulate"])
@pytest.mark.parametrize("kernels", [True, False], ids=["hip", "fallback"])
@pytest.mark.parametrize("layout", LC.LAYOUTS)
@pytest.mark.parametrize("case", LC.PROJ_CASES, ids=LC.proj_id)
def test_lora_projection_fp64(gpu, case, layout, kernels, acc, monkeypatch):
    monkeypatch.setattr(_lin_module(), "_LORA_KERNELS", kernels)
    spy = spy_on(monkeypatch)
    LC.check_projection(case, layout, acc, gpu)
    # the rank-r products ran where the test says they ran: two tails and one gradient launch on the HIP
    # kernels (T % 64 == 0), none otherwise
    want = (2, 1) if kernels and case.T % 64 == 0 else (0, 0)
    assert (spy.xwt, spy.grads) == want, (spy.xwt, spy.grads)


@pytest.mark.parametrize("kernels", [True, False], ids=["hip", "fallback"])
@pytest.mark.parametrize("layout", LC.LAYOUTS)
@pytest.mark.parametrize("case", [LC.PROJ_CASES[0], LC.PROJ_CASES[3]], ids=LC.proj_id)
def test_lora_projection_after_adapter_update(gpu, case, layout, kernels, monkeypatch):
    """New adapter values and ``sync_adapter_()`` alone: a stale wbuf, wbt, wa or wxt column fails per element."""
    monkeypatch.setattr(_lin_module(), "_LORA_KERNELS", kernels)
    LC.check_projection(case, layout, False, gpu, update=True)
    LC.check_projection(case, layout, True, gpu, update=True)


@pytest.mark.parametrize("fused", [True, False], ids=["fused-tails", "unfused"])
@pytest.mark.parametrize("case", LC.MLP_CASES, ids=LC.mlp_id)
def test_lora_mlp_block_fp64(gpu, case, fused, monkeypatch):
    """The fused form takes the producer-written tails (two lora_xwt calls: the gate-up input's and the down
    output gradient's), the unfused one recomputes all four; each against fp64."""
    A = importlib.import_module("mxllm.ops.activation")
    monkeypatch.setattr(A, "_FUSE_TAIL", fused)
    spy = spy_on(monkeypatch)
    outs, wrote = LC.run_mlp(case, gpu)
    assert wrote == (fused, fused)
    assert spy.xwt == (2 if fused else 4), spy.xwt
    LC.check_mlp_outputs(case, outs, f"mlp {LC.mlp_id(case)} {'fused' if fused else 'unfused'}")


def main():
    for name, (rel, ab) in sorted(LC.measure().items()):
        print(f"{name}_MEASURED = ({rel:.3g}, {ab:.3g})")
    return 0


if __name__ == "__main__":
    sys.exit(main())
