"""MXFP4 projection weights on the GPU: csrc/kernels/mxfp4_gemm.hip through ``w4_dequant`` / ``w4_linear``
and the serving engine over ``W4Linear`` projections.  The checks are those of tests/_mxfp4.py;
tests/test_mxfp4_cpu.py runs each of them with the Python reference in place of the HIP op.

Every dequantised weight is exactly a bf16 number (mxllm/serve/quant.py), so:

* ``w4_dequant`` is compared bit for bit, for all 16 codes x scale bytes 1..254 x both nibble positions;
* with magnitude codes 1..4, scale bytes 125..129 and integer |x| <= 3 every partial sum of ``w4_linear``
  is an integer multiple of 2^-3 below 2^24 * 2^-3: the output is the bf16 rounding of the fp64 product
  whatever the summation order (assert_exact);
* Gaussian inputs are bounded per element against the fp64 product with the reference-decoded weights.

W4_Y / W4_DEQ_Y were obtained as tests/_parity.py describes: the fp32 CPU expression against fp64 at these
inputs, doubled, c_rel at least one bf16 ulp.  ``python -m tests.test_mxfp4_gpu`` prints the measurement
(no GPU needed).
"""
import sys

import pytest
import torch

from tests import _mxfp4 as X
from tests._parity import ULP_BF16

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16

# <NAME>_MEASURED = (rel, abs) on the CPU; <NAME> = (max(2 rel, one ulp), 2 abs)
W4_Y_MEASURED = (0.00389, 2.15e-07)
W4_Y = (ULP_BF16, 4.3e-07)  # 2 x 0.00389 < one ulp; 2 x 2.15e-07
W4_DEQ_Y_MEASURED = (0.00389, 9.67e-08)
W4_DEQ_Y = (ULP_BF16, 1.93e-07)  # 2 x 0.00389 < one ulp; 2 x 9.67e-08

STREAM_M = 64  # the cap the multi-pass tests pass to w4_linear

# (M, N, K, MXLLM_W4_NC, the launcher branch <token blocks MB, K-splitting waves NW, channel groups NC>).
# K: 512 -> four waves, one chunk each; 4608 -> four waves, nine chunks each (two batches of four and a
# single one); 1024 / 5120 -> eight waves, one chunk / a batch and a single one; 1536 -> four waves,
# three chunks (no whole batch: the batch of two and a single one).
# N: 96 -> six workgroups; 1040 -> N % 32 != 0, one group per wave whatever is asked; 8192 -> the default
# takes two groups from 3 rows on (256 workgroups of 32 channels), one below.
W4_CASES = []
for _K in (512, 4608):
    for _M, _mb in ((1, 1), (16, 1), (17, 2), (32, 2)):
        W4_CASES += [(_M, 96, _K, "", f"<{_mb}, 4, 1>"), (_M, 1040, _K, "", f"<{_mb}, 4, 1>"),
                     (_M, 8192, _K, "", f"<{_mb}, 4, {1 if _M < 3 else 2}>")]
for _K, _nw in ((1024, 8), (5120, 8), (1536, 4)):
    W4_CASES += [(1, 1040, _K, "", f"<1, {_nw}, 1>"), (17, 1040, _K, "", f"<2, {_nw}, 1>")]
# one case per forced variant (N = 8192: 128 workgroups of 64 channels, the least the switch accepts)
for _nc in ("1", "2", "4"):
    W4_CASES += [(16, 8192, 4608, _nc, f"<1, 4, {_nc}>"), (32, 8192, 5120, _nc, f"<2, 8, {_nc}>"),
                 (5, 8192, 1024, _nc, f"<1, 8, {_nc}>")]
W4_CASES += [(17, 8192, 512, "4", "<2, 4, 4>")]
# 33 .. stream_m rows: passes over 32-row slices (a one-row last pass; two whole passes)
W4_PASSES = [(33, 1040, 512), (64, 96, 4608)]
# more rows than stream_m; K % 512 != 0 (at one row and at many): dequantise + bf16 GEMM
W4_FALLBACK = [(65, 1040, 512), (4, 96, 768), (40, 96, 1280)]


def w4_id(case):
    M, N, K, nc, _ = case
    return f"{M}-{N}-{K}" + (f"-nc{nc}" if nc else "")


def _ops():
    from mxllm.ops import native

    return native()


def _linear(x, codes, scales):
    return _ops().w4_linear(x, codes, scales, STREAM_M)


def test_w4_dequant_every_code_every_scale(gpu):
    X.check_every_code(_ops().w4_dequant, gpu)


@pytest.mark.parametrize("kind", ["int", "gauss"])
@pytest.mark.parametrize("case", W4_CASES, ids=w4_id)
def test_w4_linear_every_branch(gpu, case, kind, monkeypatch):
    M, N, K, nc, _ = case
    monkeypatch.setenv("MXLLM_W4_NC", nc)
    X.check_linear(kind, M, N, K, _linear, gpu, W4_Y)


@pytest.mark.parametrize("kind", ["int", "gauss"])
@pytest.mark.parametrize("M,N,K", W4_PASSES)
def test_w4_linear_passes(gpu, M, N, K, kind):
    assert 32 < M <= STREAM_M
    X.check_linear(kind, M, N, K, _linear, gpu, W4_Y)


@pytest.mark.parametrize("M,N,K", W4_FALLBACK)
def test_w4_linear_fallback_parity(gpu, M, N, K):
    assert M > STREAM_M or K % 512
    X.check_fallback(M, N, K, _linear, _ops().w4_dequant, gpu, W4_DEQ_Y)


def test_w4_linear_refuses_foreign_operands(gpu):
    x, codes, scales, _ = X.linear_case("gauss", 4, 96, 512)
    ops = _ops()
    with pytest.raises(RuntimeError):
        ops.w4_linear(x.to(gpu), codes.to(gpu)[:, :128], scales.to(gpu), STREAM_M)  # codes not contiguous
    with pytest.raises(RuntimeError):
        ops.w4_linear(x.to(gpu), codes.to(gpu), scales.to(gpu)[:, :8].contiguous(), STREAM_M)  # a scale short
    with pytest.raises(RuntimeError):
        ops.w4_linear(x.to(gpu)[:, :256].contiguous(), codes.to(gpu), scales.to(gpu), STREAM_M)  # K of x
    with pytest.raises(RuntimeError):
        ops.w4_linear(x.float().to(gpu), codes.to(gpu), scales.to(gpu), STREAM_M)


def test_w4_module_routes_to_the_kernel(gpu):
    """W4Linear.forward on the GPU is w4_linear with the module's STREAM_M, bit for bit, for a strided
    3-D input."""
    from mxllm.serve import quant

    x, codes, scales, _ = X.linear_case("gauss", 16, 1040, 512)
    lin = quant.W4Linear(codes=codes, scales=scales).to(gpu)
    xd = X.strided(x, 24, 0, gpu)
    y = lin(xd.view(2, 8, 512))
    assert y.shape == (2, 8, 1040)
    want = _ops().w4_linear(xd, lin.codes, lin.scales, quant.STREAM_M)
    assert torch.equal(X.bits(y.view(16, 1040).cpu()), X.bits(want.cpu()))


def test_engine_mxfp4_prefill_and_graphed_decode(gpu):
    X.check_engine(gpu, expect_graphs=True)


# --------------------------------------------------------------------------- measurement (CPU)
def measure():
    """fp32 ``x.float() @ w.t()`` against fp64 at the Gaussian inputs above: W4_Y (the kernel's cases and the
    passes), W4_DEQ_Y (the fallback's)."""
    from tests.test_rowwise_strict_gpu import _meas

    acc = {}
    for name, cases in (("W4_Y", [c[:3] for c in W4_CASES] + W4_PASSES), ("W4_DEQ_Y", W4_FALLBACK)):
        for M, N, K in sorted(set(cases)):
            x, _, _, r64 = X.linear_case("gauss", M, N, K)
            _meas(acc, name, x.float() @ X.dense("gauss", N, K).t(), r64, BF16)
    return acc


def main(argv):
    for name, (rel, ab) in measure().items():
        print(f"{name}_MEASURED = ({rel:.3g}, {ab:.3g})")
        print(f"{name} = ({max(2 * rel, ULP_BF16):.3g}, {2 * ab:.3g})")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
