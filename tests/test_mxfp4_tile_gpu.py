"""The LDS-tiled MXFP4 GEMM (csrc/kernels/mxfp4_gemm.hip w4a16_tile_kernel) through ``w4_gemm`` and the
33 .. TILE_MAX_M row route of ``W4Linear``.  Inputs, references and the bound are those of
tests/test_mxfp4_gpu.py: the kernel has the same rounding points (exact bf16 weights, f32 accumulation, one
rounding of the result), so ``int`` cases are exact whatever the summation order and W4_Y carries over.
"""
import pytest
import torch

from tests._mxfp4 import bits, check_linear, linear_case, strided
from tests.test_mxfp4_gpu import W4_Y

pytestmark = pytest.mark.gpu

# (M, N, K).  A workgroup owns 128 channels (four waves x two 16-channel groups) and an M-block of 32 rows
# (M <= 32), 64 (M <= 64) or 128; more rows go over grid.y.  K is split over grid.z until 256 workgroups
# exist, four ways at most: the split follows the workgroup count, not K, so every N below 8192 runs split 4.
# M: 17 -> the 32-row block; 33 / 64 -> the 64-row block, one row of its third token block / full; 65 / 127 /
#    128 -> the 128-row block; 129 -> a second grid.y block of one row; 300 -> three blocks.
# N: 16 -> one group of one wave; 128 -> one whole workgroup; 1040 -> nine workgroups, the last with a single
#    group (N % 32 != 0); 2048 -> 16 workgroups, two per XCD.
# K: 512 -> one chunk per K part; 1536 -> three (the ring's slot 0 twice); 4608 -> nine (odd, four laps).
# N 8192 (64 workgroups per M-block): 64 / 128 rows -> split 4; 129 rows -> split 2, two chunks per part;
#    385 / 400 rows (four M-blocks, 256 workgroups) -> K whole, written as bf16 by the GEMM kernel itself.
W4T_CASES = [(M, N, 512) for M, N in ((17, 16), (33, 16), (64, 128), (65, 128), (33, 1040), (127, 1040),
                                      (128, 1040), (129, 1040), (64, 2048), (300, 2048))]
W4T_CASES += [(M, N, 1536) for M, N in ((65, 16), (128, 128), (33, 1040), (64, 1040), (129, 2048))]
W4T_CASES += [(M, N, 4608) for M, N in ((33, 16), (300, 16), (127, 128), (64, 1040), (129, 1040))]
W4T_CASES += [(64, 8192, 512), (129, 8192, 512), (400, 8192, 512), (128, 8192, 1536), (385, 8192, 1536)]


def _ops():
    from mxllm.ops import native

    return native()


@pytest.mark.parametrize("kind", ["int", "gauss"])
@pytest.mark.parametrize("M,N,K", W4T_CASES)
def test_w4_gemm_exact_and_parity(gpu, M, N, K, kind):
    run = lambda x, codes, scales: _ops().w4_gemm(x, codes, scales)  # noqa: E731
    check_linear(kind, M, N, K, run, gpu, W4_Y)


def test_w4_gemm_refusals(gpu):
    """Either side of each mx::w4t_takes rule a call can reach; after the refusals a valid call is right."""
    ops = _ops()
    taken = {}
    for N, K in ((96, 512), (96, 768), (104, 512)):  # taken; K % 512; N % 16
        x, codes, scales, _ = linear_case("int", 40, N, K)
        taken[N, K] = (strided(x, 24, 3, gpu), codes.to(gpu), scales.to(gpu))
    x, codes, scales = taken[96, 512]
    with pytest.raises(RuntimeError, match="w4t_takes"):
        ops.w4_gemm(*taken[96, 768])
    with pytest.raises(RuntimeError, match="w4t_takes"):
        ops.w4_gemm(*taken[104, 512])
    wide = strided(linear_case("int", 40, 96, 1024)[0], 24, 3, gpu)
    assert wide[:, 8:520].data_ptr() % 16 == 0 and wide[:, 4:516].data_ptr() % 16 == 8
    assert ops.w4_gemm(wide[:, 8:520], codes, scales).shape == (40, 96)  # a 16-B aligned column window
    with pytest.raises(RuntimeError, match="w4t_takes"):
        ops.w4_gemm(wide[:, 4:516], codes, scales)  # the same window 8 B off
    with pytest.raises(RuntimeError):
        ops.w4_gemm(x.float(), codes, scales)
    check_linear("int", 40, 96, 512, lambda *a: ops.w4_gemm(*a), gpu)


def test_w4_module_routes_tile(gpu, monkeypatch):
    """W4Linear.forward at 64 rows of a strided 3-D input is w4_gemm bit for bit; with TILE_MAX_M = 0 it is
    w4_linear with the module's STREAM_M."""
    from mxllm.serve import quant

    x, codes, scales, _ = linear_case("gauss", 64, 1040, 512)
    lin = quant.W4Linear(codes=codes, scales=scales).to(gpu)
    xd = strided(x, 24, 0, gpu)
    y = lin(xd.view(4, 16, 512))
    assert y.shape == (4, 16, 1040)
    assert torch.equal(bits(y.view(64, 1040).cpu()), bits(_ops().w4_gemm(xd, lin.codes, lin.scales).cpu()))
    monkeypatch.setattr(quant, "TILE_MAX_M", 0)
    want = _ops().w4_linear(xd, lin.codes, lin.scales, quant.STREAM_M)
    assert torch.equal(bits(lin(xd.view(4, 16, 512)).view(64, 1040).cpu()), bits(want.cpu()))
