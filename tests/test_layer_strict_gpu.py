"""Strict fp64 tests of every route of the training transformer layer on the GPU (cases, references, routes and
checks: tests/_layer_cases.py).

One ``Llama._layer`` call fed by its ``add_rms_norm``, of both layers of a two-layer model: x2, h2, the rotated
q / k that reach the attention kernel, the gradient of the incoming d and of every parameter, each element
against the exact fp64 function of the same bf16 inputs.  One test id per (shape, route, layer, gradient
target); the route is selected by its switches, spies assert that it ran (a case whose route did not run fails),
``mark_ready`` is counted, and every case runs twice and must reproduce its bits.

  full fine-tune, tiny-d128 2 x 256   default (fused qkv + RoPE epilogue, fused MLP with the SwiGLU backward
                                      epilogue), no-bwd-epilogue, unfused, rec (x and m recomputed), rec-keep-x,
                                      rec-unfused-mlp, rec-unfused, deterministic (every GEMM on gemm8)
  tiny-d128 and tiny (head dim 32)    2 x 192: no fused route takes the shape
  LoRA r = 16, tiny-d128 2 x 256      lora-default (lora_qkv_attention, SwiGLU writing both tails), lora-unfused

``python -m tests.test_layer_strict_gpu`` prints the CPU measurements behind the bounds of tests/_parity.py (no
GPU needed); tests/test_layer_cases.py runs the same checks on the CPU and plants the defects they must catch.
"""
import sys

import pytest

from tests import _layer_cases as LY

pytestmark = pytest.mark.gpu

FULL_ROUTES = ("default", "no-bwd-epilogue", "unfused", "rec", "rec-keep-x", "rec-unfused-mlp", "rec-unfused",
               "deterministic")
ALL_TARGET_ROUTES = ("default", "rec", "unfused")
RUNS = ([(LY.FULL_256, r, "autograd") for r in FULL_ROUTES]
        + [(LY.FULL_256, r, t) for r in ALL_TARGET_ROUTES for t in LY.TARGETS[1:]]
        + [(LY.FULL_192, "default", "autograd"), (LY.TINY_192, "default", "autograd")]
        + [(LY.LORA_256, "lora-default", "autograd"), (LY.LORA_256, "lora-unfused", "autograd")])


@pytest.mark.parametrize("i", (0, 1), ids=("layer0", "last-layer"))
@pytest.mark.parametrize("case,route,target", RUNS, ids=[f"{LY.case_id(c)}-{r}-{t}" for c, r, t in RUNS])
def test_layer_fp64(gpu, case, route, target, i, monkeypatch):
    LY.check_layer(case, route, target, gpu, monkeypatch, i)


@pytest.mark.parametrize("ckpt", LY.CKPT_SETTINGS, ids=lambda v: f"ckpt-{v}")
@pytest.mark.parametrize("tied", [False, True], ids=["untied", "tied"])
def test_whole_model_fp64(gpu, tied, ckpt, monkeypatch):
    """Two layers on ids [2, 256] (one id in a quarter of the positions, a tenth of the labels ignored): the loss
    and every parameter gradient per element against the fp64 model of the whole network, with no / every / the
    first layer under ``ckpt.checkpoint`` (the last: the other layer recomputes x and m), tied and untied head."""
    LY.check_whole_model(tied, ckpt, gpu, monkeypatch)


def main():
    for name, (rel, ab) in sorted(dict(LY.measure(), **LY.measure_model()).items()):
        print(f"{name}_MEASURED = ({rel:.3g}, {ab:.3g})")
    return 0


if __name__ == "__main__":
    sys.exit(main())
