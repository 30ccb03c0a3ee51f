"""Strict fp64 tests of the training step of both trainers on the GPU (cases, the reference of a step and the
checks: tests/_step_cases.py).

Three optimizer steps of ``Trainer`` (``compute_grads`` + ``_optimizer_step`` over the flat buffers) and of
``Zero3Trainer.train_step`` on the whole-model case (tiny-d128, 2 layers, ids [2, 256]), one process, one GPU.
Every step is checked from the trainer's own state before it and its own gradient buffer: the loss (mean over
the micro-batches of each one's mean over its valid tokens), every element of the gradient buffer, the clip norm,
master / m / v after the update, the stored bf16 parameters (the master's high half by the split rule), LoRA's
adapter copies and frozen weights; the state between two steps bit for bit; and a second trainer that runs the
same steps through plain ``train_step`` -- nothing read in between, the overlapped update really overlapping the
next forward -- must reproduce the losses and the final master / m / v bit for bit.

  Trainer       1 full fine-tune, MXLLM_GEMM8=all, one micro-batch: fused clip norm armed, clipped and unclipped
                2 the same, three micro-batches, an all-ignored one first (step 2) and last (step 3)
                3 fp32 gradients   4 tied embeddings (no fresh gradients)   5 activation_checkpointing=1
                6 MXLLM_DETERMINISTIC=1   7 no clipping, one-launch AdamW   8 LoRA r = 16 (1 and 2 micro-batches)
                9 LoRA with the overlapped update (per-chunk adapter copies)
  Zero3Trainer  10 world 1, fp32 gradients   11 activation_checkpointing=1, three micro-batches, an all-ignored
                one first   12 bf16 gradients   13 emulated world 4, every layer checkpointed

The fp64 reference runs on the device.  tests/test_step_cases.py runs the same checks on the CPU and plants the
defects they must catch; ``python -m tests._step_cases`` prints the measurements behind the bounds.
"""
import pytest

from tests import _step_cases as SC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", SC.CASES, ids=SC.case_id)
def test_step_fp64(gpu, case, monkeypatch):
    SC.run_case(case, gpu, monkeypatch)
