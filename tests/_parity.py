"""Per-element parity check for kernel outputs against an fp64 reference.

One global norm ratio (``|a - b| / |b| < 1e-2`` on Gaussian data) cannot see a wrong 8-column
chunk, a wrong row of a partially filled last block or one element missed by a second grid pass:
each moves the ratio by a fraction of itself.  ``assert_parity`` bounds every element instead:

    |out - ref| <= c_rel * |ref| + c_abs * scale

``scale`` is the max |ref| of the element's row (last dimension) or of the whole tensor (or, for
an output whose every element can cancel, a given magnitude of its operands).  The
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
# Attention (tests/test_attention_strict_gpu.py; ``python -m tests.test_attention_strict_gpu`` prints the
# measurements): the fp32 model of the algorithm documented in attn_fwd.hip / attn_bwd.hip against fp64.
# The abs terms are those of the documented bf16 roundings of P~, P and dS before their MFMA products,
# not of fp32 arithmetic; O against its row, lse against the tensor, the gradients against the
# magnitude of their operands (``scales`` there).
ATTN_O_MEASURED = (0.00389, 0.00402)
ATTN_O = (ULP_BF16, 0.00804)  # 2 x 0.00389 < one ulp; 2 x 0.00402
ATTN_LSE_MEASURED = (0, 1.71e-07)
ATTN_LSE = (ULP_F32, 3.42e-07)  # 2 x 0 < one ulp; 2 x 1.71e-07
ATTN_DQ_MEASURED = (0, 0.00146)
ATTN_DQ = (ULP_F32, 0.00292)  # 2 x 0 < one ulp; 2 x 0.00146
ATTN_DK_MEASURED = (0, 0.00238)
ATTN_DK = (ULP_F32, 0.00476)  # 2 x 0 < one ulp; 2 x 0.00238
ATTN_DV_MEASURED = (0, 0.00204)
ATTN_DV = (ULP_F32, 0.00408)  # 2 x 0 < one ulp; 2 x 0.00204
ATTN_ROPE_DQKV_MEASURED = (0.00389, 0.00101)
ATTN_ROPE_DQKV = (ULP_BF16, 0.00202)  # 2 x 0.00389 < one ulp; 2 x 0.00101

# Decode attention (tests/test_decode_exact_gpu.py; ``python -m tests.test_decode_exact_gpu`` prints the
# measurements): the fp32 model of the algorithm documented in decode.hip (online softmax in the exp2
# domain per 64-key wave, the waves and then the 256-key splits merged, one division) against an fp64
# softmax; each head's output against its own maximum.  _MFMA: head_dim 128, P rounded to bf16 before the
# PV product (the abs term is that rounding's); _F32: the scalar kernel (head_dim 64 / 32) and the split
# merge of decode_fuse.h, P and the partials in fp32.
DECODE_O_MFMA_MEASURED = (0.00383, 0.00183)
DECODE_O_MFMA = (ULP_BF16, 0.00366)  # 2 x 0.00383 < one ulp; 2 x 0.00183
DECODE_O_F32_MEASURED = (0.00389, 5.9e-07)
DECODE_O_F32 = (ULP_BF16, 1.18e-06)  # 2 x 0.00389 < one ulp; 2 x 5.9e-07
# Decode GEMMs (tests/test_skinny_exact_gpu.py; ``python -m tests.test_skinny_exact_gpu`` prints the
# measurements): fp32 ``x.float() @ w.float().t()`` against the fp64 product at the Gaussian inputs of the
# tests, each output against its row's maximum.  W8_Y: the weights are the reference decode of the e4m3
# codes, the channel scale included.  W8_DEQ_Y: w8_linear's fallback (shapes the decode kernel does not take)
# dequantises to bf16 first -- its weights are the bf16 rounding of code * scale, the reference's too.
SKINNY_Y_MEASURED = (0.00388, 2.74e-07)
SKINNY_Y = (ULP_BF16, 5.48e-07)  # 2 x 0.00388 < one ulp; 2 x 2.74e-07
W8_Y_MEASURED = (0.00388, 7.83e-07)
W8_Y = (ULP_BF16, 1.57e-06)  # 2 x 0.00388 < one ulp; 2 x 7.83e-07
W8_DEQ_Y_MEASURED = (0.00379, 2.6e-07)
W8_DEQ_Y = (ULP_BF16, 5.2e-07)  # 2 x 0.00379 < one ulp; 2 x 2.6e-07
# The LoRA training path (tests/test_lora_strict_gpu.py; ``python -m tests.test_lora_strict_gpu`` prints the
# measurements, tests/_lora_cases.py ``measure`` makes them).  SWIGLU_LORA_TAIL: fp32
# ``s * (out.float() @ V.float().t())`` against the fp64 product of the same bf16 ``out``, each row against
# its maximum.  LORA_PROJ_*: the fp32 model of the augmented projection documented in mxllm/ops/linear.py
# (_LoRAAugFn) against plain fp64 with no intermediate rounding; the abs terms are those of the two stored
# bf16 tails t = s x A^T and g = s dy B, not of fp32 arithmetic.  LORA_MLP_*: the same models chained through
# the SwiGLU, every tensor that crosses an op boundary (gu, m, dm, dgu) rounded to bf16 as the ops store
# it.  Every output against its row's maximum: at these Gaussian operands none cancels as a whole.
SWIGLU_LORA_TAIL_MEASURED = (0.00389, 9.47e-07)
SWIGLU_LORA_TAIL = (ULP_BF16, 1.89e-06)  # 2 x 0.00389 < one ulp; 2 x 9.47e-07
LORA_PROJ_Y_MEASURED = (0.00389, 0.00313)
LORA_PROJ_Y = (ULP_BF16, 0.00626)  # 2 x 0.00389 < one ulp; 2 x 0.00313
LORA_PROJ_DX_MEASURED = (0.00389, 0.00289)
LORA_PROJ_DX = (ULP_BF16, 0.00578)  # 2 x 0.00389 < one ulp; 2 x 0.00289
LORA_PROJ_DA_MEASURED = (0.00389, 0.00318)
LORA_PROJ_DA = (ULP_BF16, 0.00636)  # 2 x 0.00389 < one ulp; 2 x 0.00318
LORA_PROJ_DB_MEASURED = (0.00389, 0.0051)
LORA_PROJ_DB = (ULP_BF16, 0.0102)  # 2 x 0.00389 < one ulp; 2 x 0.0051
LORA_MLP_Y_MEASURED = (0.00389, 0.0109)
LORA_MLP_Y = (ULP_BF16, 0.0218)  # 2 x 0.00389 < one ulp; 2 x 0.0109
LORA_MLP_DX_MEASURED = (0.00389, 0.00819)
LORA_MLP_DX = (ULP_BF16, 0.0164)  # 2 x 0.00389 < one ulp; 2 x 0.00819
LORA_MLP_DA_MEASURED = (0.00388, 0.00751)
LORA_MLP_DA = (ULP_BF16, 0.015)  # 2 x 0.00388 < one ulp; 2 x 0.00751
LORA_MLP_DB_MEASURED = (0.00388, 0.0232)
LORA_MLP_DB = (ULP_BF16, 0.0464)  # 2 x 0.00388 < one ulp; 2 x 0.0232
# The transformer layer (tests/test_layer_strict_gpu.py; ``python -m tests.test_layer_strict_gpu`` prints the
# measurements, tests/_layer_cases.py ``measure`` makes them): one ``Llama._layer`` call fed by its add_rms_norm,
# the fp32 model of the layer with every tensor the ops store between kernels rounded to bf16 (listed in that
# module's doc) against the exact fp64 function of the same bf16 inputs and its true gradients.  The abs terms
# are those of the chain of bf16 intermediates, not of fp32 arithmetic.  Every output against its row's maximum
# (a d-gamma: the vector's); max over both layers of every shape, and for the gradients over the targets
# (returned to autograd, added to a preset buffer).  _F32: the gradients accumulated over two micro-batches
# into an fp32 buffer (no output rounding: the rel term is fp32's).  LAYER_LORA_*: the LoRA layer, whose
# stored tails add roundings; one DA / DB per projection, DB per diagonal block.
# MODEL_*: the whole two-layer model on ids (embedding, first norm, both layers, fused head + cross-entropy with
# bf16 logits and bf16 d(logits)), the same models chained, tied and untied head; per-layer gradients over both
# layers.  MODEL_LOSS: the loss (fp32 output) against its own value; its measured abs term is three standard
# errors of the mean of the per-token losses (rms of the model's per-token errors / sqrt(n_valid)), not one
# draw of the mean's error: tests/_layer_cases.py ``measure_model`` says why.
LAYER_DD_MEASURED = (0.00389, 0.00827)
LAYER_DD = (ULP_BF16, 0.0165)  # 2 x 0.00389 < one ulp; 2 x 0.00827
LAYER_DG_ATTN_MEASURED = (0.00385, 0.00852)
LAYER_DG_ATTN = (ULP_BF16, 0.017)  # 2 x 0.00385 < one ulp; 2 x 0.00852
LAYER_DG_ATTN_F32_MEASURED = (0, 0.00681)
LAYER_DG_ATTN_F32 = (ULP_F32, 0.0136)  # 2 x 0 < one ulp; 2 x 0.00681
LAYER_DG_MLP_MEASURED = (0.00384, 0.0077)
LAYER_DG_MLP = (ULP_BF16, 0.0154)  # 2 x 0.00384 < one ulp; 2 x 0.0077
LAYER_DG_MLP_F32_MEASURED = (0, 0.00593)
LAYER_DG_MLP_F32 = (ULP_F32, 0.0119)  # 2 x 0 < one ulp; 2 x 0.00593
LAYER_DG_NEXT_MEASURED = (0.00385, 0.00667)
LAYER_DG_NEXT = (ULP_BF16, 0.0133)  # 2 x 0.00385 < one ulp; 2 x 0.00667
LAYER_DG_NEXT_F32_MEASURED = (0, 0.0037)
LAYER_DG_NEXT_F32 = (ULP_F32, 0.0074)  # 2 x 0 < one ulp; 2 x 0.0037
LAYER_DW_D_MEASURED = (0.00389, 0.0102)
LAYER_DW_D = (ULP_BF16, 0.0204)  # 2 x 0.00389 < one ulp; 2 x 0.0102
LAYER_DW_D_F32_MEASURED = (0, 0.00926)
LAYER_DW_D_F32 = (ULP_F32, 0.0185)  # 2 x 0 < one ulp; 2 x 0.00926
LAYER_DW_GU_MEASURED = (0.00389, 0.0151)
LAYER_DW_GU = (ULP_BF16, 0.0302)  # 2 x 0.00389 < one ulp; 2 x 0.0151
LAYER_DW_GU_F32_MEASURED = (0, 0.0107)
LAYER_DW_GU_F32 = (ULP_F32, 0.0214)  # 2 x 0 < one ulp; 2 x 0.0107
LAYER_DW_O_MEASURED = (0.00389, 0.0135)
LAYER_DW_O = (ULP_BF16, 0.027)  # 2 x 0.00389 < one ulp; 2 x 0.0135
LAYER_DW_O_F32_MEASURED = (0, 0.0104)
LAYER_DW_O_F32 = (ULP_F32, 0.0208)  # 2 x 0 < one ulp; 2 x 0.0104
LAYER_DW_QKV_MEASURED = (0.00389, 0.0169)
LAYER_DW_QKV = (ULP_BF16, 0.0338)  # 2 x 0.00389 < one ulp; 2 x 0.0169
LAYER_DW_QKV_F32_MEASURED = (0, 0.0197)
LAYER_DW_QKV_F32 = (ULP_F32, 0.0394)  # 2 x 0 < one ulp; 2 x 0.0197
LAYER_H2_MEASURED = (0.00389, 0.00845)
LAYER_H2 = (ULP_BF16, 0.0169)  # 2 x 0.00389 < one ulp; 2 x 0.00845
LAYER_K_MEASURED = (0.00389, 0.0073)
LAYER_K = (ULP_BF16, 0.0146)  # 2 x 0.00389 < one ulp; 2 x 0.0073
LAYER_LORA_DA_D_MEASURED = (0.00389, 0.0188)
LAYER_LORA_DA_D = (ULP_BF16, 0.0376)  # 2 x 0.00389 < one ulp; 2 x 0.0188
LAYER_LORA_DA_GU_MEASURED = (0.00386, 0.0123)
LAYER_LORA_DA_GU = (ULP_BF16, 0.0246)  # 2 x 0.00386 < one ulp; 2 x 0.0123
LAYER_LORA_DA_O_MEASURED = (0.00388, 0.0153)
LAYER_LORA_DA_O = (ULP_BF16, 0.0306)  # 2 x 0.00388 < one ulp; 2 x 0.0153
LAYER_LORA_DA_QKV_MEASURED = (0.00389, 0.0194)
LAYER_LORA_DA_QKV = (ULP_BF16, 0.0388)  # 2 x 0.00389 < one ulp; 2 x 0.0194
LAYER_LORA_DB_D_MEASURED = (0.00387, 0.0272)
LAYER_LORA_DB_D = (ULP_BF16, 0.0544)  # 2 x 0.00387 < one ulp; 2 x 0.0272
LAYER_LORA_DB_GU_MEASURED = (0.00389, 0.0321)
LAYER_LORA_DB_GU = (ULP_BF16, 0.0642)  # 2 x 0.00389 < one ulp; 2 x 0.0321
LAYER_LORA_DB_O_MEASURED = (0.00388, 0.0282)
LAYER_LORA_DB_O = (ULP_BF16, 0.0564)  # 2 x 0.00388 < one ulp; 2 x 0.0282
LAYER_LORA_DB_QKV_MEASURED = (0.00389, 0.0369)
LAYER_LORA_DB_QKV = (ULP_BF16, 0.0738)  # 2 x 0.00389 < one ulp; 2 x 0.0369
LAYER_LORA_DD_MEASURED = (0.00389, 0.0322)
LAYER_LORA_DD = (ULP_BF16, 0.0644)  # 2 x 0.00389 < one ulp; 2 x 0.0322
LAYER_LORA_H2_MEASURED = (0.00389, 0.0146)
LAYER_LORA_H2 = (ULP_BF16, 0.0292)  # 2 x 0.00389 < one ulp; 2 x 0.0146
LAYER_LORA_K_MEASURED = (0.00389, 0.00651)
LAYER_LORA_K = (ULP_BF16, 0.013)  # 2 x 0.00389 < one ulp; 2 x 0.00651
LAYER_LORA_Q_MEASURED = (0.00389, 0.0064)
LAYER_LORA_Q = (ULP_BF16, 0.0128)  # 2 x 0.00389 < one ulp; 2 x 0.0064
LAYER_LORA_X2_MEASURED = (0.00389, 0.0202)
LAYER_LORA_X2 = (ULP_BF16, 0.0404)  # 2 x 0.00389 < one ulp; 2 x 0.0202
LAYER_Q_MEASURED = (0.00389, 0.00839)
LAYER_Q = (ULP_BF16, 0.0168)  # 2 x 0.00389 < one ulp; 2 x 0.00839
LAYER_X2_MEASURED = (0.00389, 0.0116)
LAYER_X2 = (ULP_BF16, 0.0232)  # 2 x 0.00389 < one ulp; 2 x 0.0116
MODEL_DEMB_MEASURED = (0.00389, 0.0129)
MODEL_DEMB = (ULP_BF16, 0.0258)  # 2 x 0.00389 < one ulp; 2 x 0.0129
MODEL_DEMB_TIED_MEASURED = (0.00389, 0.0322)
MODEL_DEMB_TIED = (ULP_BF16, 0.0644)  # 2 x 0.00389 < one ulp; 2 x 0.0322
MODEL_DG_ATTN_MEASURED = (0.00387, 0.0118)
MODEL_DG_ATTN = (ULP_BF16, 0.0236)  # 2 x 0.00387 < one ulp; 2 x 0.0118
MODEL_DG_FINAL_MEASURED = (0.00382, 0.00354)
MODEL_DG_FINAL = (ULP_BF16, 0.00708)  # 2 x 0.00382 < one ulp; 2 x 0.00354
MODEL_DG_MLP_MEASURED = (0.00382, 0.00633)
MODEL_DG_MLP = (ULP_BF16, 0.0127)  # 2 x 0.00382 < one ulp; 2 x 0.00633
MODEL_DHEAD_MEASURED = (0.00389, 0.0323)
MODEL_DHEAD = (ULP_BF16, 0.0646)  # 2 x 0.00389 < one ulp; 2 x 0.0323
MODEL_DW_D_MEASURED = (0.00389, 0.0392)
MODEL_DW_D = (ULP_BF16, 0.0784)  # 2 x 0.00389 < one ulp; 2 x 0.0392
MODEL_DW_GU_MEASURED = (0.00389, 0.0704)
MODEL_DW_GU = (ULP_BF16, 0.141)  # 2 x 0.00389 < one ulp; 2 x 0.0704
MODEL_DW_O_MEASURED = (0.00389, 0.0566)
MODEL_DW_O = (ULP_BF16, 0.113)  # 2 x 0.00389 < one ulp; 2 x 0.0566
MODEL_DW_QKV_MEASURED = (0.00389, 0.06)
MODEL_DW_QKV = (ULP_BF16, 0.12)  # 2 x 0.00389 < one ulp; 2 x 0.06
MODEL_LOSS_MEASURED = (0, 0.000162)
MODEL_LOSS = (ULP_F32, 0.000324)  # 2 x 0 < one ulp; 2 x 0.000162
# The training step (tests/test_step_strict_gpu.py, tests/test_step_cases.py; ``python -m tests._step_cases`` prints
# the measurements, tests/_step_cases.py ``measure`` makes them): the fp32 model of three optimizer steps --
# ``model_math(..., F32, model=True)`` per micro-batch, accumulation in the gradient buffer's dtype with one
# rounding per added micro-batch (_F32: fp32 adds), ``reference.adamw_`` in fp32 with an fp32 clip norm -- against
# the fp64 reference, along the fp64 reference trajectory of every case (three parameter sets each; the MODEL_*
# constants were measured at the initial weights only).  Gradient constants per parameter kind, each row against
# its maximum; a kind whose step measurement came out no larger than its MODEL_* constant has no STEP_* twin and
# is held to the MODEL_* one (DEMB_TIED, DW_O).  STEP_Z3_*: the same kinds at the weights ZeRO-3 seeds for itself
# (N(0, 0.02), every norm weight 1), where a row's gradient is noisier against its maximum; the trainer's
# constants are not widened for them.  STEP_ADAMW_*: master, m, v after one step from the same state and buffer,
# each slot against its maximum, the model evaluated at the clipped gscale and at gscale (1 +- 6 x 2^-24): the
# coefficient is one number per step shared by every element, and six fp32 roundings lie between the gradient
# and it.  STEP_LOSS: three standard errors of the mean of the micro-batch means (``measure_model``'s rule),
# relative to the loss.
STEP_ADAMW_M_MEASURED = (0, 7.27e-07)
STEP_ADAMW_M = (ULP_F32, 1.45e-06)  # 2 x 0 < one ulp; 2 x 7.27e-07
STEP_ADAMW_P_MEASURED = (0, 1.17e-07)
STEP_ADAMW_P = (ULP_F32, 2.34e-07)  # 2 x 0 < one ulp; 2 x 1.17e-07
STEP_ADAMW_V_MEASURED = (0, 1.07e-06)
STEP_ADAMW_V = (ULP_F32, 2.14e-06)  # 2 x 0 < one ulp; 2 x 1.07e-06
STEP_DEMB_MEASURED = (0.00389, 0.0214)
STEP_DEMB = (ULP_BF16, 0.0428)  # 2 x 0.00389 < one ulp; 2 x 0.0214
STEP_DEMB_F32_MEASURED = (0, 0.0261)
STEP_DEMB_F32 = (ULP_F32, 0.0522)  # 2 x 0 < one ulp; 2 x 0.0261
STEP_DG_ATTN_MEASURED = (0.00387, 0.0147)
STEP_DG_ATTN = (ULP_BF16, 0.0294)  # 2 x 0.00387 < one ulp; 2 x 0.0147
STEP_DG_ATTN_F32_MEASURED = (0, 0.0127)
STEP_DG_ATTN_F32 = (ULP_F32, 0.0254)  # 2 x 0 < one ulp; 2 x 0.0127
STEP_DG_FINAL_MEASURED = (0.00382, 0.00894)
STEP_DG_FINAL = (ULP_BF16, 0.0179)  # 2 x 0.00382 < one ulp; 2 x 0.00894
STEP_DG_FINAL_F32_MEASURED = (0, 0.00526)
STEP_DG_FINAL_F32 = (ULP_F32, 0.0105)  # 2 x 0 < one ulp; 2 x 0.00526
STEP_DG_MLP_MEASURED = (0.00389, 0.0108)
STEP_DG_MLP = (ULP_BF16, 0.0216)  # 2 x 0.00389 < one ulp; 2 x 0.0108
STEP_DG_MLP_F32_MEASURED = (0, 0.00691)
STEP_DG_MLP_F32 = (ULP_F32, 0.0138)  # 2 x 0 < one ulp; 2 x 0.00691
STEP_DHEAD_MEASURED = (0.00389, 0.0406)
STEP_DHEAD = (ULP_BF16, 0.0812)  # 2 x 0.00389 < one ulp; 2 x 0.0406
STEP_DHEAD_F32_MEASURED = (0, 0.0322)
STEP_DHEAD_F32 = (ULP_F32, 0.0644)  # 2 x 0 < one ulp; 2 x 0.0322
STEP_DW_D_MEASURED = (0.00389, 0.0522)
STEP_DW_D = (ULP_BF16, 0.104)  # 2 x 0.00389 < one ulp; 2 x 0.0522
STEP_DW_D_F32_MEASURED = (0, 0.0317)
STEP_DW_D_F32 = (ULP_F32, 0.0634)  # 2 x 0 < one ulp; 2 x 0.0317
STEP_DW_GU_MEASURED = (0.00389, 0.0808)
STEP_DW_GU = (ULP_BF16, 0.162)  # 2 x 0.00389 < one ulp; 2 x 0.0808
STEP_DW_GU_F32_MEASURED = (0, 0.0469)
STEP_DW_GU_F32 = (ULP_F32, 0.0938)  # 2 x 0 < one ulp; 2 x 0.0469
STEP_DW_O_F32_MEASURED = (0, 0.0463)
STEP_DW_O_F32 = (ULP_F32, 0.0926)  # 2 x 0 < one ulp; 2 x 0.0463
STEP_DW_QKV_MEASURED = (0.00389, 0.0621)
STEP_DW_QKV = (ULP_BF16, 0.124)  # 2 x 0.00389 < one ulp; 2 x 0.0621
STEP_DW_QKV_F32_MEASURED = (0, 0.0482)
STEP_DW_QKV_F32 = (ULP_F32, 0.0964)  # 2 x 0 < one ulp; 2 x 0.0482
STEP_LORA_DA_D_MEASURED = (0.00389, 0.0531)
STEP_LORA_DA_D = (ULP_BF16, 0.106)  # 2 x 0.00389 < one ulp; 2 x 0.0531
STEP_LORA_DA_GU_MEASURED = (0.00389, 0.0427)
STEP_LORA_DA_GU = (ULP_BF16, 0.0854)  # 2 x 0.00389 < one ulp; 2 x 0.0427
STEP_LORA_DA_O_MEASURED = (0.00388, 0.0381)
STEP_LORA_DA_O = (ULP_BF16, 0.0762)  # 2 x 0.00388 < one ulp; 2 x 0.0381
STEP_LORA_DA_QKV_MEASURED = (0.00389, 0.0613)
STEP_LORA_DA_QKV = (ULP_BF16, 0.123)  # 2 x 0.00389 < one ulp; 2 x 0.0613
STEP_LORA_DB_D_MEASURED = (0.00388, 0.061)
STEP_LORA_DB_D = (ULP_BF16, 0.122)  # 2 x 0.00388 < one ulp; 2 x 0.061
STEP_LORA_DB_GU_MEASURED = (0.00389, 0.107)
STEP_LORA_DB_GU = (ULP_BF16, 0.214)  # 2 x 0.00389 < one ulp; 2 x 0.107
STEP_LORA_DB_O_MEASURED = (0.00389, 0.0825)
STEP_LORA_DB_O = (ULP_BF16, 0.165)  # 2 x 0.00389 < one ulp; 2 x 0.0825
STEP_LORA_DB_QKV_MEASURED = (0.00389, 0.154)
STEP_LORA_DB_QKV = (ULP_BF16, 0.308)  # 2 x 0.00389 < one ulp; 2 x 0.154
STEP_LOSS_MEASURED = (0, 0.0004)
STEP_LOSS = (ULP_F32, 0.0008)  # 2 x 0 < one ulp; 2 x 0.0004
STEP_Z3_DEMB_MEASURED = (0.00389, 0.0107)
STEP_Z3_DEMB = (ULP_BF16, 0.0214)  # 2 x 0.00389 < one ulp; 2 x 0.0107
STEP_Z3_DEMB_F32_MEASURED = (0, 0.0113)
STEP_Z3_DEMB_F32 = (ULP_F32, 0.0226)  # 2 x 0 < one ulp; 2 x 0.0113
STEP_Z3_DG_ATTN_MEASURED = (0.00389, 0.00679)
STEP_Z3_DG_ATTN = (ULP_BF16, 0.0136)  # 2 x 0.00389 < one ulp; 2 x 0.00679
STEP_Z3_DG_ATTN_F32_MEASURED = (0, 0.00711)
STEP_Z3_DG_ATTN_F32 = (ULP_F32, 0.0142)  # 2 x 0 < one ulp; 2 x 0.00711
STEP_Z3_DG_FINAL_MEASURED = (0.00389, 0.00621)
STEP_Z3_DG_FINAL = (ULP_BF16, 0.0124)  # 2 x 0.00389 < one ulp; 2 x 0.00621
STEP_Z3_DG_FINAL_F32_MEASURED = (0, 0.00577)
STEP_Z3_DG_FINAL_F32 = (ULP_F32, 0.0115)  # 2 x 0 < one ulp; 2 x 0.00577
STEP_Z3_DG_MLP_MEASURED = (0.00389, 0.00927)
STEP_Z3_DG_MLP = (ULP_BF16, 0.0185)  # 2 x 0.00389 < one ulp; 2 x 0.00927
STEP_Z3_DG_MLP_F32_MEASURED = (0, 0.01)
STEP_Z3_DG_MLP_F32 = (ULP_F32, 0.02)  # 2 x 0 < one ulp; 2 x 0.01
STEP_Z3_DHEAD_MEASURED = (0.00389, 0.057)
STEP_Z3_DHEAD = (ULP_BF16, 0.114)  # 2 x 0.00389 < one ulp; 2 x 0.057
STEP_Z3_DHEAD_F32_MEASURED = (0, 0.0593)
STEP_Z3_DHEAD_F32 = (ULP_F32, 0.119)  # 2 x 0 < one ulp; 2 x 0.0593
STEP_Z3_DW_D_MEASURED = (0.00389, 0.0718)
STEP_Z3_DW_D = (ULP_BF16, 0.144)  # 2 x 0.00389 < one ulp; 2 x 0.0718
STEP_Z3_DW_D_F32_MEASURED = (0, 0.0681)
STEP_Z3_DW_D_F32 = (ULP_F32, 0.136)  # 2 x 0 < one ulp; 2 x 0.0681
STEP_Z3_DW_GU_MEASURED = (0.00389, 0.153)
STEP_Z3_DW_GU = (ULP_BF16, 0.306)  # 2 x 0.00389 < one ulp; 2 x 0.153
STEP_Z3_DW_GU_F32_MEASURED = (0, 0.206)
STEP_Z3_DW_GU_F32 = (ULP_F32, 0.412)  # 2 x 0 < one ulp; 2 x 0.206
STEP_Z3_DW_O_MEASURED = (0.00389, 0.0732)
STEP_Z3_DW_O = (ULP_BF16, 0.146)  # 2 x 0.00389 < one ulp; 2 x 0.0732
STEP_Z3_DW_O_F32_MEASURED = (0, 0.0729)
STEP_Z3_DW_O_F32 = (ULP_F32, 0.146)  # 2 x 0 < one ulp; 2 x 0.0729
STEP_Z3_DW_QKV_MEASURED = (0.00389, 0.117)
STEP_Z3_DW_QKV = (ULP_BF16, 0.234)  # 2 x 0.00389 < one ulp; 2 x 0.117
STEP_Z3_DW_QKV_F32_MEASURED = (0, 0.406)
STEP_Z3_DW_QKV_F32 = (ULP_F32, 0.812)  # 2 x 0 < one ulp; 2 x 0.406


def assert_exact(out: torch.Tensor, want: torch.Tensor, name: str = "") -> None:
    """Assert ``torch.equal(out, want)``: same shape, same dtype, every element equal (no tolerance).

    For the cases whose result is exactly representable whatever the summation order (integer
    operands of an MFMA GEMM, a one-hot softmax).  On failure the message gives the mismatch count,
    the first and the worst mismatch with both values, and the bounding box of the mismatches over
    the last two dimensions -- rows a..b, columns c..d name the wrong fragment, tile or row."""
    assert tuple(out.shape) == tuple(want.shape), f"{name}: shape {tuple(out.shape)} vs expected {tuple(want.shape)}"
    assert out.dtype == want.dtype, f"{name}: dtype {out.dtype} vs expected {want.dtype}"
    if torch.equal(out, want):
        return
    o, w = out.detach().to(torch.float64), want.detach().to(torch.float64)
    bad = ~(o == w)  # NaN compares false: counted
    diff = torch.where(torch.isfinite(o - w), (o - w).abs(), torch.full_like(o, float("inf")))
    diff = torch.where(bad, diff, torch.zeros_like(diff))
    nz = bad.nonzero()
    first = tuple(int(i) for i in nz[0])
    flat = int(diff.reshape(-1).argmax())
    worst = []
    for d in reversed(o.shape):
        worst.append(flat % d)
        flat //= d
    worst = tuple(reversed(worst))
    box = ""
    if o.dim() >= 2:
        r, c = nz[:, -2], nz[:, -1]
        box = f"; rows {int(r.min())}..{int(r.max())}, columns {int(c.min())}..{int(c.max())}"
        if o.dim() > 2:
            lead = sorted({tuple(int(i) for i in row) for row in nz[:, :-2].tolist()})
            box += f" of {len(lead)} leading index(es) from {lead[0]} to {lead[-1]}"
    elif o.dim() == 1:
        box = f"; indices {int(nz.min())}..{int(nz.max())}"
    raise AssertionError(
        f"{name or 'output'}: {int(bad.sum())} of {o.numel()} elements differ; first at {first}: out "
        f"{o[first].item():.9g}, expected {w[first].item():.9g}; worst at {worst}: out {o[worst].item():.9g}, "
        f"expected {w[worst].item():.9g}{box}")


def assert_parity(out: torch.Tensor, ref: torch.Tensor, bound, *, scale: str = "row", name: str = "") -> None:
    """Assert ``|out - ref| <= c_rel |ref| + c_abs scale`` for every element.

    ``out``: the kernel's output (any float dtype).  ``ref``: the fp64 reference, same shape, same
    device.  ``bound``: ``(c_rel, c_abs)``.  ``scale``: ``"row"`` (max |ref| over the last dimension),
    ``"tensor"``, or a number: the magnitude of the operands of an output that can cancel as a
    whole.  A non-finite ``out`` element fails.  On failure the message names the worst element (largest excess over its bound), both values there, and how many elements exceed the
    bound -- which localizes a wrong chunk, row or block."""
    c_rel, c_abs = bound
    assert ref.dtype == torch.float64, "the reference must be fp64"
    assert tuple(out.shape) == tuple(ref.shape), f"{name}: shape {tuple(out.shape)} vs reference {tuple(ref.shape)}"
    if ref.numel() == 0:
        return
    o = out.detach().to(torch.float64)
    r = ref.detach()
    if scale == "row":
        s, what = r.abs().amax(dim=-1, keepdim=True), "row-max"
    elif scale == "tensor":
        s, what = r.abs().max(), "tensor-max"
    elif isinstance(scale, (float, torch.Tensor)):
        s = torch.as_tensor(scale, dtype=torch.float64, device=r.device)
        what = f"x {float(s):.3g} (operand magnitude)"
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
        f"{c_abs:.3g} {what}; worst at {idx}: out {o[idx].item():.9g}, ref {r[idx].item():.9g}, "
        f"|diff| {err[idx].item():.3g} > bound {lim.expand_as(err)[idx].item():.3g}; first at {first}")

