"""The strict training-step tests (tests/test_step_strict_gpu.py, tests/_step_cases.py) on the CPU: the cases are
what their module says, the reference written as a trainer passes the very checks the HIP path meets, the CPU
path of both trainers passes them, every planted defect is rejected, and the constants of tests/_parity.py are
those ``measure()`` gives."""
import re

import pytest
import torch

from tests import _layer_cases as LY
from tests import _parity as P
from tests import _step_cases as SC

CPU = torch.device("cpu")
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64


# =========================================================================== the cases
def test_cases_are_the_thirteen_of_the_issue():
    assert sorted({c.num for c in SC.CASES}) == list(range(1, 14))
    assert len({SC.case_id(c) for c in SC.CASES}) == len(SC.CASES)
    assert [SC.lr_ref(s) for s in (1, 2, 3)] == pytest.approx([5e-4, 1e-3, 5e-4], rel=1e-12)
    assert SC.lr_ref(4) == pytest.approx(0.0, abs=1e-18) and SC.lr_ref(9) == pytest.approx(0.0, abs=1e-18)
    for c in SC.CASES:
        assert len(c.plan) == SC.STEPS
    c2, c11 = SC.by_name("full-gemm8-3mb-ignored"), SC.by_name("zero3-w1-ckpt1-3mb-ignored")
    assert c2.plan[1][0] == "Z" and c2.plan[2][-1] == "Z" and c11.plan[1][0] == "Z"
    cfg = LY.config(LY.MODEL_CASE)  # every weight in whole 256 x 256 tiles: what the fused clip norm needs
    assert (cfg.vocab_size, cfg.hidden, cfg.ffn, cfg.n_layers) == (512, 512, 1024, 2)


def test_lr_schedule_is_the_dataclass_documented_meaning():
    """``lr_ref`` is written out independently; the trainer's own ``lr_at`` must be the same schedule."""
    from mxllm.train.trainer import OptimConfig

    o = OptimConfig(**SC.OPT)
    for step in range(1, 8):
        assert o.lr_at(step) == pytest.approx(SC.lr_ref(step), rel=1e-12, abs=1e-18)


@pytest.mark.parametrize("tied", [False, True], ids=["untied", "tied"])
def test_micro_batches(tied):
    (ia, la), (ib, lb), (iz, lz) = [SC.micro_batch(tied, k) for k in "ABZ"]
    na, nb = int((la != SC.IGNORE).sum()), int((lb != SC.IGNORE).sum())
    assert torch.equal(ib, ia.flip(0)) and 0.35 * na < nb < 0.65 * na and not bool((lz != SC.IGNORE).any())
    assert bool(((lb == la.flip(0)) | (lb == SC.IGNORE)).all())


def test_mean_of_means_is_not_the_token_mean():
    """The loss contract: each micro-batch's mean over its own valid tokens, then the mean over the micro-batches
    (an all-ignored one counts with loss 0) -- and at these micro-batches the token mean is another number."""
    c = SC.by_name("full-gemm8-3mb-ignored")
    mbs = SC.batches(c, 1)
    loss, grads, outs = SC.ref_loss_grads(c, SC.start_params(c), mbs)
    means = [float(o["losses"].mean()) if o["losses"].numel() else 0.0 for o in outs]
    assert float(loss) == pytest.approx(sum(means) / 3, rel=1e-12) and means[1] == 0.0
    token_mean = float(torch.cat([o["losses"] for o in outs]).mean())
    assert abs(token_mean - float(loss)) > 0.1 * float(loss)
    z = outs[1]
    assert all(not bool(v.any()) for k, v in z.items() if k != "losses") and float(z["loss"]) == 0.0


def test_lora_whole_model_reference():
    """The LoRA whole model: the adapters alone have gradients, the adapter terms matter (b = 0 gives another
    loss), the off-diagonal blocks of B have none, and the fp32 model meets the LoRA bounds."""
    c = SC.by_name("lora-1mb")
    params, mb = SC.start_params(c), SC.batches(c, 1)[0]
    ref = LY.model_math(False, F64, False, params=params, batch=mb, lora=c.lora)
    keys = {f"l{i}.d{ab}_{p[1:]}" for i in (0, 1) for p in LY.PROJS for ab in "ab"}
    assert set(ref) == keys | {"loss", "losses"}
    zero_b = {k: (torch.zeros_like(v) if k.endswith("lora_b") else v) for k, v in params.items()}
    without = LY.model_math(False, F64, False, params=zero_b, batch=mb, lora=c.lora)
    assert abs(float(without["loss"] - ref["loss"])) > 0.01
    mod = LY.model_math(False, F32, True, params=params, batch=mb, lora=c.lora)
    for k in sorted(keys):
        name = next(n for n in params if LY.trainable(n, c.lora) and LY.param_key(n) == k)
        bound, bname = SC.grad_bound(c, name, BF16)
        P.assert_parity(mod[k].to(BF16), ref[k], bound, scale="row", name=f"{k} ({bname})")
        if ".db_" in k:
            mask = LY.LC.block_mask(LY.proj_splits(LY.config(LY.LORA_256), "w" + k.split("_")[1]), c.lora)
            assert not bool(ref[k][~mask].any()) and bool(ref[k][mask].any())


# =========================================================================== the reference against itself
SELF_CASES = [SC.by_name(n) for n in ("full-gemm8-fusednorm-1mb", "full-gemm8-3mb-ignored", "full-fp32grads-2mb",
                                      "tied-2mb", "lora-2mb", "zero3-w1-bf16grads-2mb", "zero3-emulated4-ckpt-2mb")]


@pytest.mark.parametrize("case", SELF_CASES, ids=SC.case_id)
def test_reference_as_a_trainer_meets_the_checks(case):
    recs, lay = SC.simulate(case)
    assert bool(SC.pad_mask(lay, "cpu").any())  # (the simulated layout has the pads the real shapes never need)
    seen = [SC.check_step(case, lay, rec, "reference") for rec in recs]
    if case.num == 1:
        assert [co == 1.0 for _, co in seen] == [True, False, True], seen
        assert min(g for g, _ in seen) < case.clip < max(g for g, _ in seen)


# =========================================================================== the CPU path of both trainers
@pytest.mark.parametrize("case", SC.CPU_CASES, ids=SC.case_id)
def test_cpu_path_meets_the_checks(case, monkeypatch):
    """Cases 1-5, 7, 8 and 10-13 on CPU tensors.  Fresh gradients, the fused clip norm and the side streams are
    GPU-only: ``_Run.check_path`` asserts that the CPU trainer has none of them."""
    SC.run_case(case, CPU, monkeypatch)


def test_cpu_prompt_only_micro_batch_has_loss_zero_and_no_gradient():
    """The un-chunked CPU ``linear_cross_entropy``: no valid label gives loss 0 and a zero gradient, as the kernels
    and the chunked path do (it used to return 0 / 0)."""
    from mxllm import ops

    g = LY._gen(5)
    h = torch.randn(8, 16, generator=g).requires_grad_(True)
    w = torch.randn(32, 16, generator=g).requires_grad_(True)
    labels = torch.full((8,), SC.IGNORE)
    for chunk in (None, 4):
        h.grad = w.grad = None
        loss = ops.linear_cross_entropy(h, w, labels, chunk=chunk)
        loss.backward()
        assert float(loss.detach()) == 0.0 and not bool(h.grad.any()) and not bool(w.grad.any()), chunk
    labels[3] = 7
    want = torch.nn.functional.cross_entropy(h.detach() @ w.detach().t(), labels, ignore_index=SC.IGNORE)
    assert float(ops.linear_cross_entropy(h, w, labels).detach()) == pytest.approx(float(want), rel=1e-6)


# =========================================================================== planted defects
# defect -> (case, the steps whose check must fail, what the failure names)
FULL3, FULL1, LORA = "full-gemm8-3mb-ignored", "full-gemm8-fusednorm-1mb", "lora-2mb"
Z3, Z3E = "zero3-w1-bf16grads-2mb", "zero3-emulated4-ckpt-2mb"
DEFECT_HITS = {
    "accum-divided-twice": (FULL3, (1, 2, 3), "gradient of"),
    # (step 2 starts with the all-ignored micro-batch: overwriting its zeros changes nothing)
    "second-microbatch-overwrites": (FULL3, (1, 3), "gradient of"),
    "stale-slot": (FULL3, (2, 3), "gradient of " + re.escape(SC.STALE_SLOT)),
    "ignored-microbatch-counted": (FULL3, (1, 2, 3), "loss"),
    "norm-skips-embedding": (FULL3, (1, 2, 3), "clip norm"),
    "norm-of-unscaled-sum": (Z3, (1, 2, 3), "clip norm"),
    "coef-not-clamped": (FULL1, (1, 3), "m of|v of|master of"),
    "bias-correction-step-minus-one": (FULL3, (1, 2, 3), "master of"),
    "lr-of-previous-step": (FULL3, (1, 2, 3), "master of"),
    "weight-decay-as-l2": (FULL3, (1, 2, 3), "m of|v of|master of"),
    "pad-not-zero": (FULL3, (1, 2, 3), "gradient pad not zero"),
    "params-rne-not-split-rule": (FULL3, (), "stored bf16 parameters"),
    "adapter-buffer-stale": (LORA, (1, 2, 3), "adapter copy"),
    # (while the step is clipped the update does not depend on the scale: the clip norm shows it)
    "zero3-scale-without-n": (Z3, (1, 2, 3), "clip norm"),
    "zero3-replicated-unit-counted-world-times": (Z3E, (1, 2, 3), "clip norm"),
}


def test_defect_list_is_the_fifteen_of_the_issue():
    assert len(SC.DEFECTS) == len(set(SC.DEFECTS)) == 15 and set(DEFECT_HITS) == set(SC.DEFECTS)


@pytest.mark.parametrize("defect", SC.DEFECTS)
def test_planted_defect_is_rejected(defect):
    """The reference as a trainer passes without the defect (test_reference_as_a_trainer_meets_the_checks); with
    it, the check of every step the defect reaches fails, and names what is wrong."""
    name, steps, what = DEFECT_HITS[defect]
    case = SC.by_name(name)
    recs, lay = SC.simulate(case, defect)
    if defect == "params-rne-not-split-rule":
        # only a tie rounds differently: the steps whose master has one (at least one does: assert it)
        steps = tuple(r.step for r in recs if bool(SC.is_tie(r.after[0]).any()))
        assert steps, "no master of this case is a tie of the split rule"
        for r in recs:
            assert int((r.stored != SC.split_hi(r.after[0])).sum()) == int(SC.is_tie(r.after[0]).sum())
    for rec in recs:
        if rec.step in steps:
            with pytest.raises(AssertionError, match=what):
                SC.check_step(case, lay, rec, defect)
        else:
            SC.check_step(case, lay, rec, defect)


# =========================================================================== the constants
def test_measured_constants_are_current():
    acc = SC.new_constants(SC.measure())
    have = {n[:-9] for n in dir(P) if n.startswith("STEP_") and n.endswith("_MEASURED")}
    assert set(acc) == have, sorted(set(acc) ^ have)
    for name, (rel, ab) in acc.items():
        f32 = name.endswith("_F32") or name in ("STEP_LOSS", "STEP_ADAMW_P", "STEP_ADAMW_M", "STEP_ADAMW_V")
        ulp = P.ULP_F32 if f32 else P.ULP_BF16
        assert getattr(P, name + "_MEASURED") == (float(f"{rel:.3g}"), float(f"{ab:.3g}")), name
        assert getattr(P, name) == (max(2 * float(f"{rel:.3g}"), ulp), pytest.approx(2 * ab, rel=5e-3)), name
