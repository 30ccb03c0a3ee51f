"""Training-path checks on the MI355X (round 3):

* the optimizer overlapped with the next forward (per-layer AdamW chunks on a
  side stream) leaves master weights BITWISE equal to the one-launch update
  after 3 steps, with bf16 and with fp32 gradients;
* fp32 gradient accumulation: the fp32-output dW GEMM (hipBLASLt, bf16 operands)
  matches an fp32 reference for beta 0 and 1, and fp32 micro-batch
  accumulation is closer to the fp64 oracle than bf16 accumulation;
* ZeRO-3 on the GPU (the config-4 code path: fresh beta-0 dW into the unit
  buffer / straight into the fp32 grad shard at world 1, the emulated world-4
  gather/reduce-scatter, full / every-layer / selective activation
  checkpointing) matches the replicated DDP trainer per parameter after 3 steps.
Reference: the fine-tuning the reference advertises (README.md:1-3,7).
"""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


def _cfg():
    from mxllm.models import get_config

    return get_config("tiny-d128").replace(n_layers=3, vocab_size=1024)


def _ddp_trainer(gpu, cfg, seed, **kw):
    from mxllm.models import Llama
    from mxllm.parallel.runtime import DistEnv
    from mxllm.parallel.zero3 import init_full_state
    from mxllm.train.trainer import OptimConfig, Trainer

    model = Llama(cfg, device=gpu, seed=0)
    sd = init_full_state(cfg, seed, gpu)
    with torch.no_grad():
        for n, p in model.named_parameters():
            p.copy_(sd[n])
    return Trainer(model, DistEnv(device=gpu, backend="nccl"), OptimConfig(lr=1e-3, weight_decay=0.01), **kw)


def _masters(tr):
    tr.params_ready()
    return {s.name: tr.flat.master[s.offset:s.offset + s.numel].view(s.shape).clone() for s in tr.flat.slots}


@pytest.mark.parametrize("gdt,sched", [(None, ""), (torch.float32, ""), (None, "lag"), (None, "cus")])
def test_overlapped_adamw_bitwise(gpu, gdt, sched, monkeypatch):
    """``sched``: "lag" = chunks issued one group ahead of the forward (MXLLM_ADAMW_LAG=1);
    "cus" = the AdamW side stream confined to a CU subset (MXLLM_ADAMW_CUS)."""
    cfg = _cfg()
    g = torch.Generator(device=gpu).manual_seed(1)
    batches = [torch.randint(0, cfg.vocab_size, (2, 256), device=gpu, generator=g) for _ in range(3)]
    out = {}
    for ovl in (False, True):
        monkeypatch.delenv("MXLLM_ADAMW_LAG", raising=False)
        monkeypatch.delenv("MXLLM_ADAMW_CUS", raising=False)
        if ovl and sched == "lag":
            monkeypatch.setenv("MXLLM_ADAMW_LAG", "1")
        if ovl and sched == "cus":
            monkeypatch.setenv("MXLLM_ADAMW_CUS", "mod8:2")
        tr = _ddp_trainer(gpu, cfg, 11, overlap_optimizer=ovl, grad_dtype=gdt)
        assert tr.overlap_optimizer == ovl
        if ovl and sched == "lag":
            assert tr._lag == 1
        if ovl and sched == "cus":
            assert isinstance(tr._side, torch.cuda.ExternalStream)
        losses = [float(tr.train_step([(b, b)])) for b in batches]
        out[ovl] = (losses, _masters(tr))
    assert out[False][0] == out[True][0]
    for n, w in out[False][1].items():
        assert torch.equal(w, out[True][1][n]), n


@pytest.mark.parametrize("cfg_name", ["tiny-d128", "tiny"])
def test_lora_overlapped_adamw_bitwise(gpu, cfg_name, monkeypatch):
    """LoRA with the overlapped update (MXLLM_LORA_OVERLAP_ADAMW=1, opt-in): each forward chunk's
    AdamW runs on the side stream followed by the copy of its adapters into their augmented GEMM
    buffers, and the next forward waits per layer.  Same losses and masters bit for bit as the
    one-launch update + one end-of-step copy, and every GEMM buffer holds the updated adapters."""
    from mxllm.models import Llama, get_config
    from mxllm.models.llama import FusedLinear
    from mxllm.parallel.runtime import DistEnv
    from mxllm.train.trainer import OptimConfig, Trainer

    cfg = get_config(cfg_name).replace(n_layers=3, vocab_size=1024)
    g = torch.Generator(device=gpu).manual_seed(5)
    batches = [torch.randint(0, cfg.vocab_size, (2, 256), device=gpu, generator=g) for _ in range(3)]
    out = {}
    for ovl in ("0", "1"):
        monkeypatch.setenv("MXLLM_LORA_OVERLAP_ADAMW", ovl)
        model = Llama(cfg, device=gpu, seed=2, lora_r=16)
        with torch.no_grad():  # non-zero B: every adapter gets a gradient
            for i, mod in enumerate(model.modules()):
                if getattr(mod, "lora_r", 0):
                    for blk in mod.lora_b_blocks():
                        blk.normal_(0, 0.02, generator=torch.Generator(device=gpu).manual_seed(i))
        tr = Trainer(model, DistEnv(device=gpu, backend="nccl"), OptimConfig(lr=1e-3, weight_decay=0.01))
        assert tr.overlap_optimizer == (ovl == "1")
        if ovl == "1":
            assert tr._chunk_copies is not None and sum(c is not None for c in tr._chunk_copies) == 3
        losses = [float(tr.train_step([(b, b)])) for b in batches]
        tr.params_ready()
        for mod in model.modules():
            if isinstance(mod, FusedLinear) and mod.augmented():
                for src, dst in mod.adapter_copies():
                    assert torch.equal(src, dst)
        out[ovl] = (losses, _masters(tr))
    assert out["0"][0] == out["1"][0]
    for n, w in out["0"][1].items():
        assert torch.equal(w, out["1"][1][n]), n


def test_overlap_is_default_for_full_finetune(gpu):
    tr = _ddp_trainer(gpu, _cfg(), 3)
    assert tr.overlap_optimizer and len(tr._chunks) == 5  # embedding, 3 layers, head


@pytest.mark.parametrize("beta", [0.0, 1.0])
def test_fp32_output_dw_gemm(gpu, beta):
    from mxllm.ops.linear import weight_grad_

    T, N, K = 512, 384, 256
    dy = torch.randn(T, N, device=gpu).bfloat16()
    x = torch.randn(T, K, device=gpu).bfloat16()
    out = torch.randn(N, K, device=gpu)
    ref = dy.float().t() @ x.float() + beta * out
    if beta == 0.0:
        out.fill_(float("nan"))  # beta 0 must not read the output
    weight_grad_(out, dy, x, beta=beta)
    assert out.dtype == torch.float32
    assert ((out - ref).abs().max() / ref.abs().max()).item() < 1e-5


def test_fp32_accumulation_closer_to_oracle(gpu):
    """4 micro-batches accumulated into the flat gradient buffer: fp32 accumulation
    vs bf16, both against the fp64 sum of the per-micro-batch fp32 gradients."""
    cfg = _cfg()
    g = torch.Generator(device=gpu).manual_seed(2)
    mbs = [torch.randint(0, cfg.vocab_size, (2, 256), device=gpu, generator=g) for _ in range(4)]
    per = []
    for b in mbs:  # each micro-batch alone, fp32 gradient
        tr = _ddp_trainer(gpu, cfg, 5, grad_dtype=torch.float32, overlap_optimizer=False)
        tr.compute_grads([(b, b)])
        per.append(tr.flat.grads.double() / 4)
    oracle = sum(per)
    err = {}
    for gdt in (None, torch.float32):
        tr = _ddp_trainer(gpu, cfg, 5, grad_dtype=gdt, overlap_optimizer=False)
        tr.compute_grads([(b, b) for b in mbs])
        err[gdt] = ((tr.flat.grads.double() - oracle).norm() / oracle.norm()).item()
    assert err[torch.float32] < 1e-5, err
    assert err[torch.float32] < err[None] / 10, err


def _zero3(gpu, cfg, seed, **kw):
    from mxllm.parallel.runtime import DistEnv
    from mxllm.parallel.zero3 import Zero3Trainer
    from mxllm.train.trainer import OptimConfig

    return Zero3Trainer(cfg, DistEnv(device=gpu, backend="nccl"), OptimConfig(lr=1e-3, weight_decay=0.01),
                        seed=seed, **kw)


def test_zero3_matches_ddp_per_parameter_gpu(gpu):
    """World 1: every dW GEMM writes the fp32 grad shard directly (beta 0 on the
    first use), norms add their fp32 dγ, no gather copies."""
    cfg = _cfg()
    g = torch.Generator(device=gpu).manual_seed(3)
    batches = [torch.randint(0, cfg.vocab_size, (2, 256), device=gpu, generator=g) for _ in range(3)]
    tr = _ddp_trainer(gpu, cfg, 9, grad_dtype=torch.float32)
    d_loss = [float(tr.train_step([(b, b)])) for b in batches]
    ref = _masters(tr)
    del tr
    got = {}
    for ck in (False, True, 2):
        z = _zero3(gpu, cfg, 9, activation_checkpointing=ck)
        assert all(u.local for u in z.units)
        z_loss = [float(z.train_step([(b, b)])) for b in batches]
        for a, b in zip(d_loss, z_loss):
            assert abs(a - b) < 2e-3 * max(1.0, abs(a)), (ck, d_loss, z_loss)
        w = z.full_master_state()
        got[ck] = w
        assert set(w) == set(ref)
        for n, r in ref.items():
            d = (w[n] - r).abs()
            # 3 AdamW steps of lr 1e-3 move a weight by ~3e-3; fp32 gradients in both
            # trainers: they differ only by GEMM algorithm / reduction order
            bad = int((d > 2e-4).sum())
            assert float(d.mean()) < 2e-5 and bad <= max(4, 2e-3 * d.numel()), (ck, n, float(d.max()), bad)
    for ck in (True, 2):  # checkpointing recomputes the identical forward
        for n, w in got[False].items():
            assert torch.equal(w, got[ck][n]), (ck, n)


@pytest.mark.parametrize("ck", [False, True])
def test_zero3_emulated_world4_one_step_gpu(gpu, ck):
    """Emulated world 4 (the config-4 sizing proxy): the gathered unit is the local
    shard tiled 4x and the reduce-scatter sums the 4 slices.  Build that tiled
    model as a replicated DDP model, take its fp32 gradient, sum each unit's 4
    slices, apply the clip + AdamW step by hand: the emulated trainer's master
    shard must match after one step."""
    from mxllm.ops import reference as ref_ops

    cfg = _cfg()
    ids = torch.randint(0, cfg.vocab_size, (2, 256), device=gpu, generator=torch.Generator(device=gpu).manual_seed(4))
    z = _zero3(gpu, cfg, 13, activation_checkpointing=ck, emulate_world=4)
    tiled = z.full_master_state()  # every unit = its rank-0 shard tiled 4x
    shard0 = z.master.clone()
    tr = _ddp_trainer(gpu, cfg, 13, grad_dtype=torch.float32, overlap_optimizer=False)
    with torch.no_grad():
        for n, p in tr.model.named_parameters():
            p.copy_(tiled[n])
    tr.flat.master.copy_(tr.flat.params)
    tr.compute_grads([(ids, ids)])
    gd = {s.name: tr.flat.grads[s.offset:s.offset + s.numel] for s in tr.flat.slots}
    exp = torch.zeros_like(z.grads)
    off = 0
    for u in z.units:
        full = torch.zeros(u.full_numel, dtype=torch.float32, device=gpu)
        for name, o, n in zip(u.names, u.offsets, u.numels):
            full[o:o + n] = gd[name]
        # sharded unit: the emulated reduce-scatter sums the 4 slices; the replicated RMSNorm
        # unit: the emulated all-reduce of 4 identical ranks = 4 x its gradient
        exp[off:off + u.shard_numel] = full * 4 if u.replicated else full.view(4, -1).sum(0)
        off += u.shard_numel
    z.train_step([(ids, ids)])
    o = z.opt
    scale = 1.0 / 4
    gnorm = exp.double().norm().item() * scale
    gscale = min(1.0, o.grad_clip / (gnorm + 1e-6)) * scale
    m = torch.zeros_like(shard0)
    v = torch.zeros_like(shard0)
    want = shard0.clone()
    ref_ops.adamw_(want, exp, m, v, lr=o.lr, beta1=o.beta1, beta2=o.beta2, eps=o.eps, weight_decay=o.weight_decay,
                   step=1, grad_scale=gscale)
    d = (z.master.float() - want).abs()
    # step 1 of AdamW moves every weight by ~lr * sign(g): only near-zero gradients can differ
    assert float(d.mean()) < 2e-5 and int((d > 2e-4).sum()) <= max(8, 2e-3 * d.numel()), float(d.max())


@pytest.mark.parametrize("ck", [False, 2])
def test_zero3_overlapped_adamw_bitwise_gpu(gpu, ck):
    """ZeRO-3's per-unit AdamW on the side stream, overlapped with the next forward
    (each unit waited for just before it is used), gives bitwise the same weights and
    losses as the one-launch update after the step."""
    cfg = _cfg()
    g = torch.Generator(device=gpu).manual_seed(6)
    batches = [torch.randint(0, cfg.vocab_size, (2, 256), device=gpu, generator=g) for _ in range(3)]
    res = {}
    for ov in ("0", "1"):
        os.environ["MXLLM_Z3_ADAMW_OVERLAP"] = ov
        try:
            z = _zero3(gpu, cfg, 21, activation_checkpointing=ck, grad_dtype=torch.float32)
        finally:
            os.environ.pop("MXLLM_Z3_ADAMW_OVERLAP", None)
        assert z.overlap_optimizer == (ov == "1")
        losses = [z.train_step([(b, b)]) for b in batches]
        res[ov] = ([float(x) for x in losses], z.full_master_state())
        del z
    assert res["0"][0] == res["1"][0]
    for n, w in res["0"][1].items():
        assert torch.equal(w, res["1"][1][n]), n


def test_bench_config2_field_tiny(gpu, tmp_path):
    """The 1-GPU bench line carries the config-2 (full fine-tune DDP) result."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "b.json"
    r = subprocess.run([sys.executable, "bench.py", "--model", "tiny-d128", "--steps", "2", "--warmup", "1",
                        "--seq-len", "256", "--full", "--config2", "on", "--full-model", "tiny-d128", "--full-steps", "2",
                        "--full-warmup", "1", "--json-out", str(out)], cwd=root, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    j = json.loads(out.read_text())
    c2 = j["config2_8b_full"]
    assert "error" not in c2, c2
    assert c2["value"] > 0 and "config 2" in c2["label"] and c2["config"]["finetune"].startswith("full")
    assert "overlapped" in c2["config"]["optimizer"]
    assert "gemm_8192_bf16_tflops" in j["calibration"], j["calibration"]  # --full: the box calibration too


@pytest.mark.parametrize("gbf16,zero", [(True, False), (True, True), (False, False)])
def test_split_master_adamw_kernel_bitwise(gpu, gbf16, zero):
    """The SPLIT AdamW kernel (fp32 master as bf16 high half + int16 low half)
    against the fp32-master kernel: master / m / v bit for bit after 3 steps, the
    high half = the master rounded half-up on its bits, the gradient cleared iff
    asked; split/join kernels round-trip exactly."""
    from mxllm.ops import SplitMaster, adamw_step_

    n = (1 << 20) + 64
    g = torch.Generator(device=gpu).manual_seed(7)
    p32 = torch.randn(n, device=gpu, generator=g) * 0.05
    sm = SplitMaster(torch.empty(n, dtype=torch.bfloat16, device=gpu))
    sm.copy_(p32)
    assert torch.equal(sm.float().view(torch.int32), p32.view(torch.int32))
    m1, v1, m2, v2 = (torch.zeros(n, device=gpu) for _ in range(4))
    for step in range(1, 4):
        grad = torch.randn(n, device=gpu, generator=g)
        grad = grad.bfloat16() if gbf16 else grad
        g2 = grad.clone()
        kw = dict(lr=1e-3, beta1=0.9, beta2=0.95, eps=1e-8, weight_decay=0.01, step=step,
                  grad_scale=torch.tensor([0.7], device=gpu))
        adamw_step_(p32, grad, m1, v1, None, zero_grad=zero, **kw)
        adamw_step_(sm, g2, m2, v2, None, zero_grad=zero, **kw)
        assert bool((g2 == 0).all()) == zero
    assert torch.equal(sm.float().view(torch.int32), p32.view(torch.int32))
    assert torch.equal(m1, m2) and torch.equal(v1, v2)
    bits = p32.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    assert torch.equal(sm.hi.view(torch.int16).to(torch.int64) & 0xFFFF, ((bits + 0x8000) >> 16) & 0xFFFF)


@pytest.mark.parametrize("gdt", [None, torch.float32])
@pytest.mark.parametrize("accum", [1, 2])
def test_bucketed_grad_norm_overlap(gpu, gdt, accum, monkeypatch):
    """The clip norm from per-bucket sums of squares taken on a side stream during the
    backward (MXLLM_NORM_OVERLAP=1; measured neutral, off by default) equals a one-pass norm of the final gradient
    buffer at every step (fp32 summation order aside), with and without micro-batch
    accumulation, and the first step's norm equals the non-overlapped trainer's; small
    buckets so the model spans several."""
    from mxllm import ops

    cfg = _cfg()
    g = torch.Generator(device=gpu).manual_seed(5)
    batches = [torch.randint(0, cfg.vocab_size, (2, 256), device=gpu, generator=g) for _ in range(3 * accum)]
    first = {}
    for ov in ("1", "0"):
        monkeypatch.setenv("MXLLM_NORM_OVERLAP", ov)
        tr = _ddp_trainer(gpu, cfg, 13, grad_dtype=gdt, bucket_mb=1.0, first_bucket_mb=0.25)
        assert (tr._norm_side is not None) == (ov == "1")
        assert tr.fresh_grads  # the gradient buffer still holds the step's gradients afterwards
        for i in range(3 if ov == "1" else 1):
            tr.train_step([(b, b) for b in batches[i * accum:(i + 1) * accum]])
            torch.cuda.synchronize()
            got = float(tr.last_grad_norm)
            ref = float(ops.sq_norm(tr.flat.grads).sqrt())  # the buffer holds the micro-batch MEAN
            assert abs(got - ref) <= 1e-6 * ref, (ov, i, got, ref)
            if i == 0:
                first[ov] = got
        if ov == "1":
            assert len(tr.ddp.buckets) > 3
    assert abs(first["1"] - first["0"]) <= 1e-6 * first["0"], first


def test_fused_grad_norm_matches_full_pass(gpu, monkeypatch):
    """The clip norm from the dW GEMMs' per-tile partials (gemm8_sq) plus a direct pass over the other
    gradients equals the full pass over the SAME flat gradient to fp32 rounding at every step, every armed
    GEMM weight took the fused path, and the first step's gradients and update match the full-pass trainer.

    Only the first step is compared across the two trainers: the two norms differ in their last fp32 bits
    (different summation order), so the clip coefficients do, and from the second step on a master value
    sitting on a bf16 rounding boundary can round the other way -- after that the runs are different
    (equally valid) trajectories (scripts/diag/fused_norm_diag.py: step-0 gradients bitwise equal, step-1
    gradients ~1 bf16 ulp apart)."""
    from mxllm import ops

    monkeypatch.setenv("MXLLM_GEMM8", "all")  # the tiny shapes on gemm8 (the table holds real ones)
    cfg = _cfg()
    g = torch.Generator(device=gpu).manual_seed(3)
    batches = [torch.randint(0, cfg.vocab_size, (2, 256), device=gpu, generator=g) for _ in range(3)]
    res = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("MXLLM_FUSED_GRAD_NORM", fused)
        tr = _ddp_trainer(gpu, cfg, 5)
        tr.train_step([(batches[0], batches[0])])
        res[fused] = (float(tr.last_grad_norm), tr.flat.grads.clone(), _masters(tr))
        if fused == "1":
            for i, b in enumerate(batches):
                if i:
                    tr.train_step([(b, b)])
                got = float(tr.last_grad_norm)
                ref = float(ops.sq_norm(tr.flat.grads).sqrt())
                assert abs(got - ref) <= 1e-6 * ref, (i, got, ref)
            done = [n for n, p in tr.model.named_parameters() if getattr(p, "_mx_sq_done", None) is True]
            assert tr._sq_params and any("wgu" in n for n in done) and any("wd" in n for n in done), done
            assert not any("tok_emb" in n for n in done)  # the embedding gradient is summed directly
        else:
            assert not tr._sq_params
    (n1, g1, m1), (n0, g0, m0) = res["1"], res["0"]
    assert abs(n1 - n0) <= 1e-6 * n0, (n1, n0)
    assert torch.equal(g1, g0)  # the fused dW GEMMs store the same gradient bits
    for k in m0:
        assert torch.allclose(m1[k].float(), m0[k].float(), rtol=0, atol=1e-6), k
