"""Model / engine level checks on the MI355X: the HIP path against the
pure-PyTorch reference path with the same weights, decode kernels against
their references, the native loader feeding the GPU, and smoke()."""
import math
import os

import pytest
import torch

from mxllm.ops import reference as ref

pytestmark = pytest.mark.gpu


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


@pytest.mark.parametrize("preset,lora", [("tiny-d128", 0), ("tiny-d128", 8), ("tiny-d128", 16), ("tiny", 0)])
def test_train_step_matches_reference_path(gpu, preset, lora, monkeypatch):
    from mxllm.models import Llama, get_config

    cfg = get_config(preset)
    torch.manual_seed(0)
    m = Llama(cfg, device=gpu, lora_r=lora, seed=5)
    if lora:
        with torch.no_grad():
            for mod in m.modules():
                if getattr(mod, "lora_r", 0):
                    for blk in mod.lora_b_blocks():
                        blk.normal_(0, 0.02)
            m.sync_adapters_()
    ids = torch.randint(0, cfg.vocab_size, (2, 192), device=gpu)
    loss = m(ids, ids)
    loss.backward()
    g_native = {n: p.grad.float().clone() for n, p in m.named_parameters() if p.requires_grad}
    m.zero_grad(set_to_none=True)
    monkeypatch.setenv("MXLLM_REFERENCE_OPS", "1")
    loss_ref = m(ids, ids)
    loss_ref.backward()
    assert abs(loss.item() - loss_ref.item()) < 2e-2 * max(1, abs(loss_ref.item()))
    for n, p in m.named_parameters():
        if p.requires_grad:
            e = _rel(g_native[n], p.grad)
            assert e < 6e-2, (n, e)


@pytest.mark.parametrize("D,Hq,Hkv", [(128, 8, 2), (128, 32, 8), (128, 64, 8), (128, 16, 1), (64, 32, 8), (32, 8, 2)])
def test_decode_kernels(gpu, D, Hq, Hkv):
    """rope_append + decode attention (D=128: the MFMA kernel) vs an fp32 reference:
    GQA group sizes 4 / 8 / 16, key counts at and around the 64-key wave and
    256-key split boundaries, permuted cache slots."""
    from mxllm.ops import native

    torch.manual_seed(1)
    max_seq = 700
    lens = [0, 5, 63, 255, 256, 300, 640]
    B = len(lens)
    kc = torch.randn(B + 1, Hkv, max_seq, D, device=gpu, dtype=torch.bfloat16)
    vc = torch.randn_like(kc)
    slots = torch.tensor([2, 0, 3, 7, 1, 6, 4], dtype=torch.int32, device=gpu)
    pos = torch.tensor(lens, dtype=torch.int32, device=gpu)
    cos, sin = ref.rope_tables(1024, D, 500000.0, None, gpu)
    qkv = torch.randn(B, (Hq + 2 * Hkv) * D, device=gpu, dtype=torch.bfloat16)
    kc_ref, vc_ref = kc.clone(), vc.clone()
    q = native().rope_append(qkv, cos, sin, pos, slots, kc, vc, Hq, Hkv, D)
    out = native().decode_attn(q, kc, vc, pos, slots, max(lens) + 1, 1.0 / math.sqrt(D), 1)
    assert torch.equal(native().decode_attn(q, kc, vc, pos, slots, max(lens) + 1, 1.0 / math.sqrt(D), 1), out)
    # with arrival counters the split merge runs inside the attention launch (last-arriving
    # workgroup, sc1 hand-off): bit-identical to the combine kernel, and the counters are
    # back at zero after every call
    cnt = torch.zeros(B * Hkv + 5, dtype=torch.int32, device=gpu)
    for _ in range(3):
        o2 = native().decode_attn(q, kc, vc, pos, slots, max(lens) + 1, 1.0 / math.sqrt(D), 1, None, cnt)
        assert torch.equal(o2, out)
        assert int(cnt.abs().sum()) == 0
    x = qkv.float().view(B, Hq + 2 * Hkv, D)
    for i in range(B):
        p, s = lens[i], int(slots[i])
        c, sn = cos[p].view(1, -1), sin[p].view(1, -1)

        def rot(t):
            return torch.cat([t[..., :D // 2] * c - t[..., D // 2:] * sn, t[..., D // 2:] * c + t[..., :D // 2] * sn], -1)

        qr = rot(x[i, :Hq])
        assert _rel(q[i], qr) < 1e-2
        kc_ref[s, :, p] = rot(x[i, Hq:Hq + Hkv]).to(torch.bfloat16)
        vc_ref[s, :, p] = x[i, Hq + Hkv:].to(torch.bfloat16)
        assert torch.equal(kc[s, :, p], kc_ref[s, :, p]) and torch.equal(vc[s, :, p], vc_ref[s, :, p])
        kk = kc_ref[s, :, :p + 1].float().repeat_interleave(Hq // Hkv, 0)
        vv = vc_ref[s, :, :p + 1].float().repeat_interleave(Hq // Hkv, 0)
        att = (torch.einsum("hd,hld->hl", q[i].float(), kk) / math.sqrt(D)).softmax(-1)
        o = torch.einsum("hl,hld->hd", att, vv)
        assert _rel(out[i].view(Hq, D), o) < 2e-2


def test_sampler(gpu):
    from mxllm.ops import native

    logits = torch.randn(5, 128256, device=gpu)
    assert torch.equal(native().sample(logits, 0.0, 0, 0), logits.argmax(-1))
    # split-vocabulary kernel: odd vocabularies (partial chunks, > 64 chunks), bf16 ties -> smallest index
    for V in (7, 1000, 70001, 200003):
        x = torch.randn(3, V, device=gpu).to(torch.bfloat16)
        x[1, V // 3] = x[1, (2 * V) // 3] = 9.0  # tie across chunks
        assert torch.equal(native().sample(x, 0.0, 0, 0), x.float().argmax(-1)), V
        assert int(native().sample(x, 0.0, 0, 0)[1]) == V // 3
    # temperature sampling follows the softmax distribution (chi-square-ish sanity)
    small = torch.tensor([[0.0, 1.0, 2.0, -1.0]], device=gpu).repeat(4000, 1).contiguous()
    draws = native().sample(small, 1.0, 123, 0).cpu()
    freq = torch.bincount(draws, minlength=4).float() / 4000
    p = torch.softmax(torch.tensor([0.0, 1.0, 2.0, -1.0]), 0)
    assert (freq - p).abs().max().item() < 0.03


def test_engine_gpu_matches_cpu(gpu):
    from mxllm.models import Llama, get_config
    from mxllm.serve.engine import Engine

    cfg = get_config("tiny-d128")
    m = Llama(cfg, device=gpu, seed=3).eval()
    eng = Engine(m, max_batch=4, max_seq=512)
    prompts = [[1, 2, 3, 4, 5], list(range(10, 300)), [7]]
    out = eng.generate(prompts, max_new_tokens=8)
    # recompute greedily with full forwards through the HIP training path
    for p, o in zip(prompts, out):
        seq = list(p)
        with torch.no_grad():
            for _ in range(len(o)):
                seq.append(int(m(torch.tensor([seq], device=gpu))[0, -1].float().argmax()))
        agree = sum(int(a == b) for a, b in zip(o, seq[len(p):]))
        assert agree >= len(o) - 1, (o, seq[len(p):])  # bf16 ties may flip at most one late token


def test_engine_decode_graphs_match_eager(gpu):
    """hipGraph-replayed decode (padded batch buckets, scratch slot) produces
    the same greedy tokens as eager decode, across continuous batching."""
    from mxllm.models import Llama, get_config
    from mxllm.serve.engine import Engine

    cfg = get_config("tiny-d128")
    m = Llama(cfg, device=gpu, seed=5).eval()
    prompts = [[1, 2, 3], list(range(20, 90)), [9, 8], list(range(300, 320)), [4] * 7]
    outs = []
    for graphs in (False, True):
        eng = Engine(m, max_batch=4, max_seq=600, use_graphs=graphs)
        outs.append(eng.generate(prompts, max_new_tokens=40))
        if graphs:
            assert len(eng._graphs) >= 2  # several (batch, key-bound) buckets captured
    for a, b in zip(*outs):
        agree = sum(int(x == y) for x, y in zip(a, b))
        assert agree >= len(a) - 1, (a, b)


@pytest.mark.parametrize("graphs", [False, True])
def test_decode_step_latency(gpu, graphs):
    """Report decode-step time (tiny-d128, batch 4) eager vs graphed."""
    import time

    from mxllm.models import Llama, get_config
    from mxllm.serve.engine import Engine

    m = Llama(get_config("tiny-d128"), device=gpu, seed=5).eval()
    eng = Engine(m, max_batch=4, max_seq=512, use_graphs=graphs)
    for s in range(4):
        eng.prefill(s, [1, 2, 3, 4])
    tok = torch.ones(4, dtype=torch.long, device=gpu)
    for _ in range(3):
        eng.decode([0, 1, 2, 3], tok)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(50):
        eng.decode([0, 1, 2, 3], tok)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / 50 * 1e3
    print(f"decode step tiny-d128 B=4 graphs={graphs}: {ms:.3f} ms")


def test_native_loader_to_gpu(gpu):
    from mxllm.data.loader import TokenLoader

    toks = torch.randint(0, 1000, (20000,), dtype=torch.int32)
    ld = TokenLoader(toks, 256, 4, 0, 1, seed=0, device=gpu)
    ids, lab, _, _ = ld.next_device()
    assert ids.is_cuda and ids.shape == (4, 256) and torch.equal(ids[:, 1:], lab[:, :-1])
    ld.close()


def test_smoke_entry(gpu):
    import __graft_entry__

    __graft_entry__.smoke()


def test_bench_contract_tiny(gpu, tmp_path):
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "b.json"
    r = subprocess.run([sys.executable, "bench.py", "--model", "tiny-d128", "--steps", "2", "--warmup", "1",
                        "--seq-len", "256", "--json-out", str(out), "--dump-outputs", str(tmp_path / "dump")],
                       cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    j = json.loads(out.read_text())
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config"):
        assert k in j
    assert j["value"] > 0 and j["n_gpus"] == 1
    # a plain run (no --full) measures the headline only
    assert "calibration" not in j and not j["gpu_after_timed_steps"] and not [k for k in j if k.startswith("config2")]
    # --dump-outputs: the last step's loss and the parameters it trained, float32
    import numpy as np

    loss, w = np.load(tmp_path / "dump" / "loss.npy"), np.load(tmp_path / "dump" / "trained_params.npy")
    assert loss.dtype == np.float32 and loss.shape == (1,) and abs(float(loss[0]) - j["final_loss"]) < 1e-3
    assert w.dtype == np.float32 and w.size >= j["trainable_params"] and np.isfinite(w).all() and np.any(w != 0)


def test_bench_two_ranks_on_one_gpu(gpu, tmp_path):
    """Rehearse the multi-rank bench path (self-launch of N ranks by
    ``bench.py --gpus 2``, DDP hooks, bucketed all-reduce of GPU grads, barrier,
    max-over-ranks timing) with 2 ranks sharing the one GPU of the test box over
    gloo (RCCL needs one GPU per rank)."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "b2.json"
    env = dict(os.environ, MXLLM_BACKEND="gloo")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--model", "tiny-d128", "--steps", "2",
                        "--warmup", "1", "--seq-len", "256", "--json-out", str(out)], cwd=root, env=env,
                       capture_output=True, text=True, timeout=400)
    assert r.returncode == 0, r.stderr[-3000:]
    j = json.loads(out.read_text())
    assert j["n_gpus"] == 2 and j["config"]["parallelism"] == "dp2" and j["value"] > 0


@pytest.mark.parametrize("parallel", ["ddp", "zero3"])
def test_two_node_scripts_on_one_gpu(gpu, parallel):
    """BASELINE config 5 rehearsal on the GPU: scripts/run_node0.sh + run_node1.sh
    start two torchrun agents ('nodes', one rank each) that rendezvous on
    127.0.0.1 and train the tiny Llama on the box's one GPU through the HIP
    kernels (gloo between the two ranks: RCCL needs one GPU per rank).  ZeRO-3
    with activation checkpointing shards parameters / gradients / optimizer over
    the two nodes.  Reference: /root/reference/scripts/run_node0.sh:10-16."""
    import socket
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, MXLLM_BACKEND="gloo", NPROC_PER_NODE="1", NNODES="2", MASTER_ADDR="127.0.0.1",
               MASTER_PORT=str(port), MXLLM_PG_TIMEOUT_S="120")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        env.pop(k, None)
    args = ["--model", "tiny-d128", "--steps", "3", "--seq-len", "128", "--micro-batch", "1", "--log-every", "1",
            "--finetune", "full", "--parallel", parallel]
    if parallel == "zero3":
        args += ["--activation-checkpointing", "1"]
    p1 = subprocess.Popen(["bash", "scripts/run_node1.sh"] + args, cwd=root, env=env, stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, text=True)
    try:
        p0 = subprocess.run(["bash", "scripts/run_node0.sh"] + args, cwd=root, env=env, capture_output=True,
                            text=True, timeout=240)
        out1, _ = p1.communicate(timeout=120)
    finally:
        if p1.poll() is None:
            p1.kill()
    log = p0.stdout + p0.stderr
    assert p0.returncode == 0 and p1.returncode == 0, log[-2000:] + out1[-2000:]
    assert "step 2" in log and "cuda" in log


def test_zero3_emulated_world8_tiny_gpu(gpu):
    """ZeRO-3 with activation checkpointing and the world-8 emulation on the GPU
    (HIP kernels, direct dW into the unit gradient buffer, async reduce path)."""
    from mxllm.models import get_config
    from mxllm.parallel.runtime import DistEnv
    from mxllm.parallel.zero3 import Zero3Trainer
    from mxllm.train.trainer import OptimConfig

    cfg = get_config("tiny-d128").replace(n_layers=3, vocab_size=1024)
    env = DistEnv(device=gpu, backend="nccl")
    ids = torch.randint(0, cfg.vocab_size, (2, 128), device=gpu)
    losses = {}
    for ck in (False, True):
        tr = Zero3Trainer(cfg, env, OptimConfig(lr=1e-3), seed=3, activation_checkpointing=ck)
        losses[ck] = [float(tr.train_step([(ids, ids)])) for _ in range(3)]
    assert losses[True][-1] < losses[True][0]
    for a, b in zip(losses[False], losses[True]):
        assert abs(a - b) < 1e-3 * max(1.0, abs(a)), losses
    tr8 = Zero3Trainer(cfg, env, OptimConfig(lr=1e-3), seed=3, activation_checkpointing=True, emulate_world=8)
    # sharded units hold 1/8 of their content, the replicated RMSNorm unit all of it
    assert tr8.master.numel() == sum(u.full_numel // (1 if u.replicated else 8) for u in tr8.units)
    for _ in range(2):
        loss = tr8.train_step([(ids, ids)])
    assert torch.isfinite(loss).all()


def test_gpu_monitor_samples(gpu):
    """AMD SMI monitor (A7): the bound device is found by PCI id and reports
    memory / activity fields; the background sampler delivers samples."""
    import threading

    from mxllm.utils.gpumon import GpuMonitor, sample_device

    s = sample_device(gpu.index)
    print("gpu sample:", s)
    assert s and ("vram_total_mb" in s or "gfx_activity_pct" in s), s
    got = []
    ev = threading.Event()

    def cb(x):
        got.append(x)
        if len(got) >= 2:
            ev.set()

    mon = GpuMonitor(gpu, 0.05, cb).start()
    ev.wait(10)
    mon.stop()
    assert len(got) >= 2 and "hbm_allocated_gb" in got[0]


def test_lora_producers_pad_in_place(gpu, monkeypatch):
    """Every LoRA GEMM operand (x and dy) arrives already padded by its producer
    kernel: the augmented path never falls back to a copy on GPU."""
    import importlib

    from mxllm.models import Llama, get_config

    L = importlib.import_module("mxllm.ops.linear")  # (mxllm.ops.linear the attribute is the function)

    calls = {"padded": 0, "copied": 0}
    orig = L._padded_rows

    def spy(t, pad):
        r = orig(t, pad)
        calls["padded" if r is not None else "copied"] += 1
        return r

    monkeypatch.setattr(L, "_padded_rows", spy)
    m = Llama(get_config("tiny-d128"), device=gpu, lora_r=8, seed=2)
    ids = torch.randint(0, 1000, (2, 128), device=gpu)
    m(ids, ids).backward()
    n_lin = 4 * len(m.layers)
    assert calls == {"padded": 2 * n_lin, "copied": 0}, calls


def test_engine_fp8_weights_close_to_bf16(gpu):
    """Serving with e4m3 projection weights: prefill logits stay close to the
    bf16 engine's, and graphed decode runs through the fp8 decode GEMM."""
    from mxllm.models import Llama, get_config
    from mxllm.serve.engine import Engine
    from mxllm.serve.quant import W8Linear, quantize_model_fp8_

    cfg = get_config("tiny-d128")
    prompt = list(range(3, 60))
    ref = Engine(Llama(cfg, device=gpu, seed=9).eval(), max_batch=2, max_seq=256)
    l_ref = ref.prefill(0, prompt)
    m8 = Llama(cfg, device=gpu, seed=9).eval()
    assert quantize_model_fp8_(m8) > 0 and isinstance(m8.layers[0].wgu, W8Linear)
    eng = Engine(m8, max_batch=2, max_seq=256)
    l8 = eng.prefill(0, prompt)
    cos = torch.nn.functional.cosine_similarity(l8.float(), l_ref.float(), dim=0).item()
    assert cos > 0.99, cos
    out = eng.generate([prompt, [1, 2, 3]], max_new_tokens=8)
    assert all(len(o) == 8 for o in out)
    # the fp8 x fp8 path (> SMALL_M tokens per call) against the bf16 reference layer
    from mxllm.serve.quant import dequantize_e4m3

    lin = m8.layers[0].wgu
    x = torch.randn(40, lin.in_features, device=gpu, dtype=torch.bfloat16)
    yr = x.float() @ dequantize_e4m3(lin.q, lin.scale).t()
    assert _rel(lin(x), yr) < 3e-2


@pytest.mark.parametrize("small_m", [8, 16])
def test_engine_fp8_graphed_decode_b16_close_to_bf16(gpu, small_m, monkeypatch):
    """Graphed decode of 16 sequences (the 16-row bucket): per-row logits of the fp8
    engine vs the bf16 engine, both with the default routing (SMALL_M = 8: the
    16-row calls quantise activations per token, W8A8 on hipBLASLt) and with the
    weight-only kernel forced (SMALL_M = 16: W8A16)."""
    from mxllm.models import Llama, get_config
    from mxllm.serve import quant
    from mxllm.serve.engine import Engine

    monkeypatch.setattr(quant, "SMALL_M", small_m)
    cfg = get_config("tiny-d128").replace(n_layers=4)
    g = torch.Generator().manual_seed(3)
    prompts = [torch.randint(3, cfg.vocab_size, (20 + i,), generator=g).tolist() for i in range(16)]
    tok = torch.randint(3, cfg.vocab_size, (16,), generator=g)
    logits = {}
    for kind in ("bf16", "fp8"):
        m = Llama(cfg, device=gpu, seed=21).eval()
        if kind == "fp8":
            quant.quantize_model_fp8_(m)
        eng = Engine(m, max_batch=16, max_seq=128)
        assert eng.use_graphs
        for i, p in enumerate(prompts):
            eng.prefill(i, p)
        logits[kind] = eng.decode(list(range(16)), tok)[:16].float()
    cos = torch.nn.functional.cosine_similarity(logits["fp8"], logits["bf16"], dim=1)
    assert cos.min().item() > 0.99, cos


def test_lora_fused_swiglu_tails_match_unfused(gpu, monkeypatch):
    """The SwiGLU pass writing the down projection's forward tail and the gate-up projection's
    backward tail (no lora_xwt over m / dgu) gives the loss and every adapter gradient of the
    unfused path, and removes exactly those two lora_xwt calls per layer."""
    import importlib

    from mxllm.models import Llama, get_config

    A = importlib.import_module("mxllm.ops.activation")
    Lin = importlib.import_module("mxllm.ops.linear")  # (the mxllm.ops attributes are the functions)

    cfg = get_config("tiny-d128").replace(n_layers=2)

    class Spy:
        def __init__(self, real):
            self.real, self.xwt = real, 0

        def __getattr__(self, k):
            if k == "lora_xwt":
                self.xwt += 1
            return getattr(self.real, k)

    def run(flag):
        monkeypatch.setattr(A, "_FUSE_TAIL", flag)
        spy = Spy(Lin.native())
        monkeypatch.setattr(Lin, "native", lambda: spy)
        m = Llama(cfg, device=gpu, lora_r=16, seed=3)
        with torch.no_grad():
            g = torch.Generator(device=gpu).manual_seed(0)
            for n, p in m.named_parameters():
                p.copy_(torch.randn(p.shape, device=gpu, generator=g).to(p.dtype) * 0.02)
        m.sync_adapters_()
        m.refresh_images_()
        ids = torch.randint(0, cfg.vocab_size, (2, 128), device=gpu, generator=torch.Generator(device=gpu).manual_seed(1))
        loss = m(ids, ids)
        loss.backward()
        return float(loss), {n: p.grad.float() for n, p in m.named_parameters() if p.requires_grad}, spy.xwt

    l0, g0, n0 = run(False)
    l1, g1, n1 = run(True)
    assert n0 - n1 == 2 * cfg.n_layers, (n0, n1)
    assert abs(l0 - l1) < 1e-3 * max(1.0, abs(l0)), (l0, l1)
    for k in g0:
        assert _rel(g1[k], g0[k]) < 2e-2, k


def test_lora_transposed_buffers_match_gpu(gpu, monkeypatch):
    """LoRA projections with TRANSPOSED augmented buffers (forward NN, dX TN GEMM,
    A kept as a k-contiguous copy for the HIP rank-r kernel) give the same loss and
    adapter gradients as the row-major layout, on the HIP path."""
    import mxllm.models.llama as L
    from mxllm.models import get_config

    cfg = get_config("tiny-d128").replace(n_layers=2)

    def run(flag):
        monkeypatch.setattr(L, "LORA_T", flag)
        m = L.Llama(cfg, device=gpu, lora_r=16, seed=3)
        with torch.no_grad():
            g = torch.Generator(device=gpu).manual_seed(0)
            for n, p in m.named_parameters():
                p.copy_(torch.randn(p.shape, device=gpu, generator=g).to(p.dtype) * 0.02)
        m.sync_adapters_()
        m.refresh_images_()  # the transposed [W; A] dX images of the row-major layout follow W
        ids = torch.randint(0, cfg.vocab_size, (2, 128), device=gpu, generator=torch.Generator(device=gpu).manual_seed(1))
        loss = m(ids, ids)
        loss.backward()
        return float(loss), {n: p.grad.float() for n, p in m.named_parameters() if p.requires_grad}

    l0, g0 = run(())
    l1, g1 = run(("qkv", "o", "gu", "d"))
    assert abs(l0 - l1) < 1e-3 * max(1.0, abs(l0)), (l0, l1)
    for k in g0:
        assert _rel(g1[k], g0[k]) < 2e-2, k


def test_ring_attention_one_rank_gpu(gpu):
    """Context-parallel attention path on the GPU kernels (HIP rope_split at
    gathered zigzag positions, flash fwd/bwd per block, LSE merge, rope_merge):
    a one-rank ring equals the plain attention block, forward and backward.
    (Multi-rank rings: tests/test_context_parallel.py on gloo.)"""
    import socket

    import torch.distributed as dist

    from mxllm import ops
    from mxllm.ops import reference as ref
    from mxllm.parallel.context import RingAttention

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        B, S, Hq, Hkv, D = 2, 256, 8, 2, 128
        cos, sin = ref.rope_tables(S, D, 500000.0, None, gpu)
        qkv = (torch.randn(B * S, (Hq + 2 * Hkv) * D, device=gpu) * 0.5).to(torch.bfloat16).requires_grad_(True)
        g = torch.randn(B * S, Hq * D, device=gpu).to(torch.bfloat16)
        o1 = RingAttention(dist.group.WORLD)(qkv, cos, sin, B, S, Hq, Hkv, D)
        (d1,) = torch.autograd.grad(o1, qkv, g)
        o2 = ops.attention_block(qkv, cos, sin, B, S, Hq, Hkv, D, causal=True)
        (d2,) = torch.autograd.grad(o2, qkv, g)
        assert _rel(o1, o2) < 1e-2 and _rel(d1, d2) < 2e-2, (_rel(o1, o2), _rel(d1, d2))
    finally:
        dist.destroy_process_group()


def _tp_gpu_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), MXLLM_BACKEND="gloo", LOCAL_RANK=str(rank))
    import torch.distributed as dist

    from mxllm.models import Llama, get_config
    from mxllm.parallel import runtime
    from mxllm.parallel.tensor import shard_llama
    from mxllm.serve.engine import Engine

    env = runtime.init(rank=rank, world_size=world)
    cfg = get_config("tiny-d128").replace(n_kv_heads=2, n_heads=4)
    full = Llama(cfg, device=env.device, seed=3).eval()
    local = shard_llama(full, rank, world)
    del full
    eng = Engine(local, max_batch=2, max_seq=256, tp_group=dist.group.WORLD)
    logits = eng.prefill_batch([0, 1], [list(range(1, 40)), list(range(50, 67))])
    outs = eng.generate([[5, 6, 7, 8]], max_new_tokens=4)
    if rank == 0:
        q.put((logits.cpu(), outs))
    runtime.cleanup()


def test_tp_engine_two_ranks_one_gpu(gpu):
    """Tensor-parallel serving through the HIP kernels at shard shapes (local
    heads, FFN slice, vocab-parallel head): 2 ranks share the test box's GPU
    over gloo; prefill logits match the unsharded engine."""
    import socket

    import torch.multiprocessing as mp

    from mxllm.models import Llama, get_config
    from mxllm.serve.engine import Engine

    cfg = get_config("tiny-d128").replace(n_kv_heads=2, n_heads=4)
    full = Llama(cfg, device=gpu, seed=3).eval()
    ref_logits = Engine(full, max_batch=2, max_seq=256).prefill_batch([0, 1], [list(range(1, 40)),
                                                                               list(range(50, 67))]).cpu()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_tp_gpu_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    logits, outs = q.get(timeout=180)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    err = ((logits - ref_logits).norm() / ref_logits.norm()).item()
    assert err < 2e-2, err
    assert len(outs[0]) == 4


def test_hf_checkpoint_on_gpu_matches_transformers(gpu, tmp_path):
    """A Hugging Face Llama directory loaded onto the GPU (bf16, HIP kernels) against
    transformers' fp32 CPU forward of the same checkpoint; then one LoRA training
    step on it and a merged export that transformers reads back."""
    transformers = pytest.importorskip("transformers")
    from transformers import LlamaConfig, LlamaForCausalLM

    from mxllm.models import load_hf_llama, save_hf_llama

    cfg = LlamaConfig(vocab_size=512, hidden_size=512, intermediate_size=1024, num_hidden_layers=2,
                      num_attention_heads=4, num_key_value_heads=2, max_position_embeddings=131072,
                      rope_theta=500000.0, rope_scaling={"rope_type": "llama3", "factor": 8.0, "low_freq_factor": 1.0,
                                                         "high_freq_factor": 4.0,
                                                         "original_max_position_embeddings": 8192},
                      rms_norm_eps=1e-5, tie_word_embeddings=False)
    torch.manual_seed(0)
    ref = LlamaForCausalLM(cfg).float().eval()
    ref.save_pretrained(tmp_path / "src", safe_serialization=True)
    m = load_hf_llama(str(tmp_path / "src"), device=gpu, dtype=torch.bfloat16, lora_r=16)
    ids = torch.randint(0, 512, (2, 256))
    with torch.no_grad():
        want = ref(ids).logits
        got = m(ids.to(gpu)).float().cpu()
    assert _rel(got, want) < 2e-2
    opt = torch.optim.SGD([p for p in m.parameters() if p.requires_grad], lr=1e-2)
    loss = m(ids.to(gpu), labels=ids.to(gpu))
    loss.backward()
    opt.step()
    m.sync_adapters_()
    save_hf_llama(m, str(tmp_path / "out"))
    back = LlamaForCausalLM.from_pretrained(str(tmp_path / "out")).float().eval()
    with torch.no_grad():
        got2 = m(ids.to(gpu)).float().cpu()
        want2 = back(ids).logits
    assert _rel(got2, want2) < 2e-2


def test_engine_embeddings_gpu_match_cpu(gpu):
    """/v1/embeddings path on the GPU (final hidden states through the HIP kernels, run on
    the engine thread while it serves) against the CPU reference model."""
    from mxllm.models import Llama, get_config
    from mxllm.serve.engine import Engine

    cfg = get_config("tiny-d128")
    cpu = Llama(cfg, device="cpu", dtype=torch.float32, seed=3).eval()
    g = Llama(cfg, device=gpu, dtype=torch.bfloat16, seed=3).eval()
    with torch.no_grad():
        for pc, pg in zip(cpu.parameters(), g.parameters()):
            pg.copy_(pc.to(pg.dtype))
    eng = Engine(g, max_batch=2, max_seq=256)
    eng.start()
    try:
        seqs = [list(range(5, 70)), list(range(100, 300, 3))]
        got = eng.embed(seqs)
        want = Engine(cpu, max_batch=2, max_seq=256).embed(seqs)
    finally:
        eng.stop()
    assert got.shape == want.shape
    assert (torch.nn.functional.cosine_similarity(got, want, dim=1) > 0.995).all()


def test_swiglu_recompute_bitwise_gpu(gpu, monkeypatch):
    """Selective checkpointing on the HIP path: recomputing m = swiglu(gu) and the normed projection
    inputs in the backward of the un-checkpointed layers gives bitwise the loss and gradients of
    saving them (same kernels)."""
    import mxllm.models.llama as L
    from mxllm.models import get_config

    cfg = get_config("tiny-d128").replace(n_layers=3)
    ids = torch.randint(0, cfg.vocab_size, (2, 128), device=gpu, generator=torch.Generator(device=gpu).manual_seed(0))

    def run(policy, ck=1):
        monkeypatch.setattr(L, "RECOMPUTE_SWIGLU", policy)
        m = L.Llama(cfg, device=gpu, seed=4, activation_checkpointing=ck)
        loss = m(ids, ids)
        loss.backward()
        return float(loss), {n: p.grad.float().clone() for n, p in m.named_parameters()}

    l0, g0 = run("0")
    for ck in (1, 0):  # also the normed qkv / gate-up inputs (ops.normed_linear), every layer at ck 0
        l1, g1 = run("auto", ck)
        assert l0 == l1
        for k in g0:
            assert torch.equal(g0[k], g1[k]), (ck, k)
