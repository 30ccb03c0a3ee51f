"""Multi-adapter LoRA serving on the CPU: the reference op, PEFT adapter files, the engine's adapter
mode on ``tiny``, the server and the client (inputs and references: tests/_lora_serve.py)."""
import json
import os
import socket
import subprocess
import sys
import threading
import time

import pytest
import torch

from mxllm.data.tokenizer import ByteTokenizer
from mxllm.models import Llama, get_config
from mxllm.models import adapter as AD
from mxllm.serve import client
from mxllm.serve.engine import Engine, SamplingParams
from tests import _lora_serve as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16 = torch.bfloat16
PROMPTS = [[5, 9, 77, 1, 300], [3, 4], list(range(20, 43)), [7, 7, 7, 8]]


# =========================================================================== reference op
@pytest.mark.parametrize("si", [0, 1])
def test_reference_op_against_per_row_fp64_loop(si):
    from mxllm.ops import lora_delta_rows_

    K, sp, r = L.SHAPES[si]
    c = L.make_case(K, sp, r, 5)
    y = c["y0"].clone()
    lora_delta_rows_(y, c["x"], c["ids"], L.tables_of(c))
    want = c["y0"].double().clone()
    for b, aid in enumerate(c["ids"].tolist()):
        if aid < 0:
            continue
        t = c["a"][aid].double() @ c["x"][b].double()
        off = 0
        for i, n in enumerate(sp):
            for col in range(off, off + n):
                want[b, col] += float(c["s"][aid]) * float(t[i * r:(i + 1) * r] @ c["b"][aid, col].double())
            off += n
    live = c["ids"] >= 0
    assert torch.equal(y[~live].view(torch.int16), c["y0"][~live].view(torch.int16))  # rows with id -1 keep their bits
    from tests._parity import assert_parity

    assert_parity(y[live], want[live], L.LORA_DELTA_Y, name="CPU reference op")
    assert not torch.equal(y[live], c["y0"][live])
    # the segments form gives the same bits as the ids form
    y2 = c["y0"].clone()
    lora_delta_rows_(y2, c["x"], None, L.tables_of(c), segments=L.segments_of(c["ids"]))
    assert torch.equal(y2.view(torch.int16), y.view(torch.int16))


def test_adapter_tables_put_and_clear():
    from mxllm.ops import AdapterTables

    cfg = get_config("tiny")
    tabs = AdapterTables(cfg, 2, 16, "cpu", max_rows=4)
    ad = L.random_adapter(cfg, 8, 1)
    tabs.put(1, ad)
    t = tabs.layers[1]["wqkv"]
    A, B = ad["weights"][(1, "k_proj")]
    assert torch.equal(t.a[1, 16:24], A) and not t.a[1, 24:32].any() and not t.a[0].any()
    assert torch.equal(t.b[1, cfg.q_dim:cfg.q_dim + cfg.kv_dim, :8], B) and not t.b[1, :, 8:].any()
    assert float(t.s[1]) == ad["scaling"] == t.scales[1]
    tabs.clear(1)
    assert not any(x.a.any() or x.b.any() or x.s.any() for lay in tabs.layers for x in lay.values())
    with pytest.raises(ValueError):
        tabs.put(0, L.random_adapter(cfg, 32, 1))
    with pytest.raises(ValueError):
        tabs.put(2, ad)


# =========================================================================== adapter files
def _write_peft_dir(path, cfg, r=4, projections=("q_proj", "v_proj"), config=None, tensors=None):
    """A hand-built PEFT directory (what ``peft``'s save_pretrained writes for a Llama)."""
    from safetensors.torch import save_file

    os.makedirs(path, exist_ok=True)
    ad = L.random_adapter(cfg, r, 11, alpha=8.0, projections=projections)
    sd = {}
    for (i, p), (A, B) in ad["weights"].items():
        mod = "self_attn" if p in ("q_proj", "k_proj", "v_proj", "o_proj") else "mlp"
        sd[f"base_model.model.model.layers.{i}.{mod}.{p}.lora_A.weight"] = A
        sd[f"base_model.model.model.layers.{i}.{mod}.{p}.lora_B.weight"] = B
    sd.update(tensors or {})
    conf = {"peft_type": "LORA", "r": r, "lora_alpha": 8.0, "target_modules": list(projections), "bias": "none",
            "task_type": "CAUSAL_LM", "lora_dropout": 0.05}
    conf.update(config or {})
    with open(os.path.join(path, "adapter_config.json"), "w") as f:
        json.dump(conf, f)
    save_file(sd, os.path.join(path, "adapter_model.safetensors"))
    return ad


def test_load_hand_built_peft_directory_subset_of_projections(tmp_path):
    cfg = get_config("tiny")
    want = _write_peft_dir(str(tmp_path / "a"), cfg)
    got = AD.load_adapter(str(tmp_path / "a"), cfg, r_max=16)
    assert got["r"] == 4 and got["scaling"] == 2.0 and set(got["weights"]) == set(want["weights"])
    for k, (A, B) in want["weights"].items():
        assert torch.equal(got["weights"][k][0], A) and torch.equal(got["weights"][k][1], B)
    from mxllm.ops import AdapterTables

    tabs = AdapterTables(cfg, 1, 16, "cpu", max_rows=2)
    tabs.put(0, got)  # the other five projections stay zero
    t = tabs.layers[0]["wqkv"]
    assert t.a[0, :4].any() and not t.a[0, 16:32].any() and t.a[0, 32:36].any()
    assert all(not tabs.layers[i][p].a.any() and not tabs.layers[i][p].b.any() for i in range(cfg.n_layers)
               for p in ("wo", "wgu", "wd"))
    _write_peft_dir(str(tmp_path / "rs"), cfg, config={"use_rslora": True})
    assert AD.load_adapter(str(tmp_path / "rs"), cfg)["scaling"] == 8.0 / 2.0  # alpha / sqrt(r)


def test_load_adapter_rejections(tmp_path):
    cfg = get_config("tiny")
    bad = {
        "dora": dict(config={"use_dora": True}),
        "modules_to_save": dict(config={"modules_to_save": ["lm_head"]}),
        "bias": dict(config={"bias": "all"}),
        "unknown target": dict(config={"target_modules": ["q_proj", "v_proj", "embed_tokens"]}),
        "not lora": dict(config={"peft_type": "IA3"}),
        "wrong shape": dict(tensors={"base_model.model.model.layers.0.self_attn.q_proj.lora_A.weight":
                                     torch.zeros(4, cfg.hidden + 8, dtype=BF16)}),
        "unexpected tensor": dict(tensors={"base_model.model.lm_head.lora_A.weight": torch.zeros(4, 8, dtype=BF16)}),
    }
    for name, kw in bad.items():
        _write_peft_dir(str(tmp_path / name), cfg, **kw)
        with pytest.raises(ValueError):
            AD.load_adapter(str(tmp_path / name), cfg, r_max=16)
    _write_peft_dir(str(tmp_path / "r32"), cfg, r=32)
    with pytest.raises(ValueError, match="rank"):
        AD.load_adapter(str(tmp_path / "r32"), cfg, r_max=16)
    assert AD.load_adapter(str(tmp_path / "r32"), cfg, r_max=32)["r"] == 32


def _lora_model(cfg, r=8, seed=3):
    m = Llama(cfg, lora_r=r, lora_alpha=16.0, seed=seed).eval()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for layer in m.layers:
            for lin in (layer.wqkv, layer.wo, layer.wgu, layer.wd):
                for blk in lin.lora_b_blocks():
                    blk.copy_(torch.randn(blk.shape, generator=g) * 0.05)
        m.sync_adapters_()
    return m


def test_save_adapter_names_shapes_and_round_trip(tmp_path):
    from safetensors.torch import load_file

    cfg = get_config("tiny")
    m = _lora_model(cfg)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    AD.save_adapter(m, a)
    sd = load_file(os.path.join(a, "adapter_model.safetensors"))
    assert len(sd) == cfg.n_layers * 7 * 2
    for i in range(cfg.n_layers):
        for p, (mod, _, _) in AD.PROJECTIONS.items():
            n_out, n_in = AD.proj_shape(cfg, p)
            assert tuple(sd[f"base_model.model.model.layers.{i}.{mod}.{p}.lora_A.weight"].shape) == (8, n_in)
            assert tuple(sd[f"base_model.model.model.layers.{i}.{mod}.{p}.lora_B.weight"].shape) == (n_out, 8)
    conf = json.load(open(os.path.join(a, "adapter_config.json")))
    assert conf["peft_type"] == "LORA" and conf["r"] == 8 and conf["lora_alpha"] == 16.0
    assert sorted(conf["target_modules"]) == sorted(AD.PROJECTIONS) and conf["bias"] == "none"
    lay = m.layers[1].wqkv  # k_proj: rows q_dim.., columns r..2r of the block-diagonal B; rows r..2r of the stacked A
    assert torch.equal(sd["base_model.model.model.layers.1.self_attn.k_proj.lora_A.weight"], lay.lora_a[8:16])
    assert torch.equal(sd["base_model.model.model.layers.1.self_attn.k_proj.lora_B.weight"],
                       lay.lora_b[cfg.q_dim:cfg.q_dim + cfg.kv_dim, 8:16])
    # save -> load -> save: bitwise
    AD.save_adapter(AD.load_adapter(a, cfg, r_max=16), b)
    for fn in ("adapter_config.json", "adapter_model.safetensors"):
        assert open(os.path.join(a, fn), "rb").read() == open(os.path.join(b, fn), "rb").read(), fn
    # an off-diagonal block of lora_b has no place in PEFT's layout
    with torch.no_grad():
        m.layers[0].wgu.lora_b[0, 8] = 0.5
    with pytest.raises(ValueError, match="off-diagonal"):
        AD.save_adapter(m, str(tmp_path / "c"))


# =========================================================================== engine on tiny
@pytest.fixture(scope="module")
def tiny():
    cfg = get_config("tiny")
    model = Llama(cfg, seed=0).eval()
    ads = {"a0": L.random_adapter(cfg, 16, 1), "a1": L.random_adapter(cfg, 8, 2)}
    eng = Engine(model, max_batch=4, max_seq=256, max_adapters=2, max_lora_rank=16)
    for n, a in ads.items():
        eng.load_adapter(n, a)
    return cfg, model, ads, eng


def test_base_requests_unchanged_and_mixed_batch_equals_alone(tiny):
    cfg, model, ads, eng = tiny
    plain = Engine(model, max_batch=4, max_seq=256)
    assert plain.lora is None
    base = plain.generate(PROMPTS, max_new_tokens=6)
    assert eng.generate(PROMPTS, max_new_tokens=6) == base  # base requests in an adapter-enabled engine
    names = ["a0", None, "a1", "a0"]
    mixed = eng.generate(PROMPTS, max_new_tokens=6, adapters=names)
    alone = [eng.generate([p], max_new_tokens=6, adapters=[n])[0] for p, n in zip(PROMPTS, names)]
    assert mixed == alone
    assert mixed[1] == base[1]
    assert all(mixed[i] != base[i] for i in (0, 2, 3))  # the adapters change the output
    assert eng.stats()["lora_adapters"] == ["a0", "a1"]


def test_engine_logits_against_fp64(tiny):
    """Teacher-forced prefill + decode logits of a mixed batch against the fp64 forward with each row's
    adapter unmerged; bound: twice the base engine's own error (measured here, same prompts)."""
    cfg, model, ads, eng = tiny
    prompts, names = PROMPTS[:3], ["a0", "a1", None]
    forced = [[11, 12, 13], [14, 15, 16], [17, 18, 19]]

    def run(e, use):
        outs = [e.prefill_batch([0, 1, 2], prompts, use)]
        for st in range(3):
            outs.append(e.decode([0, 1, 2], torch.tensor([f[st] for f in forced])).float())
        for s in range(3):
            e.lens[s] = 0
            e.slot_adapter[s] = -1
        return torch.stack(outs, 1).double()

    def err(out, use):
        worst = 0.0
        for i, n in enumerate(use):
            ref = L.forward_fp64(model, prompts[i] + forced[i], ads.get(n))[len(prompts[i]) - 1:]
            worst = max(worst, float(((out[i] - ref).abs() / ref.abs().amax(-1, keepdim=True)).max()))
        return worst

    base_err = err(run(Engine(model, max_batch=4, max_seq=256), None), [None] * 3)
    got = err(run(eng, names), names)
    assert 0 < got <= 2 * base_err, (got, base_err)
    wrong = err(run(eng, names), ["a1", "a0", None])  # against the swapped adapters: far outside
    assert wrong > 20 * base_err, (wrong, base_err)


def test_unload_refused_while_in_use_then_slot_reused(tiny):
    cfg, model, ads, _ = tiny
    eng = Engine(model, max_batch=2, max_seq=128, max_adapters=1)
    assert eng.load_adapter("x", ads["a0"]) == 0
    with pytest.raises(ValueError, match="slots"):
        eng.load_adapter("y", ads["a1"])
    with pytest.raises(ValueError, match="already"):
        eng.load_adapter("x", ads["a1"])
    r = eng.submit([1, 2, 3], SamplingParams(max_new_tokens=3), adapter="x")
    with pytest.raises(ValueError, match="in use"):
        eng.unload_adapter("x")  # waiting
    eng.step()
    assert not r.done.is_set()
    with pytest.raises(ValueError, match="in use"):
        eng.unload_adapter("x")  # active
    while not r.done.is_set():
        eng.step()
    out_x = list(r.output)
    eng.unload_adapter("x")
    assert eng.adapters == {} and not eng.lora.layers[0]["wqkv"].a.any()
    assert eng.load_adapter("y", ads["a1"]) == 0  # the slot is reused
    out_y = eng.generate([[1, 2, 3]], max_new_tokens=3, adapters=["y"])[0]
    ref = Engine(model, max_batch=2, max_seq=128, max_adapters=1)
    ref.load_adapter("y", ads["a1"])
    assert out_y == ref.generate([[1, 2, 3]], max_new_tokens=3, adapters=["y"])[0] and out_y != out_x
    with pytest.raises(ValueError):
        eng.unload_adapter("x")


def test_unknown_adapter_finishes_with_error_and_misuse_raises(tiny):
    cfg, model, ads, eng = tiny
    r = eng.generate([[1, 2, 3]], max_new_tokens=2, adapters=["nope"], return_requests=True)[0]
    assert r.finish_reason == "error" and "nope" in r.error and r.output == []
    plain = Engine(model, max_batch=2, max_seq=64)
    r = plain.generate([[1, 2, 3]], max_new_tokens=2, adapters=["a0"], return_requests=True)[0]
    assert r.finish_reason == "error"
    with pytest.raises(ValueError):
        plain.load_adapter("a0", ads["a0"])
    with pytest.raises(ValueError, match="single-GPU"):
        Engine(model, max_batch=2, max_seq=64, max_adapters=1, tp_group=object())
    with pytest.raises(NotImplementedError):
        eng.score([[1, 2, 3]], adapter="a0")
    with pytest.raises(NotImplementedError):
        eng.embed([[1, 2, 3]], adapter="a0")


def test_fp8_weights_with_adapter():
    """W8Linear projections: the delta is added to whatever the projection returned; the logits stay
    within the fp8 engine's own distance from bf16 (tests/test_serve.py test_fp8_weight_engine_cpu)."""
    from mxllm.serve.quant import W8Linear, quantize_model_fp8_

    cfg = get_config("tiny")
    ad = L.random_adapter(cfg, 8, 5)
    prompt = [5, 9, 77, 1, 300, 12, 44]
    m8 = Llama(cfg, seed=4).eval()
    quantize_model_fp8_(m8)
    assert isinstance(m8.layers[0].wd, W8Linear)
    engs = [Engine(m, max_batch=2, max_seq=128, max_adapters=1) for m in (Llama(cfg, seed=4).eval(), m8)]
    for e in engs:
        e.load_adapter("a", ad)
    l16, l8 = (e.prefill_batch([0], [prompt], ["a"])[0] for e in engs)
    base8 = Engine(m8, max_batch=2, max_seq=128).prefill(0, prompt)
    cos = torch.nn.functional.cosine_similarity
    assert cos(l8, l16, dim=0).item() > 0.99
    assert cos(l8, base8, dim=0).item() < 0.9  # and the adapter is applied
    assert len(engs[1].generate([prompt], max_new_tokens=4, adapters=["a"])[0]) == 4


# =========================================================================== server and client
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.fixture(scope="module")
def served(tiny):
    import uvicorn

    from mxllm.serve.server import build_app

    cfg, model, ads, _ = tiny
    eng = Engine(model, max_batch=4, max_seq=256, max_adapters=2)
    eng.load_adapter("a0", ads["a0"])
    port = _free_port()
    srv = uvicorn.Server(uvicorn.Config(build_app(eng, ByteTokenizer(512), "tiny-base"), host="127.0.0.1", port=port,
                                        log_level="error"))
    th = threading.Thread(target=srv.run, daemon=True)
    th.start()
    for _ in range(200):
        if srv.started:
            break
        time.sleep(0.05)
    yield f"http://127.0.0.1:{port}/v1", eng, ads["a0"]
    srv.should_exit = True
    th.join(10)
    eng.stop()


def test_server_routes_model_names_to_adapters(served):
    import httpx

    url, eng, a0 = served
    assert [m["id"] for m in httpx.get(url + "/models", timeout=10).json()["data"]] == ["tiny-base", "a0"]
    assert "mxllm_lora_adapters 1" in httpx.get(url.replace("/v1", "") + "/metrics", timeout=10).text

    def chat(model):
        return httpx.post(url + "/chat/completions", timeout=60, json={
            "model": model, "messages": [{"role": "user", "content": "hello"}], "max_tokens": 6}).json()

    def text(model, **kw):
        return httpx.post(url + "/completions", timeout=60, json=dict({"model": model, "prompt": "hello", "max_tokens": 6},
                                                                      **kw))

    def stream(model):
        with httpx.stream("POST", url + "/chat/completions", timeout=60, json={
                "model": model, "messages": [{"role": "user", "content": "hello"}], "max_tokens": 6, "stream": True}) as s:
            lines = [json.loads(ln[6:]) for ln in s.iter_lines() if ln.startswith("data: {")]
        return "".join(c["choices"][0].get("delta", {}).get("content") or "" for c in lines)

    base, other, ad = chat("tiny-base"), chat("some-other-name"), chat("a0")
    assert base["choices"][0]["message"] == other["choices"][0]["message"]  # not an adapter: the base model
    assert ad["choices"][0]["message"] != base["choices"][0]["message"] and ad["model"] == "a0"
    assert stream("a0") == ad["choices"][0]["message"]["content"] != stream("tiny-base")
    tb, ta = text("tiny-base").json(), text("a0").json()
    assert ta["choices"][0]["text"] != tb["choices"][0]["text"]
    # the same tokens as the engine gives directly
    tok = ByteTokenizer(512)
    ids = tok.encode("hello")
    direct = Engine(eng.model, max_batch=2, max_seq=256, max_adapters=1)
    direct.load_adapter("a0", a0)
    want = direct.generate([ids], max_new_tokens=6, adapters=["a0"])[0]
    assert ta["choices"][0]["text"] == tok.decode([t for t in want if t not in direct.eos_ids])
    assert text("a0", echo=True, logprobs=1).status_code == 400  # prompt scoring with an adapter
    assert text("tiny-base", echo=True, logprobs=1).status_code == 200


def test_local_completion_reaches_the_adapter(tmp_path):
    from mxllm.serve.local import ensure_local_engine

    cfg = get_config("tiny")
    AD.save_adapter(L.random_adapter(cfg, 8, 7), str(tmp_path / "ad"))
    try:
        eng, _ = ensure_local_engine("tiny-lora-local", "cpu", max_batch=2, max_seq=256,
                                     adapters={"my-adapter": str(tmp_path / "ad")})
        assert eng.adapters == {"my-adapter": 0}
        msgs = [{"role": "user", "content": "hi"}]
        base = client.completion("tiny-lora-local", msgs, api_base="local", max_tokens=6)
        ad = client.completion("my-adapter", msgs, api_base="local", max_tokens=6)
        assert ad.choices[0].message.content != base.choices[0].message.content
        assert ad.usage["completion_tokens"] >= 1
        t_ad = client.text_completion("my-adapter", "hi", api_base="local", max_tokens=6, logprobs=0)
        t_base = client.text_completion("tiny-lora-local", "hi", api_base="local", max_tokens=6, logprobs=0)
        assert t_ad.choices[0].logprobs["token_logprobs"] != t_base.choices[0].logprobs["token_logprobs"]
    finally:
        client.unregister_local("tiny-lora-local")


def test_trainer_save_adapter_serves_the_trained_model(tmp_path):
    """A LoRA run with --save-adapter writes a PEFT directory that ``load_adapter`` accepts; served
    on the base weights it gives the LoRA model's logits.  Both are compared with the fp64 forward
    (adapter unmerged) under twice the base engine's own error at the same prompt."""
    out = tmp_path / "adapter"
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "src/distributed_finetuning.py", "--model", "tiny", "--finetune", "lora",
                        "--lora-r", "8", "--lora-alpha", "16", "--lr", "3e-2", "--steps", "3", "--seq-len", "32",
                        "--micro-batch", "1", "--seed", "0", "--save-adapter", str(out)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    cfg = get_config("tiny")
    ad = AD.load_adapter(str(out), cfg, r_max=16)
    assert ad["r"] == 8 and ad["scaling"] == 2.0 and len(ad["weights"]) == cfg.n_layers * 7
    assert any(bool(B.any()) for _, B in ad["weights"].values())  # training moved B off zero
    lm = Llama(cfg, lora_r=8, lora_alpha=16.0, seed=0).eval()  # the run's base weights (frozen) ...
    AD.apply_adapter_(lm, ad)  # ... with the trained adapter
    base = Llama(cfg, seed=0).eval()
    with torch.no_grad():
        src = dict(lm.named_parameters())
        for n, q in base.named_parameters():
            q.copy_(src[n])
    prompt = list(range(30, 50))
    ref_base = L.forward_fp64(base, prompt)[-1]
    ref = L.forward_fp64(base, prompt, ad)[-1]
    nerr = lambda x, rf: float((x.double() - rf).abs().max() / rf.abs().max())  # noqa: E731
    base_err = nerr(Engine(base, max_batch=2, max_seq=128).prefill(0, prompt), ref_base)
    eng = Engine(base, max_batch=2, max_seq=128, max_adapters=1)
    eng.load_adapter("trained", str(out))
    got = eng.prefill_batch([0], [prompt], ["trained"])[0]
    with torch.no_grad():
        fwd = lm(torch.tensor([prompt]))[0, -1].float()
    assert nerr(got, ref) <= 2 * base_err and nerr(fwd, ref) <= 2 * base_err, (nerr(got, ref), nerr(fwd, ref), base_err)
    assert nerr(got, ref_base) > 4 * base_err  # the adapter matters
