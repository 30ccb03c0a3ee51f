"""OpenAI-compatible HTTP server backed by the mxllm engine.

Endpoints: POST /v1/chat/completions, POST /v1/completions (both with
optional SSE streaming), GET /v1/models, GET /health, GET /metrics
(Prometheus text).  This is the local stand-in for the "LiteLLM-compatible
API endpoint" hosting Llama-3.1-70B that the reference calls remotely
(reference README.md:18, docs/setup_guide.md:10).

Run:  python -m mxllm.serve.server --model llama3.1-8b --port 8000
"""
from __future__ import annotations

import argparse
import asyncio
import json
import logging
import os
import time
import uuid

import torch
from fastapi import FastAPI, HTTPException, Request
from fastapi.responses import JSONResponse, PlainTextResponse, StreamingResponse

from .engine import Engine, SamplingParams

log = logging.getLogger("mxllm.server")


def _stop_ids(tok, stop):
    if not stop:
        return ()
    if isinstance(stop, str):
        stop = [stop]
    ids = []
    for s in stop:
        enc = tok.encode(s, bos=False)
        if len(enc) == 1:
            ids.append(enc[0])
    return tuple(ids)


def build_app(engine: Engine, tokenizer, model_name: str, api_key: str | None = None):
    app = FastAPI(title="mxllm OpenAI-compatible server")
    engine.start()
    stats = {"requests": 0, "errors": 0, "prompt_tokens": 0, "completion_tokens": 0}

    def auth(req: Request):
        if api_key:
            h = req.headers.get("authorization", "")
            if h != f"Bearer {api_key}":
                raise HTTPException(status_code=401, detail="invalid api key")

    def sampling_params(body, chat: bool) -> SamplingParams:
        """The request body's sampling fields (both routes, streaming or not).  Raises
        ValueError on a bad value (answered with HTTP 400)."""
        try:
            if chat:
                lp = body.get("logprobs")
                if lp not in (None, True, False):
                    raise ValueError("logprobs must be a boolean on /chat/completions")
                top = body.get("top_logprobs")
                if top is not None and not lp:
                    raise ValueError("top_logprobs needs logprobs: true")
                logprobs = (0 if top is None else top) if lp else None
            else:
                logprobs = body.get("logprobs")
            if logprobs is not None and (isinstance(logprobs, bool) or not isinstance(logprobs, int)):
                raise ValueError(f"logprobs / top_logprobs must be an integer in 0..20, got {logprobs!r}")
            bias = body.get("logit_bias")
            if bias is not None and not isinstance(bias, dict):
                raise ValueError("logit_bias must be an object of token id -> bias")
            return SamplingParams(
                max_new_tokens=int(body.get("max_tokens") or body.get("max_completion_tokens") or 128),
                temperature=float(body.get("temperature", 0.0) or 0.0),
                top_p=float(body.get("top_p", 1.0) or 1.0),
                top_k=int(body.get("top_k", 0) or 0),
                stop_ids=_stop_ids(tokenizer, body.get("stop")),
                seed=int(body.get("seed", 0) or 0),
                presence_penalty=float(body.get("presence_penalty") or 0.0),
                frequency_penalty=float(body.get("frequency_penalty") or 0.0),
                repetition_penalty=float(1.0 if body.get("repetition_penalty") is None
                                         else body["repetition_penalty"]),
                logit_bias=bias or None,
                logprobs=logprobs,
            )
        except TypeError as e:
            raise ValueError(str(e)) from None

    def bad_request(e):
        return JSONResponse({"error": {"message": str(e), "type": "invalid_request_error"}}, status_code=400)

    def adapter_of(body):
        """The request's ``model`` when it names a loaded LoRA adapter, else None (the base model)."""
        name = body.get("model")
        return name if isinstance(name, str) and name in engine.adapters else None

    async def run(prompt_ids, params, adapter=None):
        r = engine.submit(prompt_ids, params, adapter)
        while not r.done.is_set():
            await asyncio.sleep(0.002)
        if r.error:
            stats["errors"] += 1
            if "logit_bias" in r.error or "LoRA adapter" in r.error:  # rejected at admission: the caller's mistake
                raise ValueError(r.error)
            raise HTTPException(status_code=500, detail=r.error)
        stats["prompt_tokens"] += len(prompt_ids)
        stats["completion_tokens"] += len(r.output)
        return r

    def tok_str(t: int) -> str:
        return tokenizer.decode([t])

    def chat_logprobs(toks, entries):
        """OpenAI chat shape: one entry per token with its top list."""
        def one(t, lp):
            s_ = tok_str(t)
            return {"token": s_, "logprob": lp, "bytes": list(s_.encode("utf-8"))}

        return {"content": [dict(one(t, e[0]), top_logprobs=[one(i, l) for i, l in e[1]])
                            for t, e in zip(toks, entries)]}

    def text_logprobs(toks, entries, offset: int = 0):
        """OpenAI completions shape; ``entries`` may start with None (the first prompt token)."""
        out = {"tokens": [], "token_logprobs": [], "top_logprobs": [], "text_offset": []}
        for t, e in zip(toks, entries):
            s_ = tok_str(t)
            out["tokens"].append(s_)
            out["token_logprobs"].append(None if e is None else e[0])
            out["top_logprobs"].append(None if e is None else {tok_str(i): l for i, l in e[1]})
            out["text_offset"].append(offset)
            offset += len(s_)
        return out

    def usage(r):
        u = {"prompt_tokens": len(r.prompt), "completion_tokens": len(r.output),
             "total_tokens": len(r.prompt) + len(r.output)}
        if getattr(engine, "prefix_cache", False):  # OpenAI's field: prompt tokens served from the prefix cache
            u["prompt_tokens_details"] = {"cached_tokens": r.cached_tokens}
        return u

    @app.get("/health")
    async def health():
        return {"status": "ok", "model": model_name, "active": len(engine.active), "waiting": len(engine.waiting)}

    @app.get("/v1/models")
    async def models():
        data = [{"id": model_name, "object": "model", "owned_by": "mxllm"}]
        data += [{"id": a, "object": "model", "owned_by": "mxllm", "parent": model_name} for a in sorted(engine.adapters)]
        return {"object": "list", "data": data}

    @app.get("/metrics")
    async def metrics():
        lines = [f"mxllm_requests_total {stats['requests']}", f"mxllm_errors_total {stats['errors']}",
                 f"mxllm_prompt_tokens_total {stats['prompt_tokens']}",
                 f"mxllm_completion_tokens_total {stats['completion_tokens']}",
                 f"mxllm_engine_steps_total {engine.steps}", f"mxllm_active_sequences {len(engine.active)}",
                 f"mxllm_waiting_requests {len(engine.waiting)}",
                 f"mxllm_ttft_seconds_sum {engine.ttft_sum:.6f}", f"mxllm_ttft_seconds_count {engine.finished}",
                 f"mxllm_request_latency_seconds_sum {engine.latency_sum:.6f}",
                 f"mxllm_request_latency_seconds_count {engine.finished}",
                 f"mxllm_prefill_tokens_total {engine.prefill_tokens}",
                 f"mxllm_prefix_cache_query_tokens_total {getattr(engine, 'prefix_query_tokens', 0)}",
                 f"mxllm_prefix_cache_hit_tokens_total {getattr(engine, 'prefix_hit_tokens', 0)}",
                 f"mxllm_prefill_chunks_total {getattr(engine, 'prefill_chunks', 0)}",
                 f"mxllm_spec_steps_total {getattr(engine, 'spec_steps', 0)}",
                 f"mxllm_spec_draft_tokens_total {getattr(engine, 'spec_draft_tokens', 0)}",
                 f"mxllm_spec_accepted_tokens_total {getattr(engine, 'spec_accepted_tokens', 0)}",
                 f"mxllm_prefill_seconds_total {engine.prefill_s:.6f}",
                 f"mxllm_decode_tokens_total {engine.decode_tokens}",
                 f"mxllm_decode_seconds_total {engine.decode_s:.6f}",
                 f'mxllm_kv_cache_info{{kv_cache_dtype="{engine.kv_dtype}"}} 1',
                 f"mxllm_kv_cache_bytes {engine.kv.nbytes()}", f"mxllm_lora_adapters {len(engine.adapters)}"]
        return PlainTextResponse("\n".join(lines) + "\n")

    @app.post("/v1/chat/completions")
    @app.post("/chat/completions")
    async def chat(req: Request):
        auth(req)
        body = await req.json()
        stats["requests"] += 1
        msgs = body.get("messages") or []
        ids = tokenizer.apply_chat_template(msgs)
        try:
            params = sampling_params(body, chat=True)
            if body.get("stream"):
                return StreamingResponse(_stream(ids, params, chat=True, adapter=adapter_of(body)),
                                         media_type="text/event-stream")
            r = await run(ids, params, adapter_of(body))
        except ValueError as e:
            return bad_request(e)
        text = tokenizer.decode([t for t in r.output if t not in engine.eos_ids])
        choice = {"index": 0, "message": {"role": "assistant", "content": text}, "finish_reason": r.finish_reason}
        if params.logprobs is not None:
            choice["logprobs"] = chat_logprobs(r.output, r.logprobs)
        return JSONResponse({
            "id": f"chatcmpl-{uuid.uuid4().hex[:24]}", "object": "chat.completion", "created": int(time.time()),
            "model": body.get("model", model_name), "choices": [choice], "usage": usage(r)})

    @app.post("/v1/completions")
    @app.post("/completions")
    async def completions(req: Request):
        auth(req)
        body = await req.json()
        stats["requests"] += 1
        prompt = body.get("prompt", "")
        prompt = prompt if isinstance(prompt, str) else prompt[0]
        ids = tokenizer.encode(prompt)
        echo = bool(body.get("echo"))
        try:
            params = sampling_params(body, chat=False)
            if body.get("stream"):
                return StreamingResponse(_stream(ids, params, chat=False, adapter=adapter_of(body)),
                                         media_type="text/event-stream")
            scored = None
            if echo and params.logprobs is not None:  # prompt scoring: one full forward, no KV cache
                scored = (await asyncio.get_running_loop().run_in_executor(
                    None, engine.score, [ids], params.logprobs, adapter_of(body)))[0]
            if echo and body.get("max_tokens") == 0:  # nothing generated
                out, out_lp, reason = [], [], "length"
                use = {"prompt_tokens": len(ids), "completion_tokens": 0, "total_tokens": len(ids)}
                stats["prompt_tokens"] += len(ids)
            else:
                r = await run(ids, params, adapter_of(body))
                out, out_lp, reason, use = r.output, r.logprobs, r.finish_reason, usage(r)
        except (ValueError, NotImplementedError) as e:
            return bad_request(e)
        text = tokenizer.decode([t for t in out if t not in engine.eos_ids])
        choice = {"index": 0, "text": (prompt + text) if echo else text, "finish_reason": reason}
        if params.logprobs is not None:
            if scored is not None:
                choice["logprobs"] = text_logprobs(list(ids) + list(out), scored + list(out_lp))
            else:
                choice["logprobs"] = text_logprobs(out, out_lp, len(prompt) if echo else 0)
        return JSONResponse({
            "id": f"cmpl-{uuid.uuid4().hex[:24]}", "object": "text_completion", "created": int(time.time()),
            "model": body.get("model", model_name), "choices": [choice], "usage": use})

    @app.post("/v1/embeddings")
    @app.post("/embeddings")
    async def embeddings(req: Request):
        """OpenAI embeddings: ``input`` a string, a list of strings, a token list or a
        list of token lists; mean-pooled final hidden states, unit norm."""
        auth(req)
        body = await req.json()
        stats["requests"] += 1
        inp = body.get("input", "")
        if inp == "" or inp == [] or (isinstance(inp, list) and any(x == "" or x == [] for x in inp)):
            return JSONResponse({"error": {"message": "empty input", "type": "invalid_request_error"}},
                                status_code=400)
        if isinstance(inp, str):
            seqs = [tokenizer.encode(inp)]
        elif inp and all(isinstance(x, int) for x in inp):
            seqs = [list(inp)]
        else:
            seqs = [tokenizer.encode(x) if isinstance(x, str) else list(x) for x in inp]
        if not seqs or any(not q for q in seqs):
            return JSONResponse({"error": {"message": "empty input", "type": "invalid_request_error"}},
                                status_code=400)
        try:
            vec = await asyncio.get_running_loop().run_in_executor(None, engine.embed, seqs, adapter_of(body))
        except (ValueError, NotImplementedError) as e:
            return JSONResponse({"error": {"message": str(e), "type": "invalid_request_error"}}, status_code=400)
        n = sum(len(q) for q in seqs)
        return JSONResponse({
            "object": "list", "model": body.get("model", model_name),
            "data": [{"object": "embedding", "index": i, "embedding": v.tolist()} for i, v in enumerate(vec)],
            "usage": {"prompt_tokens": n, "total_tokens": n}})

    async def _stream(ids, params, chat: bool, adapter=None):
        r = engine.submit(ids, params, adapter)
        sent = 0
        cid = f"chatcmpl-{uuid.uuid4().hex[:24]}"
        while True:
            done = r.done.is_set()
            toks = r.output[sent:]
            if toks:
                text = tokenizer.decode([t for t in toks if t not in engine.eos_ids])
                if chat:
                    choice = {"index": 0, "delta": {"content": text}, "finish_reason": None}
                else:
                    choice = {"index": 0, "text": text, "finish_reason": None}
                if params.logprobs is not None:  # the entries of this chunk's tokens
                    ent = r.logprobs[sent:sent + len(toks)]
                    choice["logprobs"] = chat_logprobs(toks, ent) if chat else text_logprobs(toks, ent)
                sent += len(toks)
                chunk = {"id": cid, "object": "chat.completion.chunk" if chat else "text_completion",
                         "model": model_name, "choices": [choice]}
                yield f"data: {json.dumps(chunk)}\n\n"
            if done and sent >= len(r.output):
                break
            await asyncio.sleep(0.005)
        fin = {"id": cid, "object": "chat.completion.chunk" if chat else "text_completion", "model": model_name,
               "choices": [{"index": 0, ("delta" if chat else "text"): ({} if chat else ""),
                            "finish_reason": r.finish_reason}]}
        yield f"data: {json.dumps(fin)}\n\n"
        yield "data: [DONE]\n\n"

    @app.on_event("shutdown")
    async def _shutdown():
        engine.stop()

    return app


def build_default(model: str = "tiny", device: str | None = None, max_batch: int = 8, max_seq: int = 2048,
                  checkpoint: str | None = None, tokenizer_path: str | None = None, seed: int = 0,
                  weights: str = "bf16", tp_group=None, kv_cache: str | None = None, adapters: dict | None = None,
                  max_loras: int | None = None, max_lora_rank: int = 16, prefix_cache: bool | None = None,
                  prefill_chunk: int | None = None, kv_pool_tokens: int | None = None, speculate: int | None = None):
    """Engine + tokenizer.  ``tp_group``: this rank serves its tensor-parallel
    shard (mxllm/parallel/tensor.py) of the model; the full model is built (or
    loaded) on the rank's GPU, sliced and freed.  ``kv_cache``: "bf16" / "fp8" KV cache
    (None: env MXLLM_KV_CACHE, default bf16; ``Engine(kv_dtype=...)``).  ``adapters``: {name: PEFT
    LoRA directory} served beside the base model (``max_loras`` table slots, default one per adapter,
    each of rank <= ``max_lora_rank``); a request whose ``model`` is such a name runs on that adapter.
    ``prefix_cache`` / ``prefill_chunk`` / ``kv_pool_tokens``: the engine's options of the same names
    (None: their env variables).  ``speculate`` = K: speculative decoding with up to K prompt-lookup
    drafts per request and step (``Engine(speculate=K)``; None: env MXLLM_SPECULATE)."""
    from ..data.tokenizer import get_tokenizer
    from ..models import build_model, tokenizer_path_for

    if device is None:
        device = "cuda" if torch.cuda.is_available() else "cpu"
    # ``model``: a preset name or a Hugging Face Llama directory (its weights and tokenizer.json)
    m = build_model(model, device=device, seed=seed)
    cfg = m.cfg
    tokenizer_path = tokenizer_path_for(model, tokenizer_path)
    if checkpoint:
        from ..train.checkpoint import load_model_weights

        load_model_weights(m, checkpoint)
    m.eval()
    if tp_group is not None:
        import torch.distributed as dist

        from ..parallel.tensor import shard_llama

        m = shard_llama(m, dist.get_rank(tp_group), dist.get_world_size(tp_group))
        if str(device).startswith("cuda"):
            torch.cuda.empty_cache()
    if weights == "fp8":
        from .quant import quantize_model_fp8_

        quantize_model_fp8_(m)
    elif weights == "mxfp4":  # after shard_llama: a TP rank quantises its own slice
        from .quant import quantize_model_mxfp4_

        quantize_model_mxfp4_(m)
    tok = get_tokenizer(cfg.vocab_size, tokenizer_path, cfg.bos_id, cfg.eos_id)
    eng = Engine(m, max_batch=max_batch, max_seq=max_seq, eos_ids=(cfg.eos_id, getattr(tok, "eos_id", cfg.eos_id)),
                 tp_group=tp_group, kv_dtype=kv_cache,
                 max_adapters=max(max_loras or 0, len(adapters or {})), max_lora_rank=max_lora_rank,
                 prefix_cache=prefix_cache, prefill_chunk=prefill_chunk, kv_pool_tokens=kv_pool_tokens,
                 speculate=speculate)
    for name, path in (adapters or {}).items():
        eng.load_adapter(name, path)
    return eng, tok


def parse_lora_modules(items) -> dict:
    """``NAME=DIR`` arguments of ``--lora`` -> {name: dir}."""
    out = {}
    for it in items or ():
        name, sep, path = it.partition("=")
        if not sep or not name or not path or name in out:
            raise SystemExit(f"--lora takes NAME=DIR with distinct names, got {it!r}")
        out[name] = path
    return out


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default=os.environ.get("MXLLM_MODEL", "tiny"),
                    help="preset name, or a Hugging Face Llama directory (config.json + safetensors + tokenizer.json)")
    ap.add_argument("--host", default="127.0.0.1")
    ap.add_argument("--port", type=int, default=8000)
    ap.add_argument("--max-batch", type=int, default=8)
    ap.add_argument("--max-seq", type=int, default=2048)
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--tokenizer", default=None)
    ap.add_argument("--api-key", default=os.environ.get("MXLLM_API_KEY"))
    ap.add_argument("--served-name", default=None)
    ap.add_argument("--weights", choices=["bf16", "fp8", "mxfp4"],
                    default=os.environ.get("MXLLM_ENGINE_WEIGHTS", "bf16"),
                    help="fp8: e4m3 projection weights; mxfp4: OCP MXFP4 projection weights, e2m1 codes with one "
                         "e8m0 scale per 32 (serving quantisation, mxllm/serve/quant.py)")
    ap.add_argument("--tp", type=int, default=1,
                    help="tensor-parallel degree: launch with torchrun --nproc-per-node=TP; rank 0 serves HTTP, "
                         "the other ranks follow its schedule")
    ap.add_argument("--kv-cache", choices=["bf16", "fp8"], default=os.environ.get("MXLLM_KV_CACHE") or "bf16",
                    help="fp8: e4m3 KV cache, one byte per element and one f32 scale per (token, KV head) row "
                         "(head_dim 128; mxllm/serve/kvcache.py)")
    ap.add_argument("--lora", action="append", default=[], metavar="NAME=DIR",
                    help="serve a PEFT LoRA adapter directory under NAME beside the base model (repeatable); "
                         "a request whose model is NAME runs on it")
    ap.add_argument("--max-loras", type=int, default=None, help="adapter table slots (default: one per --lora)")
    ap.add_argument("--max-lora-rank", type=int, default=16, choices=[8, 16, 32, 64],
                    help="rank of the adapter tables; adapters of a lower rank are zero-padded")
    ap.add_argument("--kv-pool-tokens", type=int, default=None,
                    help="paged KV cache: a pool of that many tokens shared by all slots (env MXLLM_KV_POOL_TOKENS)")
    ap.add_argument("--prefix-cache", action="store_true", default=None,
                    help="share the KV blocks of common prompt prefixes between requests (needs the paged KV "
                         "cache: --kv-pool-tokens; bf16 KV cache, --tp 1; env MXLLM_PREFIX_CACHE=1)")
    ap.add_argument("--prefill-chunk", type=int, default=None, metavar="N",
                    help="prefill at most N prompt tokens per engine step, so a long prompt does not stall the "
                         "streaming requests (bf16 KV cache, --tp 1; env MXLLM_PREFILL_CHUNK)")
    ap.add_argument("--speculative-ngram", type=int, default=None, metavar="K",
                    help="speculative decoding: verify up to K tokens per request and step, drafted by n-gram "
                         "lookup in the request's own prompt and output (no draft model; --tp 1; K + 1 times the "
                         "q-heads per KV head at most 32; env MXLLM_SPECULATE)")
    return ap.parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s - %(levelname)s - %(message)s")
    group, env = None, None
    if a.tp > 1:
        import torch.distributed as dist

        from ..parallel import runtime

        env = runtime.init()
        if env.world_size != a.tp:
            raise SystemExit(f"--tp {a.tp} needs exactly {a.tp} ranks (torchrun --nproc-per-node={a.tp})")
        group = dist.group.WORLD
    eng, tok = build_default(a.model, None, a.max_batch, a.max_seq, a.checkpoint, a.tokenizer, weights=a.weights,
                             tp_group=group, kv_cache=a.kv_cache, adapters=parse_lora_modules(a.lora),
                             max_loras=a.max_loras, max_lora_rank=a.max_lora_rank, prefix_cache=a.prefix_cache,
                             prefill_chunk=a.prefill_chunk, kv_pool_tokens=a.kv_pool_tokens,
                             speculate=a.speculative_ngram)
    if group is not None:
        eng.enable_tp_sync()
        if env.rank != 0:
            try:
                eng.follow()
            finally:
                runtime.cleanup()
            return
    app = build_app(eng, tok, a.served_name or os.path.basename(os.path.normpath(a.model)), a.api_key)
    import uvicorn

    try:
        uvicorn.run(app, host=a.host, port=a.port, log_level="warning")
    finally:
        if group is not None:
            eng.stop()
            runtime.cleanup()


if __name__ == "__main__":
    main()
