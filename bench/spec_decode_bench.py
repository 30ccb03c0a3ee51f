"""Speculative decoding: what a verify step costs and what it buys.

(a) ``--part kernel``: ``verify_attn`` / ``verify_attn_kv8`` (n rows per sequence, K/V streamed once) against
    ``decode_attn`` / ``decode_attn_kv8`` over the same B * n rows as B * n sequences (K/V streamed n times),
    B in {1, 8, 64}, context in {1k, 8k}, n in {2, 4}, Llama-3.1 8B heads (32 over 8) and 70B heads (64 over 8:
    n = 4 is the two-column-block kernel), paged pools.
(b) ``--part engine``: an engine with random bf16 weights (``--model``, default llama3.1-8b).  ms per graphed
    step with n = 1 .. K + 1 rows per sequence (an engine with ``speculate = n - 1``, every row in use) against
    the plain graphed step (``speculate`` off: the parent commit's step), batch 1 / 8, context 1k: the cost
    ratio that decides whether the feature pays.
(c) ``--part tokens``: tokens/s of ``generate`` with injected drafters of known acceptance -- none right, two
    of three right, all right (the record is the plain engine's output, then the "none right" run's own: see
    the comment there; the acceptance the counters report is printed beside each figure) -- and with the
    prompt-lookup drafter on a prompt that repeats its own text, against the plain engine, batch 1 / 8.  Host clock around ``generate`` (every step ends in a read-back).

Kernels and steps: device events around a window of calls sized to at least 40 ms, the two sides of a
comparison alternating round by round in one process, the median of the rounds reported with their spread.
One JSON line per measurement, then the box's calibration line (mxllm/utils/calibrate.py).

  python bench/spec_decode_bench.py --part kernel,engine,tokens [--json-out out.jsonl]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

D, BLK = 128, 256


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / n  # seconds per call


def calls_for(fn, min_s=0.04):
    """Calls per window so that a window lasts at least ``min_s``."""
    for _ in range(3):
        fn()
    t = window(fn, 5)
    return max(5, int(math.ceil(min_s / max(t, 1e-7))))


def alternate(fns: dict, rounds: int):
    """{name: median seconds per call, name_spread: (max - min) / median} of ``fns``, alternating per round."""
    n = {k: calls_for(f) for k, f in fns.items()}
    ts = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            ts[k].append(window(f, n[k]))
    out = {}
    for k, v in ts.items():
        med = statistics.median(v)
        out[k] = med
        out[k + "_spread"] = (max(v) - min(v)) / med
    return out


def kernel_part(a, dev, emit):
    from mxllm.ops import native

    ops = native()
    scale = 1.0 / math.sqrt(D)
    for hq, hkv in ((int(x) for x in h.split(":")) for h in a.heads.split(",")):
        for B in (int(v) for v in a.batch.split(",")):
            for ctx in (int(v) for v in a.context.split(",")):
                nb = (ctx + 8 + BLK - 1) // BLK
                g = torch.Generator().manual_seed(ctx + B)
                bt = torch.stack([torch.randperm(nb, generator=g) + b * nb for b in range(B)]).to(torch.int32).to(dev)
                kp = torch.randn(B * nb, hkv, BLK, D, device=dev, dtype=torch.bfloat16)
                vp = torch.randn(B * nb, hkv, BLK, D, device=dev, dtype=torch.bfloat16)
                kc, ks = ops.kv8_quant_rows(kp.view(-1, D))
                vc, vs = ops.kv8_quant_rows(vp.view(-1, D))
                k8 = [kc.view(kp.shape), ks.view(kp.shape[:3]), vc.view(vp.shape), vs.view(vp.shape[:3])]
                for n in (int(v) for v in a.rows.split(",")):
                    if n * (hq // hkv) > 32:
                        continue
                    q = torch.randn(B * n, hq, D, device=dev, dtype=torch.bfloat16)
                    lens = torch.full((B,), ctx, dtype=torch.int32, device=dev)
                    nq = torch.full((B,), n, dtype=torch.int32, device=dev)
                    slots = torch.arange(B, dtype=torch.int32, device=dev)
                    rl = (lens.view(B, 1) + torch.arange(n, dtype=torch.int32, device=dev)).reshape(-1).contiguous()
                    rs = slots.repeat_interleave(n).contiguous()
                    ml = ctx + n
                    for fmt in ("bf16", "fp8"):
                        if fmt == "bf16":
                            fns = {"verify": lambda: ops.verify_attn(q, kp, vp, lens, nq, slots, n, ml, scale, bt),
                                   "decode_rows": lambda: ops.decode_attn(q, kp, vp, rl, rs, ml, scale, 1, bt, None)}
                        else:
                            fns = {"verify": lambda: ops.verify_attn_kv8(q, *k8, lens, nq, slots, n, ml, scale, bt),
                                   "decode_rows": lambda: ops.decode_attn_kv8(q, *k8, rl, rs, ml, scale, 1, bt)}
                        same = torch.equal(fns["verify"](), fns["decode_rows"]())
                        r = alternate(fns, a.rounds)
                        row_bytes = 256 if fmt == "bf16" else 132
                        emit(dict(part="kernel", kv=fmt, Hq=hq, Hkv=hkv, B=B, context=ctx, n=n, bitwise_equal=same,
                                  verify_us=r["verify"] * 1e6, decode_rows_us=r["decode_rows"] * 1e6,
                                  speedup=r["decode_rows"] / r["verify"], verify_spread=r["verify_spread"],
                                  decode_rows_spread=r["decode_rows_spread"],
                                  verify_gbps=2 * B * hkv * (ctx + n) * row_bytes / r["verify"] / 1e9))
                del kp, vp, k8


_MODELS = {}


def _model(a, dev):
    from mxllm.models import build_model

    if a.model not in _MODELS:  # both engine parts share the weights
        _MODELS[a.model] = build_model(a.model, device=str(dev), seed=0).eval()
    return _MODELS[a.model]


def _prompts(vocab, B, ctx, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(3, vocab - 3, (ctx,), generator=g).tolist() for _ in range(B)]


def engine_part(a, dev, emit):
    from mxllm.serve.engine import Engine

    model = _model(a, dev)
    cfg = model.cfg
    kmax = min(a.k, 32 // (cfg.n_heads // cfg.n_kv_heads) - 1)
    ctx = a.engine_context
    for kv in a.kv.split(","):
        for B in (int(v) for v in a.engine_batch.split(",")):
            prompts = _prompts(cfg.vocab_size, B, ctx)
            slots = list(range(B))
            engines = {0: Engine(model, max_batch=B, max_seq=ctx + 64, kv_dtype=kv)}
            for k in range(1, kmax + 1):
                engines[k] = Engine(model, max_batch=B, max_seq=ctx + 64, kv_dtype=kv, speculate=k)
            for e in engines.values():
                e.prefill_batch(slots, prompts)
            tok = torch.full((B,), 7, dtype=torch.long)

            def plain(e=engines[0]):
                e.decode(slots, tok)
                for s in slots:
                    e.lens[s] = ctx  # the same step again

            fns = {"n1_plain": plain}
            for k in range(1, kmax + 1):
                fns[f"n{k + 1}"] = lambda e=engines[k], k=k: e.verify(slots, [[7] * (k + 1)] * B)
            r = alternate(fns, a.rounds)
            base = r["n1_plain"]
            for name in fns:
                n = int(name[1:].split("_")[0])
                emit(dict(part="engine", model=a.model, kv=kv, batch=B, context=ctx, rows_per_sequence=n,
                          step_ms=r[name] * 1e3, spread=r[name + "_spread"], ratio_to_plain=r[name] / base,
                          ratio_to_n_plain_steps=r[name] / (n * base)))
            del engines


def tokens_part(a, dev, emit):
    from mxllm.serve.engine import Engine

    model = _model(a, dev)
    cfg = model.cfg
    K = min(a.k, 32 // (cfg.n_heads // cfg.n_kv_heads) - 1)
    ctx, new = a.engine_context, a.new_tokens

    def timed(eng, prompts):
        eng.generate(prompts, max_new_tokens=new)  # captures the graphs
        for key in ("spec_steps", "spec_draft_tokens", "spec_accepted_tokens", "steps"):
            setattr(eng, key, 0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs = eng.generate(prompts, max_new_tokens=new)
        torch.cuda.synchronize()
        return outs, time.perf_counter() - t0

    for B in (int(v) for v in a.engine_batch.split(",")):
        prompts = _prompts(cfg.vocab_size, B, ctx, seed=3)
        plain = Engine(model, max_batch=B, max_seq=ctx + new + 8)
        record, t_plain = timed(plain, prompts)
        emit(dict(part="tokens", model=a.model, batch=B, context=ctx, new_tokens=new, drafter="plain engine",
                  tokens_per_s=B * new / t_plain, steps=plain.steps))
        del plain

        def drafter(kind):
            def draft(tokens, k):
                for p, out in zip(prompts, record):
                    if tokens[:len(p)] == p:
                        at = len(tokens) - len(p)
                        right = out[at:at + k]
                        if kind == "all right":
                            return right
                        if kind == "none right":
                            return [(t + 1) % cfg.vocab_size for t in right[:1]] * k
                        return [t if j % 3 < 2 else (t + 1) % cfg.vocab_size for j, t in enumerate(right)]
                return []

            return draft

        for kind in ("none right", "two of three right", "all right"):
            eng = Engine(model, max_batch=B, max_seq=ctx + new + 8, speculate=K, drafter=drafter(kind))
            outs, t = timed(eng, prompts)
            st = eng.stats()
            emit(dict(part="tokens", model=a.model, batch=B, context=ctx, new_tokens=new, K=K, drafter=kind,
                      tokens_per_s=B * new / t, speedup=t_plain / t, steps=eng.steps, spec_steps=st["spec_steps"],
                      draft_tokens=st["spec_draft_tokens"], accepted_tokens=st["spec_accepted_tokens"],
                      same_tokens_as_record=outs == record))
            # The GEMMs of a verify step run over K + 1 times the rows of a plain step and round differently,
            # and the logits of a random model tie often: where this run left the plain engine's stream, its own
            # output (verify-step logits throughout) is the record the next drafters are right about.
            record = outs
            del eng
        # prompt lookup on a prompt that repeats its own text (a random model does not continue the pattern:
        # the acceptance printed here is what the drafter finds in this model's output, not a language model's)
        unit = _prompts(cfg.vocab_size, 1, 64, seed=9)[0]
        rep = [(unit * (ctx // 64 + 1))[:ctx] for _ in range(B)]
        plain = Engine(model, max_batch=B, max_seq=ctx + new + 8)
        _, t_plain = timed(plain, rep)
        del plain
        eng = Engine(model, max_batch=B, max_seq=ctx + new + 8, speculate=K)
        _, t = timed(eng, rep)
        st = eng.stats()
        emit(dict(part="tokens", model=a.model, batch=B, context=ctx, new_tokens=new, K=K, drafter="prompt lookup",
                  tokens_per_s=B * new / t, plain_tokens_per_s=B * new / t_plain, speedup=t_plain / t, steps=eng.steps,
                  spec_steps=st["spec_steps"], draft_tokens=st["spec_draft_tokens"],
                  accepted_tokens=st["spec_accepted_tokens"]))
        del eng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="kernel,engine,tokens")
    ap.add_argument("--heads", default="32:8,64:8")
    ap.add_argument("--batch", default="1,8,64")
    ap.add_argument("--context", default="1024,8192")
    ap.add_argument("--rows", default="2,4")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--model", default="llama3.1-8b")
    ap.add_argument("--kv", default="bf16")
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--engine-batch", default="1,8")
    ap.add_argument("--engine-context", type=int, default=1024)
    ap.add_argument("--new-tokens", type=int, default=128)
    ap.add_argument("--json-out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = open(a.json_out, "a") if a.json_out else None

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    with torch.no_grad():
        for part in a.part.split(","):
            {"kernel": kernel_part, "engine": engine_part, "tokens": tokens_part}[part](a, dev, emit)
    try:
        from mxllm.utils.calibrate import calibrate

        emit(dict(part="calibration", **calibrate(dev)))
    except Exception as e:  # noqa: BLE001
        emit(dict(part="calibration", error=str(e)))


if __name__ == "__main__":
    main()
