#!/usr/bin/env python3
"""Decode-step cost of per-request LoRA adapters (mxllm/ops/lora_serve.py, csrc/kernels/lora_serve.hip).

One GPU, random-init bf16 weights, every sequence holding --ctx cached tokens, the hipGraph-replayed
decode step of the serving engine at each batch in --batches:

  a          an engine without adapter tables (today's fused step)
  a_unfused  the same engine class with the GEMM prologue / epilogue fusions switched off
             (RMSNorm, RoPE + cache append, SwiGLU as their own kernels): what an adapter step runs
             besides the delta kernels
  b          adapter tables allocated, no row using an adapter (replays the graph of a)
  c          every row on a distinct adapter
  d          every row on the same adapter

The configurations are timed in alternation, --repeats rounds of --decode-steps replays each ended by
a device synchronise; per configuration the median round is reported with the min..max spread.
c - a is the feature's cost per step (reported per layer and per delta launch, 8 per layer);
c - a_unfused is the share of the two gather kernels alone.  Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama3.1-8b")
    ap.add_argument("--ctx", type=int, default=1024)
    ap.add_argument("--batches", default="1,8,32,64")
    ap.add_argument("--decode-steps", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--kv-cache", choices=["bf16", "fp8"], default="bf16")
    ap.add_argument("--json-out", default=None)
    a = ap.parse_args()

    from mxllm.models import Llama, get_config
    from mxllm.serve import engine as E

    if not torch.cuda.is_available():
        raise SystemExit("lora_serve_bench measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = get_config(a.model)
    model = Llama(cfg, device=dev, dtype=torch.bfloat16, seed=0)
    model.requires_grad_(False)
    batches = [int(b) for b in a.batches.split(",")]
    bmax = max(batches)
    max_seq = a.ctx + a.decode_steps + 16  # every timed round starts again at ctx cached tokens
    kw = dict(max_batch=bmax, max_seq=max_seq, kv_dtype=a.kv_cache, use_graphs=True)
    eng_a = E.Engine(model, **kw)
    eng_l = E.Engine(model, max_adapters=bmax, max_lora_rank=a.rank, **kw)
    g = torch.Generator(device=dev).manual_seed(1)
    for lay in eng_l.lora.layers:  # random adapters of the full rank in every slot, s = 2
        for t in lay.values():
            t.a.normal_(0.0, 0.02, generator=g)
            t.b.normal_(0.0, 0.02, generator=g)
            t.s.fill_(2.0)
            t.scales[:] = [2.0] * t.n_adapters
    eng_l.adapters = {f"adapter{i}": i for i in range(bmax)}
    # the unfused base step: the flags are read when the step is captured
    fused = (E._NORM_FUSED, E._ROPE_FUSED, E._SWIGLU_FUSED)
    eng_u = E.Engine(model, **kw)

    gh = torch.Generator().manual_seed(0)
    out = {"model": a.model, "ctx": a.ctx, "rank": a.rank, "kv_cache_dtype": a.kv_cache, "layers": cfg.n_layers,
           "adapter_table_gb": round(eng_l.lora.nbytes() / 1e9, 2), "decode_steps": a.decode_steps,
           "repeats": a.repeats, "decode": []}
    for bs in batches:
        slots = list(range(bs))
        tok = torch.randint(0, cfg.vocab_size, (bs,), generator=gh)
        configs = {"a": (eng_a, None), "a_unfused": (eng_u, None), "b": (eng_l, [-1] * bs),
                   "c": (eng_l, list(range(bs))), "d": (eng_l, [0] * bs)}

        def run(name, steps):
            eng, ad = configs[name]
            if name == "a_unfused":
                E._NORM_FUSED = E._ROPE_FUSED = E._SWIGLU_FUSED = False
            for s in slots:
                eng.lens[s] = a.ctx
                if ad is not None:
                    eng.slot_adapter[s] = ad[s]
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(steps):
                eng.decode(slots, tok)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t) / steps
            E._NORM_FUSED, E._ROPE_FUSED, E._SWIGLU_FUSED = fused
            return 1e3 * dt

        for name in configs:  # capture + warm every shape the timed window uses
            run(name, 3)
        times = {name: [] for name in configs}
        for _ in range(a.repeats):
            for name in configs:
                times[name].append(run(name, a.decode_steps))
        row = {"batch": bs}
        for name, ts in times.items():
            row[name] = {"ms_per_step": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}
        med = {n: statistics.median(ts) for n, ts in times.items()}
        cost = med["c"] - med["a"]
        row["c_minus_a"] = {"ms_per_step": round(cost, 4), "us_per_layer": round(1e3 * cost / cfg.n_layers, 2),
                            "us_per_delta_launch": round(1e3 * cost / (8 * cfg.n_layers), 2)}
        kern = med["c"] - med["a_unfused"]
        row["c_minus_a_unfused"] = {"ms_per_step": round(kern, 4),
                                    "us_per_delta_launch": round(1e3 * kern / (8 * cfg.n_layers), 2)}
        row["b_minus_a_ms"] = round(med["b"] - med["a"], 4)
        row["d_minus_c_ms"] = round(med["d"] - med["c"], 4)
        out["decode"].append(row)
        for eng in (eng_a, eng_u, eng_l):
            for s in slots:
                eng.lens[s] = 0
                eng.slot_adapter[s] = -1
    del eng_a, eng_u, eng_l
    torch.cuda.empty_cache()
    from mxllm.utils.calibrate import calibrate

    out["calibration"] = calibrate(dev)  # the box itself: 8192^3 bf16 GEMM TF/s, 4 GiB copy TB/s
    line = json.dumps(out)
    print(line, flush=True)
    if a.json_out:
        with open(a.json_out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
