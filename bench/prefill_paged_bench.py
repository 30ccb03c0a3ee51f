"""Paged-KV prefill attention, prefix cache and chunked prefill: what they cost and what they buy.

(a) ``--part kernel``: the attention of one 2,048-token chunk at position p0 of a slot, Llama-3.1 8B heads
    (Hq 32, Hkv 8, D 128), over a paged pool with a permuted block table: the HIP kernel
    (``prefill_attn_paged``), the gather route (rows made contiguous, then ``attn_fwd``) and, at p0 = 0,
    plain ``attn_fwd`` on contiguous K/V -- in one process, alternating round by round.  Time: device events
    around a window of calls, per call; FLOPs: 4 Hq D sum_t (p0 + t + 1), what causal attention needs.
(b) ``--part engine``: an 8B engine (random bf16 weights).  TTFT of a 2,048-token shared prefix plus a
    128-token tail, miss against hit, and with the options off; and the largest gap between two decode steps
    of 8 streaming requests while a 32k-token prompt is admitted (the second such prompt: the first one captures
    the decode graphs of its batch and key bucket), with the options off and with
    ``prefill_chunk`` unset (prefix cache only), 2048 and 8192.  Time: host clock around steps that end in the
    sampler's read-back (a device synchronise).

One JSON line per measurement, then the box's calibration line (mxllm/utils/calibrate.py).

  python bench/prefill_paged_bench.py --part kernel,engine [--json-out out.jsonl]
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

HQ, HKV, D, BLK = 32, 8, 128, 256


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / n  # seconds per call


def kernel_part(a, dev, emit):
    from mxllm.ops import native
    from mxllm.ops.decode import paged_attention_gather

    ops = native()
    scale = 1.0 / math.sqrt(D)
    n = a.chunk
    for p0 in (int(v) for v in a.p0.split(",")):
        L = p0 + n
        nb = (L + BLK - 1) // BLK
        g = torch.Generator().manual_seed(p0 + 1)
        perm = torch.randperm(nb + 3, generator=g)[:nb].to(torch.int32)  # a permuted table over a larger pool
        kp = torch.randn(nb + 3, HKV, BLK, D, device=dev, dtype=torch.bfloat16)
        vp = torch.randn(nb + 3, HKV, BLK, D, device=dev, dtype=torch.bfloat16)
        bt_host = perm.view(1, nb)
        bt = bt_host.to(dev)
        q = torch.randn(n, HQ, D, device=dev, dtype=torch.bfloat16)
        segs = [(0, n, 0, p0)]
        segs_t = torch.tensor(segs, dtype=torch.int32)
        out_h = torch.empty(n, HQ * D, device=dev, dtype=torch.bfloat16)
        out_g = torch.empty_like(out_h)
        runs = {"hip": lambda: ops.prefill_attn_paged(q, kp, vp, bt, segs_t, scale, out_h),
                "gather": lambda: paged_attention_gather(q, kp, vp, bt_host, segs, scale, out_g)}
        if p0 == 0:
            qh = q.transpose(0, 1).contiguous().unsqueeze(0)
            kc = torch.randn(1, HKV, n, D, device=dev, dtype=torch.bfloat16)
            vc = torch.randn(1, HKV, n, D, device=dev, dtype=torch.bfloat16)
            runs["attn_fwd"] = lambda: ops.attn_fwd(qh, kc, vc, True, scale)
        t = {}
        for name, fn in runs.items():  # warm up, size the window
            fn()
            torch.cuda.synchronize()
            one = window(fn, 3)
            t[name] = (fn, max(3, int(a.window_ms * 1e-3 / max(one, 1e-7))), [])
        for _ in range(a.rounds):
            for name in runs:
                fn, reps, acc = t[name]
                acc.append(window(fn, reps))
        # the two routes compute the same thing (same rounding points): compare at the size that is timed
        diff = (out_h.float() - out_g.float()).abs().max().item()
        flops = 4.0 * HQ * D * (n * p0 + n * (n + 1) / 2)
        res = {"part": "kernel", "Hq": HQ, "Hkv": HKV, "D": D, "n": n, "p0": p0, "max_abs_diff_hip_gather": diff}
        for name in runs:
            ts = sorted(t[name][2])
            med = ts[len(ts) // 2]
            res[name] = {"us": round(med * 1e6, 1), "us_min": round(ts[0] * 1e6, 1), "us_max": round(ts[-1] * 1e6, 1),
                         "tflops": round(flops / med / 1e12, 1), "calls_per_window": t[name][1]}
        res["hip_over_gather"] = round(res["gather"]["us"] / res["hip"]["us"], 3)
        emit(res)
        del kp, vp, q
        torch.cuda.empty_cache()


def engine_part(a, dev, emit):
    from mxllm.models import Llama, get_config
    from mxllm.serve.engine import Engine, SamplingParams

    cfg = get_config(a.model)
    model = Llama(cfg, device=dev, dtype=torch.bfloat16, seed=0)
    model.requires_grad_(False)
    g = torch.Generator().manual_seed(0)

    def prompt(n):
        return torch.randint(3, cfg.vocab_size - 3, (n,), generator=g).tolist()

    # ---- TTFT: shared prefix + tail, miss against hit, against the options off
    pool = 16 * (a.prefix + a.tail + 64)
    for label, kw in (("options_off", {}), ("prefix_cache", dict(prefix_cache=True))):
        eng = Engine(model, max_batch=2, max_seq=a.prefix + a.tail + 64, kv_pool_tokens=pool, eos_ids=(-1,), **kw)
        eng.generate([prompt(a.prefix + a.tail)], max_new_tokens=2)  # warm up: kernels, workspaces, graphs
        first, second = [], []
        for _ in range(a.rounds):
            pre = prompt(a.prefix)
            for acc in (first, second):  # a new prefix, then the same prefix with another tail
                r = eng.generate([pre + prompt(a.tail)], max_new_tokens=2, return_requests=True)[0]
                acc.append((r.t_first - r.t_submit, r.cached_tokens))
        res = {"part": "ttft", "engine": label, "model": a.model, "prefix": a.prefix, "tail": a.tail}
        for name, acc in (("first_request", first), ("same_prefix_again", second)):
            ts = sorted(x for x, _ in acc)
            res[name] = {"ttft_ms": round(statistics.median(ts) * 1e3, 2), "min": round(ts[0] * 1e3, 2),
                         "max": round(ts[-1] * 1e3, 2), "cached_tokens": sorted({c for _, c in acc})}
        emit(res)
        del eng
        torch.cuda.empty_cache()

    # ---- the largest inter-token gap of streaming requests while a long prompt is admitted
    n_stream, long_n = a.streams, a.long_prompt
    max_seq = long_n + 256
    pool = n_stream * 1024 + long_n + 1024
    for label, kw in (("options_off", {}), ("prefix_cache_chunk_unset", dict(prefix_cache=True)),
                      ("prefill_chunk_2048", dict(prefill_chunk=2048)), ("prefill_chunk_8192", dict(prefill_chunk=8192))):
        eng = Engine(model, max_batch=n_stream + 1, max_seq=max_seq, kv_pool_tokens=pool, prefill_tokens=long_n + 1,
                     eos_ids=(-1,), **kw)
        sp = SamplingParams(max_new_tokens=600)
        streams = [eng.submit(prompt(128), sp) for _ in range(n_stream)]
        for _ in range(40):  # the streaming batch is running; decode graphs captured
            eng.step()
        quiet = []
        for _ in range(30):
            t0 = time.perf_counter()
            eng.step()
            quiet.append(time.perf_counter() - t0)
        for rep in range(2):  # the first long prompt captures the decode graphs of its batch and key bucket: not reported
            long = eng.submit(prompt(long_n), SamplingParams(max_new_tokens=4))
            gaps = []
            while not long.done.is_set():  # every step ends with a decode step of the streaming batch
                t0 = time.perf_counter()
                eng.step()
                gaps.append(time.perf_counter() - t0)
            assert long.error is None and long.cached_tokens == 0, (long.error, long.cached_tokens)
            assert all(not r.done.is_set() for r in streams), "the streams must outlive the long prompt"
        emit({"part": "inter_token_gap", "engine": label, "model": a.model, "streams": n_stream, "long_prompt": long_n,
              "decode_step_ms_before": round(statistics.median(quiet) * 1e3, 2),
              "largest_gap_ms": round(max(gaps) * 1e3, 1), "steps_while_admitted": len(gaps),
              "long_prompt_ttft_ms": round((long.t_first - long.t_submit) * 1e3, 1)})
        del eng, streams
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="kernel,engine")
    ap.add_argument("--chunk", type=int, default=2048)
    ap.add_argument("--p0", default="0,2048,8192,30720")
    ap.add_argument("--rounds", type=int, default=5, help="alternating timed windows per route / requests per TTFT case")
    ap.add_argument("--window-ms", type=float, default=200.0, help="target length of a timed window")
    ap.add_argument("--model", default="llama3.1-8b")
    ap.add_argument("--prefix", type=int, default=2048)
    ap.add_argument("--tail", type=int, default=128)
    ap.add_argument("--streams", type=int, default=8)
    ap.add_argument("--long-prompt", type=int, default=32768)
    ap.add_argument("--json-out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prefill_paged_bench needs a GPU")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lines = []

    def emit(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        lines.append(line)
        if a.json_out:
            with open(a.json_out, "w") as f:
                f.write("\n".join(lines) + "\n")

    with torch.no_grad():
        for part in a.part.split(","):
            {"kernel": kernel_part, "engine": engine_part}[part](a, dev, emit)
    from mxllm.utils.calibrate import calibrate

    emit({"part": "calibration", **calibrate(dev)})


if __name__ == "__main__":
    main()
