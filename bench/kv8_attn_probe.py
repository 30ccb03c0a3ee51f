"""Decode attention over a bf16 cache (decode_attn) against the fp8 kv8 cache (decode_attn_kv8).

For every shape (q-heads / KV heads, batch, context) both kernels run on caches of the same logical
contents size; each timed window walks ``layers`` separate caches (as a decode step does), enough of
them that the working set exceeds the Infinity Cache, and the two kernels alternate round by round.
Time: device events around a window, per call.  Bytes: what the algorithm has to read, K and V rows of
256 B (bf16) or 128 B + one f32 scale (kv8); bytes/s = bytes / time.  One JSON line per shape.

  python bench/kv8_attn_probe.py [--heads 64:8,32:8] [--batches 1,8,64] [--ctx 1024,8192,32768]
"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

D = 128
HBM_PEAK_TB_S = 8.0  # MI355X HBM3E peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--heads", default="64:8,32:8", help="Hq:Hkv pairs")
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--ctx", default="1024,8192,32768")
    ap.add_argument("--rounds", type=int, default=5, help="alternating timed windows per kernel")
    ap.add_argument("--window-ms", type=float, default=40.0, help="target length of a timed window")
    ap.add_argument("--min-bytes", type=float, default=2 ** 31, help="bf16 working set walked per window, at least")
    ap.add_argument("--max-bytes", type=float, default=40e9, help="skip shapes whose one-layer bf16 cache is larger")
    ap.add_argument("--json-out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kv8_attn_probe needs a GPU")
    from mxllm.ops import native

    ops, dev = native(), torch.device("cuda", 0)
    scale = 1.0 / math.sqrt(D)
    lines = []
    for hq, hkv in (tuple(int(v) for v in p.split(":")) for p in a.heads.split(",")):
        for B in (int(b) for b in a.batches.split(",")):
            for ctx in (int(c) for c in a.ctx.split(",")):
                rows = B * hkv * ctx
                b16, b8 = rows * 2 * D * 2, rows * 2 * (D + 4)
                if b16 > a.max_bytes:
                    continue
                layers = max(1, min(512, math.ceil(a.min_bytes / b16)))
                q = torch.randn(B, hq, D, device=dev).bfloat16()
                lens = torch.full((B,), ctx, dtype=torch.int32, device=dev)
                c16 = [(torch.randn(B, hkv, ctx, D, device=dev, dtype=torch.bfloat16),
                        torch.randn(B, hkv, ctx, D, device=dev, dtype=torch.bfloat16)) for _ in range(layers)]
                c8 = []
                for k, v in c16:
                    kq, ks = ops.kv8_quant_rows(k.view(-1, D))
                    vq, vs = ops.kv8_quant_rows(v.view(-1, D))
                    c8.append((kq.view(B, hkv, ctx, D), ks.view(B, hkv, ctx), vq.view(B, hkv, ctx, D), vs.view(B, hkv, ctx)))

                def run16():
                    for k, v in c16:
                        ops.decode_attn(q, k, v, lens, None, ctx, scale, 0, None, None)

                def run8():
                    for kq, ks, vq, vs in c8:
                        ops.decode_attn_kv8(q, kq, ks, vq, vs, lens, None, ctx, scale, 0, None)

                def window(fn, n):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(n):
                        fn()
                    e1.record()
                    e1.synchronize()
                    return e0.elapsed_time(e1) * 1e-3 / (n * layers)  # seconds per call

                t = {}
                for name, fn in (("bf16", run16), ("kv8", run8)):  # warm up, size the window
                    fn()
                    torch.cuda.synchronize()
                    one = window(fn, 2) * layers
                    t[name] = (fn, max(2, int(a.window_ms * 1e-3 / max(one, 1e-7))), [])
                for _ in range(a.rounds):
                    for name in ("bf16", "kv8"):
                        fn, n, acc = t[name]
                        acc.append(window(fn, n))
                res = {"Hq": hq, "Hkv": hkv, "batch": B, "ctx": ctx, "layers_walked": layers}
                for name, nbytes in (("bf16", b16), ("kv8", b8)):
                    ts = sorted(t[name][2])
                    med = ts[len(ts) // 2]
                    res[name] = {"us": round(med * 1e6, 2), "us_min": round(ts[0] * 1e6, 2), "us_max": round(ts[-1] * 1e6, 2),
                                 "bytes": nbytes, "tb_s": round(nbytes / med / 1e12, 3),
                                 "hbm_peak_share": round(nbytes / med / 1e12 / HBM_PEAK_TB_S, 3)}
                res["speedup_kv8"] = round(res["bf16"]["us"] / res["kv8"]["us"], 3)
                line = json.dumps(res)
                print(line, flush=True)
                lines.append(line)
                del c16, c8
                torch.cuda.empty_cache()
    if a.json_out:
        with open(a.json_out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
