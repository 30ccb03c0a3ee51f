#!/usr/bin/env python3
"""MXFP4-weight decode GEMM (csrc/kernels/mxfp4_gemm.hip w4a16_gemm_kernel) at the Llama-3.1-70B / 8B
projection shapes: achieved weight-streaming bandwidth per channel-group count (MXLLM_W4_NC, read per
call) beside ``w8_linear`` and the bf16 skinny GEMM on the same shapes; variants interleaved in one
process (median of per-call events, median over rounds).  Every variant cycles through enough copies of
its weight to exceed the 256 MB Infinity Cache, so each call streams from HBM as a decode step does.

``--crossover``: the pass route of ``w4_linear`` (one weight pass per 32 rows) against dequantise + bf16
GEMM at M = 32 .. 256: where MXLLM_W4_STREAM_M's default comes from.

Usage: python bench/w4_probe.py [--ms 1,4,8,16,32] [--nc 0,1,2,4] [--rounds 5] [--crossover]
"""
from __future__ import annotations

import argparse
import itertools
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mxllm.ops import native  # noqa: E402
from mxllm.serve.quant import quantize_e4m3, quantize_mxfp4  # noqa: E402

SHAPES = {"70b qkv": (8192, 10240), "70b o": (8192, 8192), "70b gu": (8192, 57344), "70b down": (28672, 8192),
          "8b qkv": (4096, 6144), "8b gu": (4096, 28672), "8b down": (14336, 4096)}
RING_BYTES = 512 << 20


def ring(tensors):
    """An endless cycle over copies of ``tensors`` (a tuple), at least RING_BYTES of them together."""
    nbytes = sum(t.numel() * t.element_size() for t in tensors)
    n = max(2, -(-RING_BYTES // nbytes))
    return itertools.cycle([tensors] + [tuple(t.clone() for t in tensors) for _ in range(n - 1)])


def time_us(fn, calls):
    for _ in range(3):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for s, e in ev:
        s.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    return 1e3 * statistics.median(s.elapsed_time(e) for s, e in ev)


def close(y, ref, what):
    assert (y.float() - ref).abs().max().item() <= 1e-2 * ref.abs().max().item() + 1e-3, what


def probe(a, ops, dev):
    out = []
    big = 1 << 30
    for name, (K, N) in SHAPES.items():
        w = (torch.randn(N, K, device=dev) * 0.02).to(torch.bfloat16)
        codes, scales = quantize_mxfp4(w)
        w4, w8, w16 = ring((codes, scales)), ring(quantize_e4m3(w)), ring((w,))
        wd = ops.w4_dequant(codes, scales)  # exactly the decoded weights (tests/test_mxfp4_gpu.py)
        del w
        for M in map(int, a.ms.split(",")):
            x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
            ref = (x @ wd.t()).float()
            res = {f"nc{nc}": [] for nc in a.nc.split(",")}
            res.update(w8=[], bf16=[])
            for _ in range(a.rounds):
                for key in res:
                    if key.startswith("nc"):
                        os.environ["MXLLM_W4_NC"] = key[2:] if key != "nc0" else ""
                        close(ops.w4_linear(x, codes, scales, big), ref, (name, M, key))
                        res[key].append(time_us(lambda: ops.w4_linear(x, *next(w4), big), a.calls))
                    elif key == "w8":
                        res[key].append(time_us(lambda: ops.w8_linear(x, *next(w8)), a.calls))
                    else:
                        res[key].append(time_us(lambda: ops.skinny_linear(x, *next(w16)), a.calls))
            os.environ.pop("MXLLM_W4_NC", None)
            rec = {"case": f"{name} M{M} N{N} K{K}", "w4_mb": round(N * K * (0.5 + 1 / 32) / 1e6, 1)}
            for key, v in res.items():
                us = statistics.median(v)
                nbytes = N * K * (0.5 + 1 / 32 if key.startswith("nc") else 1 if key == "w8" else 2)
                rec[key] = {"us": round(us, 1), "tbps": round(nbytes / (us * 1e-6) / 1e12, 2)}
            print(json.dumps(rec), flush=True)
            out.append(rec)
        del w4, w8, w16, wd, codes, scales
        torch.cuda.empty_cache()
    return out


def crossover(a, ops, dev):
    out = []
    big = 1 << 30
    for name, (K, N) in SHAPES.items():
        codes, scales = quantize_mxfp4((torch.randn(N, K, device=dev) * 0.02).to(torch.bfloat16))
        w4 = ring((codes, scales))
        wd = ops.w4_dequant(codes, scales)
        for M in (32, 64, 128, 256):
            x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
            ref = (x @ wd.t()).float()
            close(ops.w4_linear(x, codes, scales, big), ref, (name, M, "passes"))
            close(ops.w4_linear(x, codes, scales, 0) if M > 32 else x @ ops.w4_dequant(codes, scales).t(), ref,
                  (name, M, "dequant + gemm"))
            res = {"passes": [], "dequant_gemm": []}
            for _ in range(a.rounds):
                res["passes"].append(time_us(lambda: ops.w4_linear(x, *next(w4), big), a.calls))
                res["dequant_gemm"].append(time_us(lambda: x @ ops.w4_dequant(*next(w4)).t(), a.calls))
            rec = {"case": f"{name} M{M} N{N} K{K}"}
            rec.update({k: round(statistics.median(v), 1) for k, v in res.items()})
            print(json.dumps(rec), flush=True)
            out.append(rec)
        del w4, wd, codes, scales
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ms", default="1,4,8,16,32")
    ap.add_argument("--nc", default="0,1,2,4", help="0 = the default rule")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--crossover", action="store_true")
    ap.add_argument("--json-out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = (crossover if a.crossover else probe)(a, native(), dev)
    if a.json_out:
        with open(a.json_out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
