"""The launch description and the one operand check of the verify attention, without a GPU.

``mx::vf_takes`` (csrc/kernels/verify_args.h) decides for ``mx_verify_attn`` (csrc/kernels/decode.hip)
whether a launch is taken; the launcher and the torch bindings ask it before anything is allocated or
enqueued.  A stand-alone driver (tests/native/test_verify_args.cpp) is built with g++ -- plain, and under
AddressSanitizer + UBSan: the products of the 32-bit overflow rules must not overflow themselves -- and fed
launch descriptions; nothing is preloaded.  Every rule on both sides of its boundary, the answer written
down here (each case names its rule).
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "test_verify_args.cpp")

P = 0x10000  # a non-null address
I32 = 2 ** 31 - 1

# a paged bf16 launch: 4 sequences x 4 rows, 32 q-heads over 8 KV heads (Llama-3.1-8B)
BASE = dict(q=P, k=2 * P, v=3 * P, lens=4 * P, nq=5 * P, slots=6 * P, bt=7 * P, ml=8 * P, po=9 * P, out=10 * P, q_bf16=1,
            out_bf16=1, kv_bf16=1, kv_u8=0, B=4, n=4, Hq=32, Hkv=8, D=128, rows=64, max_seq=256, maxb=32, nsplit=4)
KV8 = dict(BASE, kv_bf16=0, kv_u8=1, ks=11 * P, vs=12 * P)
FLAT = dict(BASE, bt=0, maxb=0, max_seq=8192)  # contiguous caches [slots, Hkv, max_seq, D]


def _with(base=BASE, **kw):
    return dict(base, **kw)


# (description, taken, rule)
CASES = [(BASE, True, "base"), (KV8, True, "base, kv8"), (FLAT, True, "base, contiguous caches")]
CASES += [(_with(**{k: 0}), False, f"null {k}") for k in ("q", "k", "v", "lens", "nq", "ml", "po", "out")]
CASES += [(_with(slots=0), True, "slots may be absent (slot = sequence)")]
CASES += [(_with(**{k: 0}), False, f"dtype: {k}") for k in ("q_bf16", "out_bf16")]
CASES += [(_with(kv_bf16=0), False, "pools: bf16 or u8"), (_with(kv_u8=1), False, "pools: not both"),
          (_with(ks=P), False, "bf16 pools take no scale pools"), (_with(vs=P), False, "bf16 pools take no scale pools"),
          (_with(KV8, ks=0), False, "u8 pools need the K scale pool"), (_with(KV8, vs=0), False, "u8 pools need the V scale pool")]
CASES += [(_with(D=64), False, "head_dim 128"), (_with(D=256), False, "head_dim 128")]
CASES += [(_with(Hq=31), False, "Hq % Hkv"), (_with(Hq=24), True, "Hq % Hkv"), (_with(Hkv=0), False, "Hkv > 0"),
          (_with(Hq=0), False, "Hq > 0"), (_with(Hq=-32, Hkv=-8), False, "Hq > 0")]
CASES += [(_with(n=0), False, "n >= 1"), (_with(n=-1), False, "n >= 1"), (_with(n=1), True, "n >= 1"),
          (_with(n=8), True, "n * group <= 32 (8 x 4)"), (_with(n=9), False, "n * group <= 32 (9 x 4)"),
          (_with(Hq=64, n=4), True, "n * group <= 32 (4 x 8)"), (_with(Hq=64, n=5), False, "n * group <= 32 (5 x 8)"),
          (_with(Hq=8, n=32), True, "n * group <= 32 (32 x 1)"), (_with(Hq=8, n=33), False, "n * group <= 32 (33 x 1)"),
          (_with(Hq=256, n=1), True, "n * group <= 32 (1 x 32)"), (_with(Hq=264, n=1), False, "n * group <= 32 (1 x 33)"),
          (_with(Hq=16, Hkv=1, n=2), True, "n * group <= 32 (2 x 16)"), (_with(Hq=16, Hkv=1, n=3), False, "n * group <= 32 (3 x 16)")]
CASES += [(_with(**{k: 0}), False, f"{k} > 0") for k in ("B", "nsplit", "rows", "max_seq")]
CASES += [(_with(B=-1), False, "B > 0"), (_with(nsplit=-4), False, "nsplit > 0"), (_with(B=1, nsplit=1), True, "B, nsplit > 0")]
CASES += [(_with(max_seq=512), True, "paged: block % 256"), (_with(max_seq=128), False, "paged: block % 256"),
          (_with(max_seq=320), False, "paged: block % 256"), (_with(maxb=0), False, "paged: maxb > 0"),
          (_with(FLAT, max_seq=300), True, "contiguous caches: any max_seq"), (_with(FLAT, max_seq=1), True, "contiguous caches: any max_seq")]
CASES += [(_with(Hkv=65535, Hq=65535), True, "grid y"), (_with(Hkv=65536, Hq=65536), False, "grid y"),
          (_with(B=65535, Hq=8), True, "grid z"), (_with(B=65536, Hq=8), False, "grid z")]
# 32-bit values: each product is formed as a division
CASES += [(_with(nsplit=2 ** 23 - 1), True, "nsplit * 256 in 31 bits"), (_with(nsplit=2 ** 23), False, "nsplit * 256 in 31 bits"),
          (_with(nsplit=2 ** 56), False, "nsplit * 256 in 64 bits"),
          (_with(maxb=2 ** 23 - 1), True, "maxb * block in 31 bits"), (_with(maxb=2 ** 23), False, "maxb * block in 31 bits"),
          (_with(maxb=2 ** 56), False, "maxb * block in 64 bits"),
          (_with(max_seq=2 ** 62, maxb=1), False, "maxb * block in 64 bits (2^62 is a multiple of 256)"),
          (_with(FLAT, max_seq=I32), True, "max_seq in 31 bits"), (_with(FLAT, max_seq=2 ** 31), False, "max_seq in 31 bits"),
          (_with(B=65535, n=32, Hq=1024, Hkv=1024), True, "B * n * Hq in 31 bits (2^31 - 2^15)"),
          (_with(B=65535, n=32, Hq=1025, Hkv=1025), False, "B * n * Hq in 31 bits"),
          (_with(B=65535, n=2 ** 40, Hq=1, Hkv=1), False, "n * group <= 32 before any product"),
          (_with(B=65535, n=1, Hq=2 ** 62, Hkv=2 ** 62), False, "grid y before any product")]


def _line(d):
    return " ".join(f"{k}={v}" for k, v in d.items())


def _build(tmp, flags, name):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp / name)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", f"-I{os.path.join(ROOT, 'csrc')}",
                        *flags, SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _run(exe, descs):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], input="\n".join(_line(d) for d in descs) + "\n", capture_output=True, text=True,
                       timeout=300, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "ERROR: AddressSanitizer" not in out and "runtime error:" not in out, out[-4000:]
    got = [ln.strip() == "1" for ln in r.stdout.splitlines()]
    assert len(got) == len(descs)
    return got


@pytest.fixture(scope="module", params=["plain", "asan_ubsan"])
def driver(request, tmp_path_factory):
    flags = [] if request.param == "plain" else ["-fsanitize=address,undefined"]
    return _build(tmp_path_factory.mktemp("vfargs"), flags, "vfargs_" + request.param)


def test_rules_on_both_sides_of_every_boundary(driver):
    got = _run(driver, [d for d, _, _ in CASES])
    bad = [(rule, _line(d), want) for (d, want, rule), g in zip(CASES, got) if g != want]
    assert not bad, bad
    share = sum(got) / len(got)
    assert 0.15 < share < 0.85, share  # the table sits on both sides
