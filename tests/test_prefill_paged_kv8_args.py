"""``mx::pp8_takes`` (csrc/kernels/prefill_paged_kv8_args.h) without a GPU: a stand-alone driver
(tests/native/test_prefill_paged_kv8_args.cpp) built with g++ plain and under AddressSanitizer + UBSan (nothing is
preloaded).  Each rule pp8_takes adds, and rules it inherits from ``mx::pp_takes`` through the four-pool description,
the 32-bit overflow rules among them (their products must not overflow themselves).
"""
import os
import shutil
import subprocess

import pytest

from tests import test_prefill_paged_args as A

P = A.P
SRC = os.path.join(A.ROOT, "tests", "native", "test_prefill_paged_kv8_args.cpp")
SHAPE = (8, 2, 256, 128)


def line(shape=SHAPE, seg=A.BASE["seg"], **kw):
    """One launch for the driver: BASE of test_prefill_paged_args over four pools of ``shape``; ``kc`` .. ``vs``
    replace a pool by (address, dtype_ok, contiguous, shape)."""
    d = dict(q=P, o=4 * P, bt=5 * P, segs=6 * P, work=7 * P, q_bf16=1, o_bf16=1, T=400, Hq=8, D=128, slots=3, maxb=3,
             ldo=1024, nwork=-1)
    pools = dict(kc=(2 * P, 1, 1, shape), ks=(8 * P, 1, 1, shape[:3]), vc=(3 * P, 1, 1, shape), vs=(9 * P, 1, 1, shape[:3]))
    pools.update({k: kw.pop(k) for k in list(kw) if k in pools})
    d.update(kw)
    out = [*d.values(), len(seg), *(x for s in seg for x in s)]
    for a, ok, cont, shp in pools.values():
        out += [a, ok, cont, len(shp), *shp]
    return " ".join(str(x) for x in out)


def pool(name, addr=P, ok=1, cont=1):
    return {name: (addr, ok, cont, SHAPE if name in ("kc", "vc") else SHAPE[:3])}


# (launch, taken, rule)
CASES = [(line(), True, "base"), (line(shape=(8, 2, 512, 128)), True, "blk 512")]
CASES += [(line(**pool(n, **kw)), False, f"{n}: {kw}") for n in ("kc", "ks", "vc", "vs") for kw in (dict(addr=0), dict(ok=0), dict(cont=0))]
CASES += [(line(ks=(P, 1, 1, (8, 2, 255))), False, "scale shape: rows"), (line(vs=(P, 1, 1, (8, 1, 256))), False, "scale shape: heads"),
          (line(ks=(P, 1, 1, (8, 2, 256, 1))), False, "scale pools have 3 dimensions"),
          (line(kc=(P, 1, 1, (8, 2, 256))), False, "code pools have 4 dimensions"),
          (line(vc=(P, 1, 1, (7, 2, 256, 128)), vs=(P, 1, 1, (7, 2, 256))), False, "K and V pools of one shape"),
          (line(shape=(8, 2, 256, 64)), False, "the pools' last dimension is q's")]
# inherited from pp_takes, reached through the code pools' shape
CASES += [(line(shape=(8, 2, 128, 128), maxb=6), False, "blk % 256"), (line(shape=(8, 3, 256, 128)), False, "Hq % Hkv"),
          (line(q_bf16=0), False, "dtype of q"), (line(seg=A._seg(1, row0=7)), False, "disjoint rows"),
          (line(shape=(8, 2, 2 ** 22, 128), maxb=1), True, "blk * 256 bytes in 31 bits"),
          (line(shape=(8, 2, 2 ** 23, 128), maxb=1), False, "blk * 256 bytes in 31 bits"),
          (line(shape=(8, 2, 2 ** 40, 128), maxb=1), False, "blk * 256 in 64 bits"),
          (line(maxb=2 ** 23 - 1), True, "maxb * blk in 31 bits"), (line(maxb=2 ** 56), False, "maxb * blk in 64 bits"),
          (line(seg=[(0, 1, 0, 2 ** 31 - 1)], maxb=2 ** 23 - 1), False, "p0 + n in 64 bits")]


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined"]], ids=["plain", "asan_ubsan"])
def test_rules_on_both_sides_of_every_boundary(tmp_path, flags):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "pp8args")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", f"-I{os.path.join(A.ROOT, 'csrc')}",
                        *flags, SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], input="\n".join(c for c, _, _ in CASES) + "\n", capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "runtime error:" not in r.stderr, (r.stdout + r.stderr)[-4000:]
    got = [x == "1" for x in r.stdout.split()]
    assert len(got) == len(CASES)
    bad = [(rule, c, want) for (c, want, rule), g in zip(CASES, got) if g != want]
    assert not bad, bad
