"""The one operand check of the MXFP4 decode GEMM launcher, without a GPU.

``mx::w4_takes`` (csrc/kernels/w4_args.h) decides for ``mx_w4a16_gemm`` (csrc/kernels/mxfp4_gemm.hip) and
for the ``w4_linear`` binding whether a launch is taken.  A stand-alone driver (tests/native/test_w4_args.cpp)
is built with g++ -- plain, and under AddressSanitizer + UBSan -- and fed launch descriptions: every rule
on both sides of its boundary with the answer written down here, and shapes whose M * ldx and N * K leave
32 bits (the offsets the kernel forms come back as 64-bit numbers).
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "test_w4_args.cpp")

P = 0x10000  # a non-null, 16-B aligned address
I32 = 2 ** 31 - 1

BASE = dict(x=P, ldx=512, codes=2 * P, scales=3 * P, y=4 * P, ldy=16, M=4, N=16, K=512)


def _k(K, **kw):
    return dict(BASE, K=K, ldx=K, **kw)


# (description, taken, rule)
CASES = [(BASE, True, "base")]
CASES += [(dict(BASE, **{p: 0}), False, f"{p} is dereferenced") for p in ("x", "codes", "scales", "y")]
CASES += [(dict(BASE, M=1), True, "1 <= M"), (dict(BASE, M=0), False, "1 <= M"), (dict(BASE, M=-1), False, "1 <= M"),
          (dict(BASE, M=32), True, "M <= 32"), (dict(BASE, M=33), False, "M <= 32"),
          (dict(BASE, M=2 ** 32 + 4), False, "M <= 32 (64-bit: 2^32 + 4 would wrap to 4)")]
CASES += [(dict(BASE, N=32, ldy=32), True, "N % 16"), (dict(BASE, N=24, ldy=24), False, "N % 16"),
          (dict(BASE, N=0), False, "N >= 16"), (dict(BASE, N=-16), False, "N >= 16"),
          (dict(BASE, N=2 ** 31 - 16, ldy=2 ** 31 - 16), True, "N fits an int"),
          (dict(BASE, N=2 ** 31, ldy=2 ** 31), False, "N fits an int"),
          (dict(BASE, N=2 ** 32 + 16, ldy=2 ** 32 + 16), False, "N fits an int (2^32 + 16 would wrap to 16)")]
CASES += [(_k(1024), True, "K % 512"), (_k(1536), True, "K % 512"), (_k(3584), True, "K % 512 (70B down, TP-8)"),
          (_k(768), False, "K % 512"), (_k(256), False, "K % 512"), (_k(128), False, "K % 512"), (_k(0), False, "K > 0"),
          (_k(-512), False, "K > 0"), (_k(2 ** 31 - 512), True, "K fits an int"), (_k(2 ** 31), False, "K fits an int"),
          (_k(2 ** 32 + 512), False, "K fits an int (2^32 + 512 would wrap to 512)")]
CASES += [(dict(BASE, ldx=520), True, "ldx % 8"), (dict(BASE, ldx=516), False, "ldx % 8"),
          (dict(BASE, ldx=504), False, "ldx >= K"), (dict(BASE, ldy=24), True, "ldy % 8"),
          (dict(BASE, ldy=20), False, "ldy % 8"), (dict(BASE, ldy=8), False, "ldy >= N")]
CASES += [(dict(BASE, x=P + 16), True, "x 16-B aligned"), (dict(BASE, x=P + 8), False, "x 16-B aligned"),
          (dict(BASE, y=4 * P + 16), True, "y 16-B aligned"), (dict(BASE, y=4 * P + 8), False, "y 16-B aligned"),
          (dict(BASE, codes=2 * P + 16), True, "codes 16-B aligned"),
          (dict(BASE, codes=2 * P + 8), False, "codes 16-B aligned"),
          (dict(BASE, scales=3 * P + 4), True, "scales 4-B aligned"),
          (dict(BASE, scales=3 * P + 2), False, "scales 4-B aligned")]
# 64-bit products: 32 rows of a 2^31-element stride; 2^20 channels of K = 8192 (N * K = 2^33)
BIG = [(dict(BASE, M=32, ldx=2 ** 31), "M * ldx = 2^36"),
       (dict(BASE, N=2 ** 20, ldy=2 ** 20, K=8192, ldx=8192), "N * K = 2^33"),
       (dict(BASE, M=32, N=2 ** 31 - 16, ldy=2 ** 31 - 16, K=2 ** 31 - 512, ldx=2 ** 31 - 512),
        "the largest of everything")]
CASES += [(d, True, rule) for d, rule in BIG]

WAVES = {512: 4, 1024: 8, 1536: 4, 2048: 8, 3584: 4, 4096: 8, 4608: 4, 8192: 8, 28672: 8, 768: 0, 256: 0, 0: 0, -1024: 0}


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
    """[(w4_takes, waves, x_end, q_end, s_end, y_end)] per description."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], input="\n".join(_line(d) for d in descs) + "\n", capture_output=True, text=True,
                       timeout=300, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "ERROR: AddressSanitizer" not in out and "runtime error:" not in out, out[-4000:]
    got = [tuple(int(x) for x in ln.split()) for ln in r.stdout.splitlines()]
    assert len(got) == len(descs) and all(len(g) == 6 for g in got)
    return got


@pytest.fixture(scope="module", params=["plain", "asan_ubsan"])
def driver(request, tmp_path_factory):
    flags = [] if request.param == "plain" else ["-fsanitize=address,undefined"]
    return _build(tmp_path_factory.mktemp("w4args"), flags, "w4args_" + request.param)


def test_rules_on_both_sides_of_every_boundary(driver):
    got = _run(driver, [d for d, _, _ in CASES])
    bad = [(rule, _line(d), want) for (d, want, rule), g in zip(CASES, got) if bool(g[0]) != want]
    assert not bad, bad
    assert sum(want for _, want, _ in CASES) > 15 and sum(not want for _, want, _ in CASES) > 25


def test_waves_per_k(driver):
    got = _run(driver, [_k(K) for K in WAVES])
    assert [g[1] for g in got] == list(WAVES.values())
    assert all(bool(g[0]) == (w > 0) for g, w in zip(got, WAVES.values()))  # a K without a split is refused


def test_offsets_are_64_bit(driver):
    got = _run(driver, [d for d, _ in BIG])
    for (d, rule), g in zip(BIG, got):
        M, N, K = d["M"], d["N"], d["K"]
        want = (1, 8 if K % 1024 == 0 else 4, 2 * ((M - 1) * d["ldx"] + K), N * K // 2, N * K // 32,
                2 * ((M - 1) * d["ldy"] + N))
        assert g == want, rule
    assert got[0][2] > 2 ** 36 and got[1][3] == 2 ** 32 and got[2][3] > 2 ** 60
