"""The one operand check of the gemm8 launchers, without a GPU.

``mx::g8_takes`` (csrc/kernels/gemm8_args.h) decides for all five launchers of
csrc/kernels/gemm8.hip whether a launch is taken.  A stand-alone driver
(tests/native/test_gemm8_args.cpp) is built with g++ -- plain, and under
AddressSanitizer + UBSan: the span arithmetic must not overflow -- and fed launch descriptions:

(a) every rule of every entry point on both sides of its boundary, with the answer written down from
    the launchers' code as it was before the check was unified (each case names its rule);
(b) ``mxllm.ops.gemm.g8_takes``, the Python mirror the dispatch predicates ask, gives the driver's
    answer on every line of (a) and of a product grid (unaligned bases, row strides that are no
    multiple of 8 or shorter than the row, row-split against column-split tails, ...).
"""
import itertools
import os
import shutil
import subprocess

import pytest

from mxllm.ops import gemm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "test_gemm8_args.cpp")

P = 0x10000  # an aligned, non-null address; P + 8: aligned to 8 B only

# accepted base descriptions per entry point (TN operands, one tile, one or two K-tiles)
PLAIN = dict(entry="plain", a=P, lda=64, a_kc=1, b=2 * P, ldb=64, b_kc=1, c=3 * P, ldc=256, M=256, N=256, K=64)
TT = dict(PLAIN, a_kc=0, b_kc=0, lda=256, ldb=256)  # weight-gradient form: both operands [K][.]
SQ = dict(PLAIN, entry="sq", sq=4 * P)
ROPE = dict(entry="epi", epi="rope", a=P, lda=64, a_kc=1, b=2 * P, ldb=64, b_kc=1, M=256, N=512, K=64,
            q=5 * P, k=6 * P, v=7 * P, cosb=8 * P, sinb=9 * P, S=256, Hq=2, Hkv=1)
SWIGLU = dict(PLAIN, entry="epi", epi="swiglu", m=5 * P, ldm=128)
BWD = dict(entry="epi", epi="swiglu_bwd", a=P, lda=64, a_kc=1, b=2 * P, ldb=256, b_kc=0, c=3 * P, ldc=512,
           M=256, N=256, K=64, gu=5 * P, ldg=512)
TAIL = dict(PLAIN, entry="tail", N=512, ldc=512, K=128, lda=128, ldb=128, at=256, ws=4 * P, ph=4)
ROPE_TAIL = dict(ROPE, entry="rope_tail", K=128, lda=128, ldb=128, at=256, ws=4 * P)
G70B = dict(SWIGLU, M=4096, N=57344, K=8192, lda=8192, ldb=8192, ldc=57344, ldm=28672)

# (description, taken, rule).  2^30 elements of bf16 = 2^31 bytes.
CASES = [
    (PLAIN, True, "base"), (TT, True, "base"), (SQ, True, "base"), (ROPE, True, "base"), (SWIGLU, True, "base"),
    (BWD, True, "base"), (TAIL, True, "base"), (ROPE_TAIL, True, "base"),
    # whole 256 x 256 tiles, every entry point
    (dict(PLAIN, M=512, N=768, ldc=768), True, "M, N multiples of 256"),
    (dict(PLAIN, M=255), False, "M multiple of 256"),
    (dict(PLAIN, M=0), False, "M > 0"),
    (dict(PLAIN, N=384, ldc=384), False, "N multiple of 256"),
    (dict(SQ, M=384), False, "sq: whole tiles"),
    (dict(BWD, N=384, ldb=384, ldc=768, ldg=768), False, "swiglu_bwd: N multiple of 256"),
    (dict(TAIL, M=384), False, "tail: the plain part's launcher refuses M % 256"),
    # K-tiles: K % 64 when an operand is k-contiguous, any K otherwise
    (dict(PLAIN, K=32), False, "K % 64 (k-contiguous)"),
    (dict(PLAIN, K=128, lda=128, ldb=128), True, "K % 64 (k-contiguous)"),
    (dict(TT, K=1), True, "any K (mn-contiguous)"),
    (dict(TT, K=1000), True, "any K (mn-contiguous)"),
    (dict(TT, b_kc=1, ldb=96, K=96), False, "K % 64 when only B is k-contiguous"),
    (dict(TT, K=0), False, "K > 0"),
    (dict(BWD, K=96, lda=96), False, "swiglu_bwd: K % 64"),
    # row strides: 16-B units, at least the stored row
    (dict(PLAIN, lda=72), True, "lda % 8"), (dict(PLAIN, lda=68), False, "lda % 8"),
    (dict(PLAIN, ldb=72), True, "ldb % 8"), (dict(PLAIN, ldb=68), False, "ldb % 8"),
    (dict(PLAIN, lda=56), False, "lda >= K (k-contiguous)"),
    (dict(PLAIN, ldb=56), False, "ldb >= K (k-contiguous)"),
    (dict(TT, lda=248), False, "lda >= M (m-contiguous)"),
    (dict(TT, ldb=248), False, "ldb >= N (n-contiguous)"),
    (dict(BWD, ldb=248), False, "swiglu_bwd: ldb >= N"),
    # 16-B aligned bases
    (dict(PLAIN, a=P + 16), True, "A 16-B aligned"), (dict(PLAIN, a=P + 8), False, "A 16-B aligned"),
    (dict(PLAIN, b=2 * P + 8), False, "B 16-B aligned"), (dict(PLAIN, c=3 * P + 8), False, "C 16-B aligned"),
    (dict(PLAIN, c=0), True, "mx_gemm8 does not ask for a non-null C"),
    # C rows: bf16 stored 16 B at a time (ldc % 8), fp32 ldc % 4; at least N wide
    (dict(PLAIN, ldc=264), True, "bf16 ldc % 8"), (dict(PLAIN, ldc=260), False, "bf16 ldc % 8"),
    (dict(PLAIN, out_f32=1, ldc=260), True, "fp32 ldc % 4"), (dict(PLAIN, out_f32=1, ldc=258), False, "fp32 ldc % 4"),
    (dict(PLAIN, ldc=248), False, "ldc >= N"),
    (dict(SQ, ldc=260), False, "sq: bf16 output, ldc % 8"),
    (dict(TAIL, ldc=516), False, "tail: ldc % 8"), (dict(TAIL, ldc=504), False, "tail: ldc >= N"),
    # beta 0 or 1
    (dict(PLAIN, beta=1.0), True, "beta 0 or 1"), (dict(PLAIN, beta=0.5), False, "beta 0 or 1"),
    # spans under 2^31 bytes.  k-contiguous operand of the plain kernel: 256 rows
    (dict(PLAIN, lda=2 ** 22 - 8), True, "A span 256 * lda * 2 < 2^31"),
    (dict(PLAIN, lda=2 ** 22), False, "A span 256 * lda * 2 < 2^31"),
    (dict(PLAIN, ldb=2 ** 22 - 8), True, "B span 256 * ldb * 2 < 2^31 (plain kernel)"),
    (dict(PLAIN, ldb=2 ** 22), False, "B span 256 * ldb * 2 < 2^31 (plain kernel)"),
    (dict(PLAIN, N=512, ldc=512, ldb=2 ** 21), True, "plain kernel: 256 rows of B, not all N"),
    (dict(PLAIN, lda=2 ** 62), False, "span arithmetic does not overflow"),
    (dict(TT, ldb=2 ** 62 + 8), False, "span arithmetic does not overflow"),
    # mn-contiguous operand: the K-tile-padded rows
    (dict(TT, K=1000, lda=2 ** 20 - 8), True, "A span kpad * lda * 2 < 2^31"),
    (dict(TT, K=1000, lda=2 ** 20), False, "A span kpad * lda * 2 < 2^31"),
    (dict(TT, K=961, ldb=2 ** 20), False, "B span kpad * ldb * 2 < 2^31 (K padded to 1024)"),
    (dict(TT, K=960, ldb=2 ** 20), True, "B span kpad * ldb * 2 < 2^31 (K = 960 = kpad)"),
    (dict(SQ, K=128, lda=2 ** 22, ldb=128), False, "sq: the plain kernel's spans"),
    (dict(TAIL, ldb=2 ** 22), False, "tail: the plain kernel's spans"),
    (dict(TAIL, ldb=2 ** 22 - 8), True, "tail: the plain kernel's spans"),
    # fused TN epilogues: weight rows are gathered from the whole matrix, N * ldb
    (dict(SWIGLU, N=512, ldc=512, ldm=256, ldb=2 ** 21 - 8), True, "swiglu: B span N * ldb * 2 < 2^31"),
    (dict(SWIGLU, N=512, ldc=512, ldm=256, ldb=2 ** 21), False, "swiglu: B span N * ldb * 2 < 2^31"),
    (dict(ROPE, ldb=2 ** 21), False, "rope: B span N * ldb * 2 < 2^31"),
    (dict(ROPE, ldb=2 ** 21 - 8), True, "rope: B span N * ldb * 2 < 2^31"),
    (dict(ROPE_TAIL, ldb=2 ** 21), False, "rope_tail: B span N * ldb * 2 < 2^31"),
    (dict(ROPE, lda=2 ** 22), False, "rope: A span 256 * lda * 2 < 2^31"),
    (G70B, True, "70B gate-up 57,344 x 8,192 is fused"),
    (dict(G70B, N=106496, K=16384, lda=16384, ldb=16384, ldc=106496, ldm=53248), False,
     "405B-class gate-up 106,496 x 16,384 is over the span"),
    # SWIGLU_BWD: W_down [K][N] n-contiguous, K * ldb
    (dict(BWD, ldb=2 ** 24 - 8), True, "swiglu_bwd: B span K * ldb * 2 < 2^31"),
    (dict(BWD, ldb=2 ** 24), False, "swiglu_bwd: B span K * ldb * 2 < 2^31"),
    # sq partials
    (dict(SQ, sq=0), False, "sq: buffer required"),
    (dict(TAIL, sq=5 * P), True, "tail sq: 4-phase schedule"),
    (dict(TAIL, sq=5 * P, ph=8), False, "tail sq: 4-phase schedule"),
    (dict(TAIL, sq=5 * P, ph=5), False, "tail sq: 4-phase schedule"),
    (dict(TAIL, ph=8), True, "tail without sq: any schedule"),
    (dict(TAIL, sq=5 * P, K=64, lda=64, ldb=64), False, "tail sq at K 64 (K < 128)"),
    # tail launches: K >= 128, `at` and the rest whole tiles, 16-B workspace
    (dict(TAIL, K=64, lda=64, ldb=64), False, "tail: K >= 128"),
    (dict(TAIL, a_kc=0, b_kc=0, lda=256, ldb=512, K=127), False, "tail: K >= 128 (mn-contiguous)"),
    (dict(TAIL, a_kc=0, b_kc=0, lda=256, ldb=512, K=130), True, "tail: any K >= 128 (mn-contiguous)"),
    (dict(TAIL, at=128), False, "tail: at % 256"), (dict(TAIL, at=0), False, "tail: at > 0"),
    (dict(TAIL, at=512), False, "tail: rest > 0"), (dict(TAIL, at=768), False, "tail: rest > 0"),
    (dict(TAIL, N=768, ldc=768, at=512), True, "tail: at, rest multiples of 256"),
    (dict(TAIL, ws=4 * P + 8), False, "tail: 16-B workspace"),
    (dict(TAIL, M=512, N=256, ldc=256, rows=1), True, "tail: row split of a 2 x 1 grid"),
    (dict(TAIL, M=512, N=256, ldc=256, rows=0), False, "tail: column split of a 2 x 1 grid has no rest"),
    (dict(TAIL, rows=1), False, "tail: row split of a 1 x 2 grid has no rest"),
    (dict(ROPE_TAIL, K=64, lda=64, ldb=64), False, "rope_tail: K >= 128"),
    (dict(ROPE_TAIL, at=128), False, "rope_tail: at % 256"), (dict(ROPE_TAIL, at=512), False, "rope_tail: at < N"),
    (dict(ROPE_TAIL, at=0), False, "rope_tail: at > 0"),
    (dict(ROPE_TAIL, ws=4 * P + 4), False, "rope_tail: 16-B workspace"),
    # RoPE epilogue
    (dict(ROPE, Hq=3), False, "rope: N = (Hq + 2 Hkv) * 128"),
    (dict(ROPE, S=128), False, "rope: S % 256"), (dict(ROPE, S=0), False, "rope: S > 0"),
    (dict(ROPE, M=768, S=512), False, "rope: M % S"), (dict(ROPE, M=768, S=256), True, "rope: M % S"),
    (dict(ROPE, q=0), False, "rope: q"), (dict(ROPE, v=7 * P + 8), False, "rope: v 16-B aligned"),
    (dict(ROPE, k=6 * P + 16), True, "rope: k 16-B aligned"),
    (dict(ROPE, cosb=0), False, "rope: tables"), (dict(ROPE, sinb=0), False, "rope: tables"),
    (dict(ROPE, c=3 * P + 2, ldc=3), True, "rope: C unused"),
    (dict(ROPE, cosb=8 * P + 4), True, "rope (epi): tables need 4-B alignment only"),
    (dict(ROPE_TAIL, cosb=8 * P + 4), False, "rope_tail: 16-B aligned tables"),
    (dict(ROPE_TAIL, sinb=9 * P + 8), False, "rope_tail: 16-B aligned tables"),
    # SwiGLU epilogue
    (dict(SWIGLU, c=0), False, "swiglu: gu required"), (dict(SWIGLU, m=0), False, "swiglu: m required"),
    (dict(SWIGLU, ldm=120), False, "swiglu: ldm >= F"), (dict(SWIGLU, ldm=132), False, "swiglu: ldm % 8"),
    (dict(SWIGLU, ldm=136), True, "swiglu: ldm % 8"), (dict(SWIGLU, m=5 * P + 8), False, "swiglu: m 16-B aligned"),
    (dict(SWIGLU, ldc=248), False, "swiglu: ldc >= 2F"),
    # SwiGLU backward epilogue
    (dict(BWD, ldc=504), False, "swiglu_bwd: ldc >= 2N"), (dict(BWD, ldc=516), False, "swiglu_bwd: ldc % 8"),
    (dict(BWD, ldg=504), False, "swiglu_bwd: ldg >= 2N"), (dict(BWD, ldg=516), False, "swiglu_bwd: ldg % 8"),
    (dict(BWD, ldg=520), True, "swiglu_bwd: ldg % 8"), (dict(BWD, gu=0), False, "swiglu_bwd: gu required"),
    (dict(BWD, gu=5 * P + 8), False, "swiglu_bwd: gu 16-B aligned"),
    (dict(BWD, c=0), False, "swiglu_bwd: dgu required"),
    (dict(BWD, m=6 * P, ldm=256), True, "swiglu_bwd: optional m"),
    (dict(BWD, m=6 * P, ldm=248), False, "swiglu_bwd: ldm >= N"),
    (dict(BWD, m=6 * P, ldm=260), False, "swiglu_bwd: ldm % 8"),
    (dict(BWD, m=6 * P + 8, ldm=256), False, "swiglu_bwd: m 16-B aligned"),
    # entry point <-> epilogue
    (dict(SWIGLU, epi="none"), False, "mx_gemm8_epi: a mode is required"),
    (dict(SWIGLU, epi="7"), False, "mx_gemm8_epi: unknown mode"),
]


def _grid():
    """Product grid for the differential: no expectations, just many ways to be off a rule."""
    out = []
    shapes = [(256, 256, 64), (512, 256, 128), (256, 512, 100), (255, 256, 64), (512, 512, 192)]
    for entry, (a_kc, b_kc), (M, N, K), dld, off, rows, at, f32 in itertools.product(
            ("plain", "sq", "tail"), itertools.product((0, 1), repeat=2), shapes, (0, 8, 4, -8), (0, 8), (0, 1),
            (128, 256), (0, 1)):
        out.append(dict(entry=entry, a=P + off, lda=(K if a_kc else M) + dld, a_kc=a_kc, b=2 * P,
                        ldb=(K if b_kc else N) + dld, b_kc=b_kc, c=3 * P + off, ldc=N + dld, out_f32=f32, M=M, N=N, K=K,
                        rows=rows, at=at, ws=4 * P + off, ph=4 + 4 * f32, sq=5 * P * rows))
    for entry, epi, (a_kc, b_kc), (M, N, K), dld, off, at in itertools.product(
            ("epi", "rope_tail"), ("none", "rope", "swiglu", "swiglu_bwd"), itertools.product((0, 1), repeat=2), shapes,
            (0, 8, 4, -8), (0, 8), (128, 256)):
        out.append(dict(entry=entry, epi=epi, a=P, lda=K + dld, a_kc=a_kc, b=2 * P + off, ldb=(K if b_kc else N) + dld,
                        b_kc=b_kc, c=3 * P, ldc=2 * N, M=M, N=N, K=K, at=at, ws=4 * P, q=5 * P, k=6 * P + off, v=7 * P,
                        cosb=8 * P + off, sinb=9 * P, S=256, Hq=N // 128 - 2, Hkv=1, m=10 * P + off, ldm=N + dld,
                        gu=11 * P, ldg=2 * N + dld))
    return out


def _line(d):
    return " ".join(f"{k}={v}" for k, v in d.items())


def _mirror(d):
    g = d.get
    ep = {f: g(f, 0) for f in ("q", "k", "v", "cosb", "sinb", "S", "Hq", "Hkv", "m", "ldm", "gu", "ldg")}
    return gemm.g8_takes(d["entry"], (g("a", 0), g("lda", 0), bool(g("a_kc", 0))),
                         (g("b", 0), g("ldb", 0), bool(g("b_kc", 0))), (g("c", 0), g("ldc", 0), True), g("M", 0), g("N", 0), g("K", 0), out_f32=bool(g("out_f32", 0)),
                         beta=g("beta", 0.0), epi=g("epi", "none"), ep=ep, rows=bool(g("rows", 0)), at=g("at", 0),
                         ws=g("ws", 0), ph=g("ph", 0), sq=g("sq", 0))


def _build(tmp, flags, name):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp / name)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", f"-I{os.path.join(ROOT, 'csrc')}",
                        *flags, SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _run(exe, descs):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], input="\n".join(_line(d) for d in descs) + "\n", capture_output=True, text=True,
                       timeout=120, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "ERROR: AddressSanitizer" not in out and "runtime error:" not in out, out[-4000:]
    got = [x == "1" for x in r.stdout.split()]
    assert len(got) == len(descs)
    return got


@pytest.fixture(scope="module", params=["plain", "asan_ubsan"])
def driver(request, tmp_path_factory):
    flags = [] if request.param == "plain" else ["-fsanitize=address,undefined"]
    return _build(tmp_path_factory.mktemp("g8args"), flags, "g8args_" + request.param)


def test_rules_on_both_sides_of_every_boundary(driver):
    got = _run(driver, [d for d, _, _ in CASES])
    bad = [(rule, _line(d), want) for (d, want, rule), g in zip(CASES, got) if g != want]
    assert not bad, bad


def test_python_mirror_agrees_with_the_c_check(driver):
    descs = [d for d, _, _ in CASES] + _grid()
    got = _run(driver, descs)
    bad = [_line(d) for d, g in zip(descs, got) if _mirror(d) != g]
    assert not bad, (len(bad), bad[:5])
    assert 0.02 < sum(got) / len(got) < 0.98  # the grid sits on both sides
