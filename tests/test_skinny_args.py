"""The one operand check of the skinny decode GEMM launchers, and the dispatch built on it, without a GPU.

``mx::sk_takes`` (csrc/kernels/skinny_args.h) decides for ``mx_skinny`` (csrc/kernels/skinny_gemm.hip) and
``mx_w8a16_gemm`` (fp8_gemm.hip) whether a launch is taken.  A stand-alone driver
(tests/native/test_skinny_args.cpp) is built with g++ -- plain, and under AddressSanitizer + UBSan: the
M * K product must not overflow -- and fed launch descriptions.  Per line it prints ``sk_takes`` and the
guard of the former launcher (the six ``if (...) return -1;`` expressions, transcribed into the driver):

(a) every rule on both sides of its boundary, the answer written down here (each case names its rule);
(b) on a product grid with every pointer given, ``sk_takes`` equals the former guard on every line;
(c) the rules that are new -- a pointer the launch dereferences is null, a count is not positive -- each
    refuse a launch the former guard took;
(d) ``mxllm.ops.linear.sk_takes``, the Python mirror the dispatch asks, gives the driver's answer on
    every line of (a)-(c).

Dispatch: the predicates of mxllm/ops/linear.py as they were before they asked the mirror, transcribed
over plain numbers, against today's functions on the Llama-3.1 8B / 70B projection shapes and a
perturbation grid.
"""
import importlib
import itertools
import os
import shutil
import subprocess

import pytest
import torch

L = importlib.import_module("mxllm.ops.linear")  # (mxllm.ops.linear is also the function of that name)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "test_skinny_args.cpp")

P = 0x10000  # a non-null address

PLAIN = dict(entry="plain", x=P, ldx=512, w=2 * P, ldw=512, y=3 * P, ldy=16, M=4, N=16, K=512)
SWIGLU = dict(PLAIN, entry="swiglu", ldy=8)  # N = 2F: F = 8
NORM = dict(PLAIN, entry="norm", gamma=4 * P)
NORM_D = dict(NORM, delta=5 * P, ldd=512, h_out=6 * P)
NORM_SW = dict(NORM, swiglu=1, ldy=8)
ROPE = dict(entry="rope", x=P, ldx=512, w=2 * P, ldw=512, M=4, N=512, K=512, cosb=7 * P, sinb=8 * P, pos=9 * P,
            q=10 * P, kc=11 * P, vc=12 * P, Hq=2, Hkv=1, max_seq=256)
ROPE_N = dict(ROPE, norm=1, gamma=4 * P)
ROPE_ND = dict(ROPE_N, delta=5 * P, ldd=512, h_out=6 * P)
MERGE = dict(entry="merge", w=2 * P, ldw=512, y=3 * P, ldy=16, M=4, N=16, K=512, ml=13 * P, po=14 * P, nsplit=1)
W8 = dict(entry="w8", x=P, ldx=512, w=2 * P, y=3 * P, ldy=16, M=4, N=16, K=512, scale=15 * P)
BASES = dict(plain=PLAIN, swiglu=SWIGLU, norm=NORM, norm_delta=NORM_D, norm_swiglu=NORM_SW, rope=ROPE, rope_norm=ROPE_N,
             rope_norm_delta=ROPE_ND, merge=MERGE, w8=W8)


def _k(d, K, **kw):
    """``d`` at another K, the K-long strides with it."""
    out = dict(d, K=K, **kw)
    for ld in ("ldx", "ldw", "ldd"):
        if d.get(ld):
            out[ld] = K
    return out


# (description, taken, rule): the table of the launchers' rules, both sides of each
CASES = [(d, True, f"{name}: base") for name, d in BASES.items()]
for name in ("plain", "swiglu", "w8"):  # up to 32 rows
    CASES += [(dict(BASES[name], M=32), True, f"{name}: M <= 32"), (dict(BASES[name], M=33), False, f"{name}: M <= 32")]
for name in ("norm", "norm_delta", "norm_swiglu", "rope_norm", "rope_norm_delta", "merge"):  # prologue rows in LDS
    d = BASES[name]
    CASES += [(dict(d, M=5), False, f"{name}: M <= 4"), (dict(d, M=1), True, f"{name}: M <= 4"),
              (_k(d, 8192), True, f"{name}: M * K <= 32768"), (_k(d, 8704), False, f"{name}: M * K <= 32768"),
              (_k(d, 8704, M=3), True, f"{name}: M * K <= 32768"), (_k(d, 16384, M=2), True, f"{name}: M * K <= 32768"),
              (_k(d, 2 ** 30), False, f"{name}: M * K in 64 bits (2^32 would wrap to 0)")]
CASES += [(dict(ROPE, M=16), True, "rope: M <= 16 without the prologue"),
          (dict(ROPE, M=17), False, "rope: M <= 16 without the prologue"),
          (_k(ROPE, 8704, M=16), True, "rope: no LDS bound without the prologue")]
for name, d in BASES.items():
    CASES += [(_k(d, 1024), True, f"{name}: K % 512"), (_k(d, 768), False, f"{name}: K % 512"),
              (dict(d, ldw=520), True, f"{name}: ldw % 8"),
              (dict(d, ldw=516), name == "w8", f"{name}: ldw % 8 (w8: code rows are contiguous, ldw unused)"),
              (dict(d, ldw=504), name == "w8", f"{name}: ldw >= K")]
    if not name.startswith("merge"):
        CASES += [(dict(d, ldx=520), True, f"{name}: ldx % 8"), (dict(d, ldx=516), False, f"{name}: ldx % 8"),
                  (dict(d, ldx=504), False, f"{name}: ldx >= K")]
    if not name.startswith("rope"):
        n_out = d["ldy"]
        CASES += [(dict(d, N=24, ldy=24), False, f"{name}: N % 16"), (dict(d, N=528, ldy=528), True, f"{name}: N % 16"),
                  (dict(d, ldy=n_out + 4), True, f"{name}: ldy % 4"), (dict(d, ldy=n_out + 2), False, f"{name}: ldy % 4"),
                  (dict(d, ldy=n_out - 4), False, f"{name}: ldy >= the output row")]
    if name.startswith(("norm", "rope")):
        CASES += [(dict(d, ldd=d.get("ldd", 0) + 8), True, f"{name}: ldd % 8"),
                  (dict(d, ldd=d.get("ldd", 0) + 4), False, f"{name}: ldd % 8 (with or without delta)")]
for name in ("norm_delta", "rope_norm_delta"):
    CASES += [(dict(BASES[name], ldd=504), False, f"{name}: delta => ldd >= K"),
              (dict(BASES[name], h_out=0), False, f"{name}: delta => h_out")]
CASES += [(dict(ROPE, delta=5 * P, ldd=8), True, "rope without the prologue: delta is not looked at"),
          (dict(SWIGLU, N=48, ldy=24), True, "swiglu: ldy >= F, not 2F"),
          (dict(SWIGLU, N=48, ldy=20), False, "swiglu: ldy >= F"),
          (dict(NORM_SW, N=48, ldy=24), True, "norm + swiglu: ldy >= N / 2"),
          (dict(NORM, N=48, ldy=24), False, "norm: ldy >= N"),
          (dict(MERGE, nsplit=0), False, "merge: nsplit >= 1"), (dict(MERGE, nsplit=17), True, "merge: nsplit >= 1"),
          (dict(PLAIN, entry="7"), False, "unknown entry")]

# (c) the new rules: each refuses; none can refuse a call that worked (the kernel would read or write at 0)
NEW = [(dict(d, w=0), f"{name}: W") for name, d in BASES.items()]
NEW += [(dict(d, x=0), f"{name}: X") for name, d in BASES.items() if name != "merge"]
NEW += [(dict(d, y=0), f"{name}: Y") for name, d in BASES.items() if not name.startswith("rope")]
NEW += [(dict(ROPE, **{k: 0}), f"rope: {k}") for k in ("cosb", "sinb", "pos", "q", "kc", "vc")]
NEW += [(dict(ROPE, **{k: v}), f"rope: {k} > 0") for k in ("Hq", "Hkv", "max_seq") for v in (0, -1)]
NEW += [(dict(ROPE, N=640), "rope: N = (Hq + 2 Hkv) * 128"), (dict(ROPE, Hq=2 ** 25 + 2), "rope: N in 64 bits (2^32 + 512 would wrap to N)"),
        (dict(ROPE, bt=16 * P, maxb=0), "rope: a block table needs maxb > 0"),
        (dict(NORM, gamma=0), "norm: gamma"), (dict(ROPE_N, gamma=0), "rope + norm: gamma"),
        (dict(MERGE, ml=0), "merge: ml"), (dict(MERGE, po=0), "merge: po"), (dict(W8, scale=0), "w8: scale")]
NEW_OK = [(dict(ROPE, bt=16 * P, maxb=2), "rope: paged"), (dict(ROPE, gamma=0), "rope without the prologue: no gamma"),
          (dict(ROPE, slots=17 * P), "rope: slots optional")]


def _grid():
    """(b): entries x M around 4 / 16 / 32 x N x K x strides (exact, +8, each one +4 / short; ldy +4 / +2 /
    short) x delta x norm x swiglu, every pointer given."""
    out = []
    strides = [dict(), dict(ldx=8, ldw=8, ldd=8, ldy=8)]
    strides += [{ld: dv} for ld in ("ldx", "ldw", "ldd") for dv in (4, -8)] + [dict(ldy=4), dict(ldy=2), dict(ldy=-4)]
    heads = {16: (2, 1), 24: (1, 1), 528: (8, 2)}
    for entry, M, N, K, ds, delta, norm, swiglu in itertools.product(
            ("plain", "swiglu", "norm", "rope", "merge", "w8"), (1, 3, 4, 5, 15, 16, 17, 31, 32, 33), (16, 24, 528),
            (512, 768, 8192, 8704), strides, (0, 1), (0, 1), (0, 1)):
        Hq, Hkv = heads[N]
        if entry == "rope":
            N = (Hq + 2 * Hkv) * 128
        n_out = N // 2 if entry == "swiglu" or (entry == "norm" and swiglu) else N
        out.append(dict(entry=entry, x=P, ldx=K + ds.get("ldx", 0), w=2 * P, ldw=K + ds.get("ldw", 0), y=3 * P,
                        ldy=n_out + ds.get("ldy", 0), M=M, N=N, K=K, swiglu=swiglu, norm=norm, delta=5 * P * delta,
                        ldd=K + ds.get("ldd", 0), gamma=4 * P, h_out=6 * P, cosb=7 * P, sinb=8 * P, pos=9 * P, q=10 * P,
                        kc=11 * P, vc=12 * P, Hq=Hq, Hkv=Hkv, max_seq=256, ml=13 * P, po=14 * P, nsplit=2, scale=15 * P))
    return out


def _line(d):
    return " ".join(f"{k}={v}" for k, v in d.items())


def _mirror(d):
    g = d.get
    return L.sk_takes(d["entry"], g("M", 0), g("N", 0), g("K", 0), g("ldx", 0), g("ldw", 0), g("ldy", 0), x=g("x", 0),
                      w=g("w", 0), y=g("y", 0), swiglu=bool(g("swiglu", 0)), norm=bool(g("norm", 0)), delta=g("delta", 0),
                      ldd=g("ldd", 0), gamma=g("gamma", 0), h_out=g("h_out", 0), scale=g("scale", 0),
                      rope={k: g(k, 0) for k in ("cosb", "sinb", "pos", "q", "kc", "vc", "Hq", "Hkv", "max_seq", "bt", "maxb")},
                      merge={k: g(k, 0) for k in ("ml", "po", "nsplit")})


def _build(tmp, flags, name):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp / name)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", f"-I{os.path.join(ROOT, 'csrc')}",
                        *flags, SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _run(exe, descs):
    """[(sk_takes, the former guard)] per description."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], input="\n".join(_line(d) for d in descs) + "\n", capture_output=True, text=True,
                       timeout=300, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "ERROR: AddressSanitizer" not in out and "runtime error:" not in out, out[-4000:]
    got = [tuple(x == "1" for x in ln.split()) for ln in r.stdout.splitlines()]
    assert len(got) == len(descs) and all(len(g) == 2 for g in got)
    return got


@pytest.fixture(scope="module", params=["plain", "asan_ubsan"])
def driver(request, tmp_path_factory):
    flags = [] if request.param == "plain" else ["-fsanitize=address,undefined"]
    return _build(tmp_path_factory.mktemp("skargs"), flags, "skargs_" + request.param)


def test_rules_on_both_sides_of_every_boundary(driver):
    got = _run(driver, [d for d, _, _ in CASES])
    bad = [(rule, _line(d), want) for (d, want, rule), (g, _) in zip(CASES, got) if g != want]
    assert not bad, bad
    # ... and the former launchers said the same (the 2^30 lines: their product was 64-bit too)
    bad = [(rule, _line(d)) for (d, _, rule), (g, old) in zip(CASES, got) if g != old]
    assert not bad, bad


def test_the_check_is_the_former_guards_on_a_grid(driver):
    grid = _grid()
    got = _run(driver, grid)
    bad = [_line(d) for d, (g, old) in zip(grid, got) if g != old]
    assert not bad, (len(bad), bad[:5])
    share = sum(g for g, _ in got) / len(got)
    assert 0.02 < share < 0.98, share  # the grid sits on both sides
    for entry in ("plain", "swiglu", "norm", "rope", "merge", "w8"):
        mine = [g for d, (g, _) in zip(grid, got) if d["entry"] == entry]
        assert 0.02 < sum(mine) / len(mine) < 0.98, entry


def test_new_rules_refuse_what_the_kernel_would_dereference(driver):
    got = _run(driver, [d for d, _ in NEW + NEW_OK])
    bad = [(rule, g) for (d, rule), (g, old) in zip(NEW, got) if g or not old]
    assert not bad, bad  # refused now, taken by the former guard
    bad = [rule for (d, rule), (g, old) in zip(NEW_OK, got[len(NEW):]) if not g]
    assert not bad, bad
    given = ("x", "w", "y", "gamma", "h_out", "cosb", "sinb", "pos", "q", "kc", "vc", "Hq", "Hkv", "max_seq", "ml", "po",
             "nsplit", "scale")
    assert all(d[k] > 0 for d in _grid() for k in given)  # the grid holds none of these lines


def test_python_mirror_agrees_with_the_c_check(driver):
    descs = [d for d, _, _ in CASES] + [d for d, _ in NEW + NEW_OK] + _grid()
    got = _run(driver, descs)
    bad = [_line(d) for d, (g, _) in zip(descs, got) if _mirror(d) != g]
    assert not bad, (len(bad), bad[:5])


# =========================================================================== dispatch is what it was
class FakeT:
    """What the dispatch predicates look at of a tensor: a GPU tensor of a shape, row stride and type."""
    is_cuda, requires_grad = True, False

    def __init__(self, shape, ld=None, dtype=torch.bfloat16, contiguous=True):
        self.shape, self.dtype, self._c = torch.Size(shape), dtype, contiguous and ld in (None, shape[-1])
        st = [1]
        for s in reversed(shape[1:]):
            st.insert(0, st[0] * s)
        if ld is not None:
            st[-2] = ld
        self._st = st

    def dim(self):
        return len(self.shape)

    def stride(self, i):
        return self._st[i]

    def is_contiguous(self):
        return self._c


class _Taken:
    def __getattr__(self, name):
        return lambda *a: "taken"


@pytest.fixture
def gpu_like(monkeypatch):
    monkeypatch.setattr(L, "use_native", lambda t: True)
    monkeypatch.setattr(L, "native", lambda: _Taken())
    assert (L.SKINNY_M, L.NORM_M, L._SKINNY_SMALL_W) == (8, 2, 128 << 20)  # the defaults


SKINNY_M, NORM_M, SMALL_W = 8, 2, 128 << 20


def old_skinny_ok(M, N, K, ldx, ldw):
    """``_skinny_ok`` as it was, for bf16 GPU tensors with unit inner strides."""
    if M > 1 and N * K > SMALL_W:
        return False
    return M <= SKINNY_M and K % 512 == 0 and N % 16 == 0 and ldx % 8 == 0 and ldw % 8 == 0


def old_linear(M, N, K, ldx, ldw):
    return SKINNY_M > 0 and M <= SKINNY_M and M > 0 and old_skinny_ok(M, N, K, ldx, ldw)


def old_linear_swiglu(M, N, K, ldx, ldw):
    if N % 16 or not 0 < M <= SKINNY_M:
        return False
    return old_skinny_ok(M, N, K, ldx, ldw)


def old_norm_linear(M, N, K, ldh, ldw, ldd):
    if not 0 < M <= min(NORM_M, SKINNY_M) or M * K > 32768 or N % 16:
        return False
    if not old_skinny_ok(M, N, K, ldh, ldw):
        return False
    return not (ldd is not None and ldd % 8)


def old_qkv_rope_ok(M, N, K, ldh, ldw, Hq, Hkv, norm):
    if not 0 < M <= (min(NORM_M, SKINNY_M) if norm else SKINNY_M) or (norm and M * K > 32768):
        return False
    if N != (Hq + 2 * Hkv) * 128:
        return False
    return old_skinny_ok(M, N, K, ldh, ldw)


def old_qkv_rope_linear(M, N, K, ldh, ldw, Hq, Hkv, norm, ldd):
    if not old_qkv_rope_ok(M, N, K, ldh, ldw, Hq, Hkv, norm):
        return False
    return not (ldd is not None and (not norm or ldd % 8))


def old_engine_merge(B, N, K, wK):
    """mxllm/serve/engine.py's condition for the merged o-projection (B <= 4 is its own policy)."""
    return N % 16 == 0 and K % 512 == 0 and B * K <= 32768 and wK == K


def _projections():
    """(N, K, Hq, Hkv) of the Llama-3.1 8B and 70B projections and heads, whole and as TP-8 shards."""
    out = []
    for H, Hq, Hkv, F in ((4096, 32, 8, 14336), (8192, 64, 8, 28672)):
        for tp in (1, 8):
            out += [((Hq + 2 * Hkv) * 128 // tp, H, Hq // tp, Hkv // tp), (H, Hq * 128 // tp, 0, 0),
                    (2 * F // tp, H, 0, 0), (H, F // tp, 0, 0), (128256 // tp, H, 0, 0)]
    return out


def _dispatch_grid():
    for (N, K, Hq, Hkv), M, dN, dK, xpad, wpad in itertools.product(
            _projections(), (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33), (0, 8), (0, 256), (0, 8, 4), (0, 8, 4)):
        yield M, N + dN, K + dK, K + dK + xpad, K + dK + wpad, Hq, Hkv


def test_dispatch_is_the_former_predicates(gpu_like):
    n = taken = 0
    for M, N, K, ldx, ldw, Hq, Hkv in _dispatch_grid():
        x, w = FakeT((M, K), ldx), FakeT((N, K), ldw)
        at = (M, N, K, ldx, ldw)
        assert L._skinny_ok(x, w) == old_linear(*at), ("linear", at)
        assert (L.linear_swiglu(x, w) is not None) == old_linear_swiglu(*at), ("linear_swiglu", at)
        gamma = FakeT((K,))
        for ldd in (None, K, K + 8, K + 4):
            d = None if ldd is None else FakeT((M, K), ldd)
            for sw in (False, True):
                assert (L.norm_linear(d, x, gamma, 1e-5, w, sw) is not None) == old_norm_linear(*at, ldd), ("norm", at, ldd)
        if Hq:
            cos, kc = FakeT((1024, 64), dtype=torch.float32), FakeT((2, Hkv, 256, 128))
            for norm in (False, True):
                want = old_qkv_rope_ok(*at, Hq, Hkv, norm)
                assert L.qkv_rope_ok(x, w, cos, cos, kc, kc, Hq, Hkv, norm) == want, ("qkv_rope_ok", at, norm)
                for ldd in (None, K, K + 4):
                    d = None if ldd is None else FakeT((M, K), ldd)
                    got = L.qkv_rope_linear(d, x, gamma if norm else None, 1e-5, w, cos, cos, None, None, kc, kc, Hq, Hkv)
                    assert (got is not None) == old_qkv_rope_linear(*at, Hq, Hkv, norm, ldd), ("qkv_rope_linear", at, norm, ldd)
        elif M <= 4 and ldw == K:  # the engine's merged o-projection: a contiguous weight, up to 4 rows
            for wK in (K, K + 128):
                assert L.merge_linear_ok(M, K, FakeT((N, wK))) == old_engine_merge(M, N, K, wK), ("merge", at, wK)
        n += 1
        taken += old_linear(*at)
    assert n > 5000 and 0.02 < taken / n < 0.98, (n, taken)
