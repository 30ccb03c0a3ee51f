"""The launch descriptions and the one operand check each of the training attention, without a GPU.

``mx::af_takes`` / ``mx::ab_takes`` (csrc/kernels/attn_args.h) decide for ``mx_attn_fwd`` / ``mx_attn_bwd``
(csrc/kernels/attn_fwd.hip, attn_bwd.hip) whether a launch is taken; the launchers ask them before anything is
enqueued.  A stand-alone driver (tests/native/test_attn_args.cpp) is built with g++ -- plain, and under
AddressSanitizer + UBSan: the products of the 32-bit overflow rules must not overflow themselves -- and fed
launch descriptions; nothing is preloaded.

(a) every rule on both sides of its boundary, the answer written down here (each case names its rule);
(b) on a grid, the checks equal the guards the launchers and the torch binding had before the header existed
    (transcribed below), except where a rule refuses what could never have been right: listed separately;
(c) the workspace / partial-head arithmetic equals the expressions it replaced, transcribed below;
(d) the Python mirrors in mxllm/ops/attention.py equal the header.
"""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "test_attn_args.cpp")

P = 0x10000  # a non-null address
I32 = 2 ** 31 - 1

# B1 Hq2 Hkv1 S=Sk=65 D32, every pointer set, every element type right
BASE = dict(q=P, k=P, v=P, o=P, lse=P, dout=P, delta=P, dq=P, dkp=P, dvp=P, work=P, q_bf16=1, kv_bf16=1, o_bf16=1,
            lse_f32=1, dout_bf16=1, out_f32=1, B=1, Hq=2, Hkv=1, S=65, Sk=65, D=32, ldo=64, causal=1, dq_mode=3)
ROPE = dict(BASE, D=128, ldo=256, dqkv=P, cos=P, sin=P, dqkv_bf16=1, ldq=512, cos_rows=65)


def _w(base=BASE, **kw):
    return dict(base, **kw)


# (description, af_takes, ab_takes, rule); None: the case does not speak about that direction
CASES = [(BASE, True, True, "base"), (ROPE, True, True, "base with dqkv")]
CASES += [(_w(**{k: 0}), False, False, f"null {k}") for k in ("q", "k", "v", "o", "lse")]
CASES += [(_w(**{k: 0}), True, False, f"null {k} (backward only)") for k in ("dout", "delta", "dkp", "dvp")]
CASES += [(_w(**{k: 0}), False, False, f"dtype: {k}") for k in ("q_bf16", "kv_bf16", "o_bf16", "lse_f32")]
CASES += [(_w(**{k: 0}), True, False, f"dtype: {k}") for k in ("dout_bf16", "out_f32")]
CASES += [(_w(dq=0), None, False, "dq or dqkv"), (_w(ROPE, dq=0), None, True, "dq or dqkv"),
          (_w(dq_mode=1, dq=0), None, False, "dq or dqkv")]
# empty calls are taken whatever else they say
CASES += [(_w(B=0, q=0, D=48, dq_mode=7), True, True, "empty: B"), (_w(S=0, Hq=3, Hkv=2), True, True, "empty: S"),
          (_w(Sk=0), True, True, "empty: Sk (the forward writes o = 0; the backward does nothing)"),
          (_w(Sk=-1), False, True, "Sk >= 0 (forward)")]
CASES += [(_w(Hq=3, Hkv=2, ldo=96), False, False, "Hq % Hkv"), (_w(Hq=4, Hkv=2, ldo=128), True, True, "Hq % Hkv"),
          (_w(Hkv=0), False, False, "Hkv > 0"), (_w(Hq=0, ldo=0), False, False, "Hq > 0"),
          (_w(Hq=-2, Hkv=-1, ldo=0), False, False, "Hq > 0")]
CASES += [(_w(D=d, ldo=2 * d), d in (32, 64, 128), d in (32, 64, 128), "D in {32, 64, 128}")
          for d in (0, 16, 32, 48, 64, 96, 128, 256)]
CASES += [(_w(ldo=64), True, True, "ldo >= Hq * D"), (_w(ldo=56), False, False, "ldo >= Hq * D"),
          (_w(ldo=72), True, True, "ldo % 8"), (_w(ldo=68), False, False, "ldo % 8")]
CASES += [(_w(causal=0), True, True, "causal in {0, 1}"), (_w(causal=2), False, False, "causal in {0, 1}"),
          (_w(causal=-1), False, False, "causal in {0, 1}")]
CASES += [(_w(dq_mode=m), None, m in (1, 2, 3), "dq_mode in 1..3") for m in (0, 1, 2, 3, 4)]
CASES += [(_w(dq_mode=1, work=0), None, True, "work for modes 2 and 3"), (_w(dq_mode=2, work=0), None, False, "work for modes 2 and 3"),
          (_w(dq_mode=3, work=0), None, False, "work for modes 2 and 3")]
# dqkv
CASES += [(_w(ROPE, dq_mode=2), None, False, "dqkv: split mode"), (_w(ROPE, D=64, ldo=128), None, False, "dqkv: D = 128"),
          (_w(ROPE, Sk=66), None, False, "dqkv: Sk = S"), (_w(ROPE, cos=0), None, False, "dqkv: cos"),
          (_w(ROPE, sin=0), None, False, "dqkv: sin"), (_w(ROPE, dqkv_bf16=0), None, False, "dqkv: bf16"),
          (_w(ROPE, ldq=516), None, False, "dqkv: ldq % 8"), (_w(ROPE, ldq=256), None, True, "dqkv: ldq >= Hq * D"),
          (_w(ROPE, ldq=248), None, False, "dqkv: ldq >= Hq * D"), (_w(ROPE, cos_rows=64), None, False, "dqkv: cos_rows >= S"),
          (_w(ROPE, cos_rows=8192), None, True, "dqkv: cos_rows >= S")]
# hpw: q-heads of one KV group, above 1 only for the 8-wave kernel (split mode, D = 128)
CASES += [(_w(ROPE, hpw=0), None, False, "hpw >= 1"), (_w(ROPE, hpw=1), None, True, "hpw >= 1"),
          (_w(ROPE, hpw=2), None, True, "hpw divides the group"), (_w(ROPE, hpw=4), None, False, "hpw divides the group"),
          (_w(hpw=2), None, False, "hpw > 1: D = 128"), (_w(D=128, ldo=256, dq_mode=2, hpw=2), None, False, "hpw > 1: split mode")]
# 32-bit quantities, forward: each product is formed by divisions
CASES += [(_w(ldo=I32 - 7), True, None, "ldo in 31 bits"), (_w(ldo=2 ** 31), False, None, "ldo in 31 bits"),
          (_w(B=1, Hq=I32 // 32, ldo=(I32 // 32) * 32, S=1), True, None, "Hq * D in 31 bits"),
          (_w(B=1, Hq=I32 // 32 + 1, ldo=2 ** 31, S=1), False, None, "Hq * D in 31 bits"),
          (_w(Hq=1, ldo=32, S=I32 - 127), True, None, "S + 127 in 31 bits"), (_w(Hq=1, ldo=32, S=I32 - 126), False, None, "S + 127 in 31 bits"),
          (_w(B=2 ** 15, Hq=2 ** 8, ldo=2 ** 13, S=255, Sk=1), True, None, "B * Hq * S in 31 bits"),
          (_w(B=2 ** 15, Hq=2 ** 8, ldo=2 ** 13, S=256, Sk=1), False, None, "B * Hq * S in 31 bits"),
          (_w(B=2 ** 40, Hq=2 ** 20, ldo=2 ** 25, S=2 ** 10), False, None, "B * Hq * S in 64 bits (2^70 would wrap to 0)"),
          (_w(D=128, ldo=256, Sk=I32 // 256 - 64), True, None, "(Sk + 64) * 2 D in 31 bits"),
          (_w(D=128, ldo=256, Sk=I32 // 256 - 63), False, None, "(Sk + 64) * 2 D in 31 bits"),
          (_w(Sk=2 ** 62), False, None, "(Sk + 64) * 2 D in 64 bits"),
          (_w(B=2 ** 12, Hq=16, Hkv=16, ldo=512, S=1, Sk=2 ** 15 - 1), True, None, "B * Hkv * Sk in 31 bits"),
          (_w(B=2 ** 12, Hq=16, Hkv=16, ldo=512, S=1, Sk=2 ** 15), False, None, "B * Hkv * Sk in 31 bits")]
# 32-bit quantities, backward
CASES += [(_w(Hq=1, D=128, ldo=128, S=I32 // 256 - 64), None, True, "S_pad * 2 D in 31 bits"),
          (_w(Hq=1, D=128, ldo=128, S=I32 // 256 - 63), None, False, "S_pad * 2 D in 31 bits"),
          (_w(S=2 ** 61), None, False, "S_pad * 2 D in 64 bits"),
          (_w(D=128, ldo=256, Sk=I32 // 256 - 128), None, True, "key rows * 2 D in 31 bits"),
          (_w(D=128, ldo=256, Sk=I32 // 256 - 127), None, False, "key rows * 2 D in 31 bits"),
          (_w(Sk=2 ** 62), None, False, "key rows * 2 D in 64 bits"),
          (_w(Hq=2 ** 10, ldo=2 ** 15, S=32704), None, True, "S_pad * Hq * D * 2 in 31 bits (511 q tiles: 2^31 - 2^22)"),
          (_w(Hq=2 ** 10, ldo=2 ** 15, S=32705), None, False, "S_pad * Hq * D * 2 in 31 bits (512 q tiles: 2^31)"),
          (_w(Hq=1, D=128, ldo=128, dq_mode=1, S=4194240), None, True, "S_pad * D * 4 in 31 bits (modes 1, 2)"),
          (_w(Hq=1, D=128, ldo=128, dq_mode=1, S=4194241), None, False, "S_pad * D * 4 in 31 bits (modes 1, 2)"),
          (_w(Hq=1, D=128, ldo=128, dq_mode=2, S=4194241), None, False, "S_pad * D * 4 in 31 bits (modes 1, 2)"),
          (_w(Hq=1, D=128, ldo=128, dq_mode=3, S=4194241), None, True, "S_pad * D * 4: not in the split mode"),
          (_w(B=2 ** 21 - 1, Hq=16, ldo=512, S=64, Sk=1), None, True, "B * Hq * S_pad in 31 bits"),
          (_w(B=2 ** 21, Hq=16, ldo=512, S=64, Sk=1), None, False, "B * Hq * S_pad in 31 bits"),
          (_w(B=2 ** 21 - 1, Hq=16, ldo=512, S=65, Sk=1), None, False, "B * Hq * S_pad in 31 bits (65 rows pad to 128)"),
          (_w(B=2 ** 50, Hq=2 ** 14, ldo=2 ** 19, S=1), None, False, "B * Hq * S_pad in 64 bits (2^70 would wrap to 0)"),
          (_w(B=2 ** 16, Hq=2 ** 8, ldo=2 ** 13, S=1, Sk=127 * 128), None, True, "key blocks * B * Hq in 31 bits"),
          (_w(B=2 ** 16, Hq=2 ** 8, ldo=2 ** 13, S=1, Sk=127 * 128 + 1), None, False, "key blocks * B * Hq in 31 bits"),
          (_w(B=2 ** 12, Hq=16, Hkv=16, ldo=512, S=1, Sk=2 ** 15 - 1), None, True, "B * Hkv * Sk in 31 bits"),
          (_w(B=2 ** 12, Hq=16, Hkv=16, ldo=512, S=1, Sk=2 ** 15), None, False, "B * Hkv * Sk in 31 bits")]


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


NAMES = ("af", "ab", "shape", "s_pad", "nkb", "work", "hpw", "P", "ds", "rope")


def _run(exe, descs):
    """One dict of the driver's answers per description."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], input="\n".join(_line(d) for d in descs) + "\n", capture_output=True, text=True,
                       timeout=300, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "ERROR: AddressSanitizer" not in out and "runtime error:" not in out, out[-4000:]
    got = [dict(zip(NAMES, (int(x) for x in ln.split()))) for ln in r.stdout.splitlines()]
    assert len(got) == len(descs)
    return got


@pytest.fixture(scope="module", params=["plain", "asan_ubsan"])
def driver(request, tmp_path_factory):
    flags = [] if request.param == "plain" else ["-fsanitize=address,undefined"]
    return _build(tmp_path_factory.mktemp("attnargs"), flags, "attnargs_" + request.param)


def test_rules_on_both_sides_of_every_boundary(driver):
    got = _run(driver, [d for d, _, _, _ in CASES])
    bad = [(rule, _line(d), (af, ab), (g["af"], g["ab"])) for (d, af, ab, rule), g in zip(CASES, got)
           if (af is not None and g["af"] != af) or (ab is not None and g["ab"] != ab)]
    assert not bad, bad
    for key, col in (("af", 1), ("ab", 2)):
        ans = [g[key] for c, g in zip(CASES, got) if c[col] is not None]
        assert 0.15 < sum(ans) / len(ans) < 0.85  # the table sits on both sides


# ---- (b) the guards of the launchers and the binding before attn_args.h, transcribed
def _old_fwd(d):
    """attn_fwd (binding): bf16 q / k / v, Hq % Hkv == 0; mx_attn_fwd: B <= 0 or S <= 0 -> nothing to do, then
    Hkv <= 0 || Hq % Hkv || ldo < Hq * D || ldo % 8 -> -1, D not in {32, 64, 128} -> -1."""
    if d["B"] <= 0 or d["S"] <= 0:
        return True
    if d["Hkv"] <= 0 or d["Hq"] % d["Hkv"] or d["ldo"] < d["Hq"] * d["D"] or d["ldo"] % 8:
        return False
    return d["D"] in (32, 64, 128)


def _old_bwd(d):
    """mx_attn_bwd: B, S or Sk <= 0 -> nothing to do; Hkv <= 0 || Hq % Hkv; dq_mode outside 1..3, no work for modes
    2 and 3; dqkv && (dq_mode != 3 || D != 128 || !cos || !sin || ldq % 8 || causal < 0); D; causal < 0.
    attn_bwd_impl (binding): dq_mode in 1..3; a row-strided o has stride % 8 == 0 (a contiguous one Hq * D, a
    multiple of 8 for every D taken); attn_bwd_rope (the only caller with dqkv): D == 128 and Sk == S."""
    if d["B"] <= 0 or d["S"] <= 0 or d["Sk"] <= 0:
        return True
    if d["Hkv"] <= 0 or d["Hq"] % d["Hkv"]:
        return False
    if d["dq_mode"] < 1 or d["dq_mode"] > 3 or (d["dq_mode"] > 1 and not d["work"]):
        return False
    if d.get("dqkv") and (d["dq_mode"] != 3 or d["D"] != 128 or not d["cos"] or not d["sin"] or d["ldq"] % 8
                          or d["causal"] < 0 or d["Sk"] != d["S"]):
        return False
    if d["D"] not in (32, 64, 128) or d["causal"] < 0:
        return False
    return d["ldo"] % 8 == 0


def _grid():
    for B, Hq, Hkv, S, Sk, D, causal, mode, dl, work, dqkv in itertools.product(
            (0, 2), (2, 3, 8), (0, 1, 2), (0, 65), (0, 65, 200), (32, 48, 128), (0, 1), (0, 1, 2, 3, 4), (0, 8, 4, -8),
            (0, P), (0, P)):
        d = _w(B=B, Hq=Hq, Hkv=Hkv, S=S, Sk=Sk, D=D, causal=causal, dq_mode=mode, ldo=Hq * D + dl, work=work)
        if dqkv:
            d.update(dqkv=P, cos=P, sin=P, dqkv_bf16=1, ldq=(Hq + 2 * Hkv) * D, cos_rows=max(S, 1))
        yield d


def test_checks_equal_the_old_guards_on_a_grid(driver):
    descs = list(_grid())
    got = _run(driver, descs)
    # the one rule on this grid that refuses what the old guards let through: a backward whose o rows are
    # shorter than Hq * D (rows that overlap: never an attention output); the forward refused it already
    new_rule = [d for d in descs if _old_bwd(d) and d["B"] > 0 and d["S"] > 0 and d["Sk"] > 0 and d["ldo"] < d["Hq"] * d["D"]]
    assert new_rule and all(d["ldo"] == d["Hq"] * d["D"] - 8 for d in new_rule)
    touched = {id(d) for d in new_rule}
    bad = []
    for d, g in zip(descs, got):
        if g["af"] != _old_fwd(d):
            bad.append(("af", _line(d)))
        want = False if id(d) in touched else _old_bwd(d)
        if g["ab"] != want:
            bad.append(("ab", _line(d)))
    assert not bad, bad[:10]
    assert 0.05 < sum(g["ab"] for g in got) / len(got) < 0.95


# ---- (c) the arithmetic stated three times before the header, transcribed
def _old_hpw(B, Hq, Hkv, Sk, D, mode, on, forced):
    if mode != 3 or D != 128 or not on or Hkv <= 0 or Hq % Hkv:
        return 1
    G, nkb = Hq // Hkv, (Sk + 127) // 128
    if forced > 0:
        return forced if G % forced == 0 else 1
    for hpw in (4, 2):
        if G % hpw == 0 and nkb * B * (Hq // hpw) >= 512:
            return hpw
    return 1


def test_workspace_and_partial_head_arithmetic(driver):
    from_attention = _attention_py()
    descs = []
    for (S, Sk), B, (G, Hkv), D, mode, forced, on in itertools.product(
            ((1, 1), (63, 65), (64, 128), (65, 127), (129, 200), (200, 129), (2048, 2048), (2048, 1920), (2047, 2049)),
            (1, 2, 16), ((1, 8), (2, 4), (4, 2), (8, 8), (3, 2)), (64, 128), (1, 2, 3), (0, 1, 2, 4, 3), (1, 0)):
        descs.append(_w(B=B, Hq=G * Hkv, Hkv=Hkv, S=S, Sk=Sk, D=D, ldo=G * Hkv * D, dq_mode=mode, forced=forced, on=on))
    got = _run(driver, descs)
    sides = set()
    for d, g in zip(descs, got):
        B, Hq, Hkv, S, Sk, D, mode = (d[k] for k in ("B", "Hq", "Hkv", "S", "Sk", "D", "dq_mode"))
        assert g["ab"] == 1, _line(d)
        s_pad, nkb = (S + 63) // 64 * 64, (Sk + 127) // 128
        hpw = _old_hpw(B, Hq, Hkv, Sk, D, mode, d["on"], d["forced"])
        work = {1: 0, 2: nkb * B * Hq * s_pad * D * 4, 3: B * Hq * (nkb * 128) * s_pad * 2}[mode]
        assert (g["s_pad"], g["nkb"], g["work"], g["hpw"], g["P"]) == (s_pad, nkb, work, hpw, Hq // hpw), _line(d)
        # the Python mirrors
        assert g["ds"] == from_attention._ds_bytes_per_head(S, Sk) and B * Hq * g["ds"] == (work if mode == 3 else B * Hq * g["ds"])
        assert bool(g["rope"]) == from_attention.attn_bwd_takes_rope(mode, D, S, Sk) == (mode == 3 and D == 128 and Sk == S)
        if mode == 3 and D == 128 and d["on"] and not d["forced"] and (Hq // Hkv) % 4 == 0:
            sides.add(nkb * B * (Hq // 4) >= 512)
    assert sides == {True, False}  # both sides of the 512-workgroup threshold


def _attention_py():
    """mxllm/ops/attention.py's pure helpers."""
    import mxllm.ops.attention as m
    return m
