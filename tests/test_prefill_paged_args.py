"""The launch description and the one operand check of the paged-KV prefill attention, without a GPU.

``mx::pp_takes`` (csrc/kernels/prefill_paged_args.h) decides for ``mx_prefill_attn_paged``
(csrc/kernels/prefill_paged.hip) whether a launch is taken; the torch binding asks it on the host before
anything is uploaded or enqueued.  A stand-alone driver (tests/native/test_prefill_paged_args.cpp) is built
with g++ -- plain, and under AddressSanitizer + UBSan: the products of the 32-bit overflow rules must not
overflow themselves -- and fed launch descriptions; nothing is preloaded.

(a) every rule on both sides of its boundary, the answer written down here (each case names its rule);
(b) the work table: one (segment, q-block) per 128 query rows, ordered by the keys a block streams, most
    first, against the same order computed here.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "test_prefill_paged_args.cpp")

P = 0x10000  # a non-null address
I32 = 2 ** 31 - 1

BASE = dict(q=P, k=2 * P, v=3 * P, o=4 * P, bt=5 * P, segs=6 * P, work=7 * P, q_bf16=1, kv_bf16=1, o_bf16=1, T=400, Hq=8,
            Hkv=2, D=128, blocks=8, blk=256, slots=3, maxb=3, ldo=1024, seg=[(5, 3, 0, 0), (13, 128, 1, 300), (146, 200, 2, 17)])


def _with(seg=None, **kw):
    d = dict(BASE, **kw)
    if seg is not None:
        d["seg"] = seg
    return d


def _seg(i, **kw):
    """BASE's segments with fields of segment ``i`` replaced."""
    names = ("row0", "n", "slot", "p0")
    segs = [dict(zip(names, s)) for s in BASE["seg"]]
    segs[i].update(kw)
    return [tuple(s[k] for k in names) for s in segs]


# (description, taken, rule)
CASES = [(BASE, True, "base")]
CASES += [(_with(**{k: 0}), False, f"null {k}") for k in ("q", "k", "v", "o", "bt", "segs", "work")]
CASES += [(_with(**{k: 0}), False, f"dtype: {k}") for k in ("q_bf16", "kv_bf16", "o_bf16")]
CASES += [(_with(D=64), False, "head_dim 128"), (_with(D=256, ldo=2048), False, "head_dim 128")]
CASES += [(_with(Hq=7), False, "Hq % Hkv"), (_with(Hq=6, ldo=768), True, "Hq % Hkv"),
          (_with(Hq=32, ldo=4096), True, "group size <= 16"), (_with(Hq=34, ldo=4352), False, "group size <= 16"),
          (_with(Hkv=0), False, "Hkv > 0"), (_with(Hq=0), False, "Hq > 0"), (_with(Hq=-8, Hkv=-2), False, "Hq > 0")]
CASES += [(_with(blk=512), True, "blk % 256"), (_with(blk=128, maxb=6), False, "blk % 256"),
          (_with(blk=320), False, "blk % 256"), (_with(blk=0), False, "blk > 0")]
CASES += [(_with(**{k: 0}), False, f"{k} > 0") for k in ("T", "blocks", "slots", "maxb")]
CASES += [(_with(seg=[]), False, "at least one segment")]
CASES += [(_with(ldo=1032), True, "ldo % 4 (8-B stores)"), (_with(ldo=1026), False, "ldo % 4 (8-B stores)"),
          (_with(ldo=1020), False, "ldo >= Hq * D")]
# segments
CASES += [(_with(seg=_seg(0, n=0)), False, "n > 0"), (_with(seg=_seg(0, n=-1)), False, "n > 0"),
          (_with(seg=_seg(0, n=1)), True, "n > 0"),
          (_with(seg=_seg(0, row0=0)), True, "rows at or past 0"), (_with(seg=_seg(0, row0=-1)), False, "rows at or past 0"),
          (_with(seg=_seg(2, row0=200)), True, "rows below T (the last row is T - 1)"),
          (_with(seg=_seg(2, row0=201)), False, "rows below T"),
          (_with(seg=_seg(0, p0=-1)), False, "p0 >= 0"),
          (_with(seg=_seg(0, p0=765)), True, "p0 + n <= maxb * blk"), (_with(seg=_seg(0, p0=766)), False, "p0 + n <= maxb * blk"),
          (_with(seg=_seg(0, slot=2)), True, "slot inside the table (two segments may read one slot)"),
          (_with(seg=_seg(0, slot=3)), False, "slot inside the table"), (_with(seg=_seg(0, slot=-1)), False, "slot >= 0"),
          (_with(seg=_seg(1, row0=8)), True, "disjoint rows (adjacent)"), (_with(seg=_seg(1, row0=7)), False, "disjoint rows"),
          (_with(seg=_seg(2, row0=140)), False, "disjoint rows"),
          (_with(seg=[(146, 200, 2, 17), (5, 3, 0, 0), (13, 128, 1, 300)]), True, "segments in any order"),
          (_with(seg=[(0, 400, 0, 0), (0, 400, 1, 0)]), False, "disjoint rows (the same rows twice)")]
CASES += [(_with(nwork=3), False, "nwork is the q-block count"), (_with(nwork=4), True, "nwork is the q-block count"),
          (_with(nwork=5), False, "nwork is the q-block count")]
# 32-bit offsets: each product is formed in 64 bits
CASES += [(_with(blk=2 ** 22, maxb=1), True, "blk * 256 bytes in 31 bits"), (_with(blk=2 ** 23, maxb=1), False, "blk * 256 bytes in 31 bits"),
          (_with(blk=2 ** 40, maxb=1), False, "blk * 256 in 64 bits (2^48 would wrap in 32)"),
          (_with(maxb=2 ** 23 - 1), True, "maxb * blk in 31 bits"), (_with(maxb=2 ** 23), False, "maxb * blk in 31 bits"),
          (_with(maxb=2 ** 56), False, "maxb * blk in 64 bits"),
          (_with(slots=2 ** 29, maxb=3), True, "slots * maxb in 31 bits"), (_with(slots=2 ** 30, maxb=3), False, "slots * maxb in 31 bits"),
          (_with(ldo=I32 - 3), True, "ldo in 31 bits"), (_with(ldo=2 ** 31), False, "ldo in 31 bits"),
          (_with(T=2 ** 31 - 1, Hq=16, Hkv=1, ldo=2048, seg=[(0, 2 ** 31 - 256, 0, 0)], maxb=2 ** 23 - 1), True,
           "nwork * Hq in 31 bits (2^24 - 2 q-blocks x 16 heads < 2^28)"),
          (_with(T=2 ** 31 - 1, Hq=256, Hkv=16, ldo=32768, seg=[(0, 2 ** 31 - 256, 0, 0)], maxb=2 ** 23 - 1), False,
           "nwork * Hq in 31 bits (2^24 - 2 q-blocks x 256 heads = 2^32 - 512)"),
          (_with(T=2 ** 31 - 1, seg=[(2 ** 31 - 2, 1, 0, 0)]), True, "row0 + n in 64 bits"),
          (_with(T=2 ** 31 - 1, seg=[(2 ** 31 - 1, 1, 0, 0)]), False, "row0 + n in 64 bits (would wrap negative in 32)"),
          (_with(seg=[(0, 1, 0, 2 ** 31 - 1)], maxb=2 ** 23 - 1), False, "p0 + n in 64 bits (would wrap negative in 32)")]


def _line(d):
    out = []
    for k, v in d.items():
        if k == "seg":
            out += ["seg=" + ":".join(str(x) for x in s) for s in v]
        else:
            out.append(f"{k}={v}")
    return " ".join(out)


def _build(tmp, flags, name):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp / name)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", f"-I{os.path.join(ROOT, 'csrc')}",
                        *flags, SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _run(exe, descs):
    """[(pp_takes, nwork, [(segment, q-block)])] per description."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], input="\n".join(_line(d) for d in descs) + "\n", capture_output=True, text=True,
                       timeout=300, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "ERROR: AddressSanitizer" not in out and "runtime error:" not in out, out[-4000:]
    got = []
    for ln in r.stdout.splitlines():
        f = ln.split()
        got.append((f[0] == "1", int(f[1]), [tuple(int(x) for x in w.split(":")) for w in f[2:]]))
    assert len(got) == len(descs)
    return got


@pytest.fixture(scope="module", params=["plain", "asan_ubsan"])
def driver(request, tmp_path_factory):
    flags = [] if request.param == "plain" else ["-fsanitize=address,undefined"]
    return _build(tmp_path_factory.mktemp("ppargs"), flags, "ppargs_" + request.param)


def test_rules_on_both_sides_of_every_boundary(driver):
    got = _run(driver, [d for d, _, _ in CASES])
    bad = [(rule, _line(d), want) for (d, want, rule), (g, _, _) in zip(CASES, got) if g != want]
    assert not bad, bad
    share = sum(g for g, _, _ in got) / len(got)
    assert 0.15 < share < 0.85, share  # the table sits on both sides


def _work(segs):
    """The work table as documented: one (segment, q-block) per 128 rows, most keys first, ties in
    segment then q-block order."""
    items = [(-(p0 + min(n, (qb + 1) * 128)), i, qb) for i, (_, n, _, p0) in enumerate(segs) for qb in range((n + 127) // 128)]
    return [(i, qb) for _, i, qb in sorted(items)]


def test_work_table_is_heaviest_first(driver):
    cases = [BASE["seg"], [(0, 1, 0, 0)], [(0, 128, 0, 0)], [(0, 129, 0, 0)], [(0, 2048, 0, 30720)],
             [(0, 600, 0, 0), (600, 57, 1, 512), (657, 1, 2, 255), (658, 300, 0, 0)]]
    got = _run(driver, [dict(seg=s) for s in cases])
    for segs, (_, nwork, work) in zip(cases, got):
        assert nwork == sum((n + 127) // 128 for _, n, _, _ in segs)
        assert work == _work(segs), segs
        keys = [p0 + min(n, (qb + 1) * 128) for i, qb in work for _, n, _, p0 in [segs[i]]]
        assert keys == sorted(keys, reverse=True)
