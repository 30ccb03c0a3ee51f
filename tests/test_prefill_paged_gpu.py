"""Per-element tests of the paged-KV prefill attention: csrc/kernels/prefill_paged.hip through
``torch.ops.mxllm.prefill_attn_paged``, and the gather route (``mxllm.ops.decode.paged_attention_gather``)
on the same cases.

Every input is built on the CPU from a fixed seed.  Pools [8 blocks, Hkv, 256, 128]; the block tables are a
non-monotonic permutation (slot 0 -> blocks 5, 2, 7); every pool row that is NOT in [0, p0 + n) of a used
slot is NaN in K and in V -- one such row reaching an MFMA poisons the output.  The q tensor has 5 rows
before, between and after the segments that belong to no segment (NaN), and ``out`` is pre-filled with a
canary bit pattern: those rows must come back bit-identical.

Gaussian parity: every output element against the fp64 softmax on the same bf16 inputs, bound
``tests/_parity.py`` ATTN_O -- the kernel keeps attn_fwd.hip's rounding points (P rounded to bf16 before PV,
one deferred rescale rule), so that error model carries over; each head's output row against its own
maximum, as tests/test_attention_strict_gpu.py applies it.

One-hot exact: q = 64 e0 in every row and head, K[j] = -64 e0 except +64 e0 at chosen keys, distinct bf16 V
rows.  The scores are +-4096 scale: the exp2 arguments are exact and every probability is exactly 1 or 0
(the gap is 8192 scale log2(e) > 1000 log2 units), so a row that sees ONE +64 key returns that key's V row
bit for bit.  (a) +64 at p0 + t: rows t .. n - 1 return V[p0 + t] (row t: the diagonal).  (b) +64 at p0 and
at p0 + t + 1: rows 0 .. t must not see the second key and return V[p0]; an off-by-one in the causal mask
fails here.

Staircase exact (every row's diagonal in ONE launch): q = 64 e0 + 2 e1, K[j] = (j // 32) e0 + (j % 32) e1, so
the raw score of key j is exactly 2 j, and a scale whose fp32 product with log2(e) is exactly 128 (searched
and asserted on the CPU): the exp2 arguments are exact multiples of 256, the newest visible key of row t,
p0 + t, has probability exactly 1 and every other one exactly 0, so row t returns V[p0 + t] bit for bit.

Refusals: one call on each side of each rule of the operand check (mx::pp_takes) that a GPU call can reach;
a refused call raises RuntimeError and leaves pools and ``out`` bitwise unchanged.  (The 32-bit overflow
rules need sizes no test allocates: tests/test_prefill_paged_args.py drives them on the host.)
"""
import functools
import math

import pytest
import torch

from tests import _parity as P
from tests._parity import assert_exact, assert_parity

pytestmark = pytest.mark.gpu

BF16, F64, I32 = torch.bfloat16, torch.float64, torch.int32
NAN = float("nan")
D, BLK, NBLOCKS, MAXB, GAP = 128, 256, 8, 3, 5
TABLE = [[5, 2, 7], [1, 6, 3], [4, 0, 0]]  # slot -> blocks (slot 2 holds at most 2 blocks)
CANARY = 0x7B5A
SCALE = 1.0 / math.sqrt(D)

HEADS = [(8, 2), (4, 4), (16, 1)]
# (n, p0) per segment; segment i lives in slot i
SEGMENTS = [((1, 0),), ((1, 255),), ((1, 256),), ((129, 0),), ((130, 191),), ((64, 575),),
            ((3, 0), (128, 300), (200, 17))]


def _ops():
    from mxllm.ops import native

    return native()


def seg_id(segs):
    return "+".join(f"n{n}p{p0}" for n, p0 in segs)


def bits(t):
    return t.view(torch.int16)


def seg_table(segs):
    """[(row0, n, slot, p0)] with GAP unowned rows before, between and after the segments; T."""
    out, row = [], GAP
    for slot, (n, p0) in enumerate(segs):
        out.append((row, n, slot, p0))
        row += n + GAP
    return out, row


def scatter(pool, slot, rows):
    """rows [Hkv, L, D] -> positions [0, L) of ``slot`` through TABLE (plain indexing)."""
    L = rows.shape[1]
    for j in range((L + BLK - 1) // BLK):
        e = min(L, (j + 1) * BLK)
        pool[TABLE[slot][j], :, :e - j * BLK] = rows[:, j * BLK:e]


def make_pools(Hkv, klog, vlog):
    """NaN pools with the logical rows of every used slot scattered in."""
    kp = torch.full((NBLOCKS, Hkv, BLK, D), NAN, dtype=BF16)
    vp = torch.full((NBLOCKS, Hkv, BLK, D), NAN, dtype=BF16)
    for slot, (k, v) in enumerate(zip(klog, vlog)):
        scatter(kp, slot, k)
        scatter(vp, slot, v)
    return kp, vp


def canary_out(T, Hq):
    return torch.full((T, Hq * D), CANARY, dtype=torch.int16).view(BF16)


@functools.lru_cache(maxsize=None)
def gauss_case(Hq, Hkv, segs):
    g = torch.Generator().manual_seed(1000 * Hq + 10 * Hkv + len(segs) + sum(n + p0 for n, p0 in segs))
    table, T = seg_table(segs)
    q = torch.full((T, Hq, D), NAN, dtype=BF16)
    klog, vlog, ref = [], [], []
    for row0, n, slot, p0 in table:
        L = p0 + n
        q[row0:row0 + n] = torch.randn(n, Hq, D, generator=g).to(BF16)
        klog.append(torch.randn(Hkv, L, D, generator=g).to(BF16))
        vlog.append(torch.randn(Hkv, L, D, generator=g).to(BF16))
        G = Hq // Hkv
        k64 = klog[-1].to(F64).repeat_interleave(G, 0)  # [Hq, L, D]
        v64 = vlog[-1].to(F64).repeat_interleave(G, 0)
        s = torch.einsum("nhd,hld->hnl", q[row0:row0 + n].to(F64), k64) * SCALE
        dead = torch.arange(L).view(1, 1, L) > (torch.arange(n).view(1, n, 1) + p0)
        pr = s.masked_fill(dead, float("-inf")).softmax(-1)
        ref.append(torch.einsum("hnl,hld->nhd", pr, v64))  # [n, Hq, D] fp64
    kp, vp = make_pools(Hkv, klog, vlog)
    return dict(q=q, kp=kp, vp=vp, table=table, T=T, ref=ref)


def run_hip(ops, dev, c, Hq, scale=SCALE, table=None):
    out = canary_out(c["T"], Hq).to(dev)
    bt = torch.tensor(TABLE, dtype=I32, device=dev)
    segs = torch.tensor(table if table is not None else c["table"], dtype=I32)
    r = ops.prefill_attn_paged(c["q"].to(dev), c["kp"].to(dev), c["vp"].to(dev), bt, segs, scale, out)
    assert r.data_ptr() == out.data_ptr()
    return out.cpu()


def run_gather(ops, dev, c, Hq, scale=SCALE):
    from mxllm.ops.decode import paged_attention_gather

    out = canary_out(c["T"], Hq).to(dev)
    paged_attention_gather(c["q"].to(dev), c["kp"].to(dev), c["vp"].to(dev), torch.tensor(TABLE, dtype=I32), c["table"],
                           scale, out)
    return out.cpu()


def check_gaps(out, table, T, name):
    owned = torch.zeros(T, dtype=torch.bool)
    for row0, n, _, _ in table:
        owned[row0:row0 + n] = True
    got = bits(out)[~owned]
    assert_exact(got, torch.full_like(got, CANARY), name=f"{name}: rows of no segment")


def check_gauss(out, c, Hq, name):
    for (row0, n, _, p0), ref in zip(c["table"], c["ref"]):
        assert_parity(out[row0:row0 + n].view(n, Hq, D), ref, P.ATTN_O, name=f"{name} O of segment (n {n}, p0 {p0})")
    check_gaps(out, c["table"], c["T"], name)


@pytest.mark.parametrize("segs", SEGMENTS, ids=seg_id)
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_prefill_paged_gaussian_parity(gpu, Hq, Hkv, segs):
    c = gauss_case(Hq, Hkv, segs)
    check_gauss(run_hip(_ops(), gpu, c, Hq), c, Hq, "hip")


@pytest.mark.parametrize("segs", SEGMENTS, ids=seg_id)
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_gather_route_gaussian_parity(gpu, Hq, Hkv, segs):
    c = gauss_case(Hq, Hkv, segs)
    check_gauss(run_gather(_ops(), gpu, c, Hq), c, Hq, "gather")


# =========================================================================== one-hot exact
def onehot_ts(n, p0):
    """Row indices t to aim at: the ends, and the rows whose key p0 + t sits on either side of a 64-key
    tile, a 32-row wave, a 128-row q-block or a 256-key block boundary."""
    ts = {0, n - 1}
    for t in range(n):
        key = p0 + t
        if key % 64 in (0, 63) or key % 256 in (0, 255) or t % 32 in (0, 31) or t % 128 in (0, 127):
            ts.add(t)
    ts = sorted(ts)
    return ts if len(ts) <= 6 else ts[:2] + ts[len(ts) // 2 - 1:len(ts) // 2 + 1] + ts[-2:]


def onehot_case(Hq, Hkv, segs, ts, second):
    """+64 e0 at key p0 + ts[i] of segment i (``second``: at p0 and at p0 + ts[i] + 1 instead, the latter
    only where it is inside the slot's rows), -64 e0 elsewhere; q = 64 e0."""
    g = torch.Generator().manual_seed(7 + Hq + Hkv + sum(ts))
    table, T = seg_table(segs)
    q = torch.full((T, Hq, D), NAN, dtype=BF16)
    klog, vlog = [], []
    for (row0, n, slot, p0), t in zip(table, ts):
        L = p0 + n
        q[row0:row0 + n] = 0
        q[row0:row0 + n, :, 0] = 64
        k = torch.zeros(Hkv, L, D, dtype=BF16)
        k[:, :, 0] = -64
        if second:
            k[:, p0, 0] = 64
            if p0 + t + 1 < L:
                k[:, p0 + t + 1, 0] = 64
        else:
            k[:, p0 + t, 0] = 64
        klog.append(k)
        vlog.append(torch.randn(Hkv, L, D, generator=g).to(BF16))
    kp, vp = make_pools(Hkv, klog, vlog)
    return dict(q=q, kp=kp, vp=vp, table=table, T=T, vlog=vlog)


def check_onehot(out, c, Hq, Hkv, ts, second, name):
    G = Hq // Hkv
    for (row0, n, slot, p0), t, v in zip(c["table"], ts, c["vlog"]):
        lo, hi, key = (0, t + 1, p0) if second else (t, n, p0 + t)
        want = v[:, key].repeat_interleave(G, 0).reshape(1, Hq * D).expand(hi - lo, Hq * D)
        assert_exact(bits(out[row0 + lo:row0 + hi]), bits(want.contiguous()),
                     name=f"{name}: segment (n {n}, p0 {p0}), target t {t}, rows {lo}..{hi - 1}")
    check_gaps(out, c["table"], c["T"], name)


@pytest.mark.parametrize("second", [False, True], ids=["diagonal", "next_key_invisible"])
@pytest.mark.parametrize("segs", SEGMENTS, ids=seg_id)
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_prefill_paged_onehot_exact(gpu, Hq, Hkv, segs, second):
    per_seg = [onehot_ts(n, p0) for n, p0 in segs]
    for i in range(max(len(x) for x in per_seg)):
        ts = [x[min(i, len(x) - 1)] for x in per_seg]
        c = onehot_case(Hq, Hkv, segs, ts, second)
        check_onehot(run_hip(_ops(), gpu, c, Hq), c, Hq, Hkv, ts, second, "hip")


# =========================================================================== staircase exact
def staircase_scale():
    """A scale s with fl32(fl32(s) * fl32(log2 e)) == 128: the launcher's scale * log2(e) is then a power of two."""
    import numpy as np

    log2e = np.float32(1.4426950408889634)
    s = np.float32(128.0) / log2e
    for cand in (s, np.nextafter(s, np.float32(0)), np.nextafter(s, np.float32(1e9))):
        if np.float32(cand) * log2e == np.float32(128.0):
            return float(cand)
    raise AssertionError("no fp32 scale gives scale * log2(e) == 128 exactly")


def staircase_case(Hq, Hkv, segs):
    g = torch.Generator().manual_seed(99 + Hq + Hkv + len(segs))
    table, T = seg_table(segs)
    q = torch.full((T, Hq, D), NAN, dtype=BF16)
    klog, vlog = [], []
    for row0, n, slot, p0 in table:
        L = p0 + n
        q[row0:row0 + n] = 0
        q[row0:row0 + n, :, 0] = 64
        q[row0:row0 + n, :, 1] = 2
        j = torch.arange(L)
        k = torch.zeros(Hkv, L, D, dtype=BF16)
        k[:, :, 0] = (j // 32).to(BF16)
        k[:, :, 1] = (j % 32).to(BF16)
        assert torch.equal(64 * k[0, :, 0].double() + 2 * k[0, :, 1].double(), 2.0 * j)  # exact in bf16
        klog.append(k)
        vlog.append(torch.randn(Hkv, L, D, generator=g).to(BF16))
    kp, vp = make_pools(Hkv, klog, vlog)
    return dict(q=q, kp=kp, vp=vp, table=table, T=T, vlog=vlog)


@pytest.mark.parametrize("segs", SEGMENTS, ids=seg_id)
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_prefill_paged_staircase_every_row_exact(gpu, Hq, Hkv, segs):
    c = staircase_case(Hq, Hkv, segs)
    out = run_hip(_ops(), gpu, c, Hq, scale=staircase_scale())
    for (row0, n, slot, p0), v in zip(c["table"], c["vlog"]):
        want = v[:, p0:p0 + n].repeat_interleave(Hq // Hkv, 0).transpose(0, 1).reshape(n, Hq * D)  # row t: V[p0 + t]
        assert_exact(bits(out[row0:row0 + n]), bits(want.contiguous()), name=f"segment (n {n}, p0 {p0})")
    check_gaps(out, c["table"], c["T"], "staircase")


# =========================================================================== refusals
def test_prefill_paged_refusals(gpu):
    ops, dev = _ops(), gpu
    Hq, Hkv = 8, 2
    c = gauss_case(Hq, Hkv, ((3, 0), (128, 300), (200, 17)))
    table, T = c["table"], c["T"]
    q, kp, vp = c["q"].to(dev), c["kp"].to(dev), c["vp"].to(dev)
    bt = torch.tensor(TABLE, dtype=I32, device=dev)
    out = canary_out(T, Hq).to(dev)
    kp0, vp0 = bits(kp).clone(), bits(vp).clone()

    def call(q=q, kp=kp, vp=vp, bt=bt, table=table, out=out):
        return ops.prefill_attn_paged(q, kp, vp, bt, torch.tensor(table, dtype=I32).reshape(-1, 4), SCALE, out)

    def with_seg(i, **kw):
        t = [dict(zip(("row0", "n", "slot", "p0"), s)) for s in table]
        t[i].update(kw)
        return [(s["row0"], s["n"], s["slot"], s["p0"]) for s in t]

    last = len(table) - 1
    row0_last, n_last = table[last][0], table[last][1]
    refused = {
        "dtype of q": dict(q=q.to(torch.float16)),
        "dtype of the pools": dict(kp=kp.to(torch.float16), vp=vp.to(torch.float16)),
        "dtype of out": dict(out=out.to(torch.float16)),
        "head_dim": dict(q=q[:, :, :64].contiguous(), kp=kp[..., :64].contiguous(), vp=vp[..., :64].contiguous(),
                         out=out[:, :Hq * 64].contiguous()),
        "Hq % Hkv": dict(q=q[:, :7].contiguous(), out=out[:, :7 * D].contiguous()),
        "group size <= 16": dict(q=torch.zeros(T, 34, D, dtype=BF16, device=dev),
                                 out=torch.zeros(T, 34 * D, dtype=BF16, device=dev)),
        "blk % 256": dict(kp=kp[:, :, :128].contiguous(), vp=vp[:, :, :128].contiguous()),
        "n > 0": dict(table=with_seg(0, n=0)),
        "rows at or past 0": dict(table=with_seg(0, row0=-1)),
        "rows below T": dict(table=with_seg(last, row0=T - n_last + 1)),
        "p0 >= 0": dict(table=with_seg(0, p0=-1)),
        "p0 + n <= maxb * blk": dict(table=with_seg(0, p0=MAXB * BLK - 3 + 1)),
        "slot >= 0": dict(table=with_seg(0, slot=-1)),
        "slot inside the table": dict(table=with_seg(0, slot=len(TABLE))),
        "disjoint rows": dict(table=with_seg(last, row0=row0_last - GAP - 1)),
    }
    for rule, kw in refused.items():
        o = kw.get("out", out)
        before = o.clone()
        with pytest.raises(RuntimeError):
            call(**kw)
        torch.cuda.synchronize()
        assert torch.equal(o.view(torch.int16), before.view(torch.int16)), rule
        assert torch.equal(bits(kp), kp0) and torch.equal(bits(vp), vp0), rule
    assert torch.equal(bits(out.cpu()), bits(canary_out(T, Hq))), "a refused call wrote into out"

    # the other side of each rule: taken, and right.  Group size 16 and Hq % Hkv == 0 are HEADS cases, blk 256
    # and head_dim 128 every case, slot = slots - 1 this one.  Rows: the same segments over q without its
    # first and last unowned rows -- the first segment starts at row 0, the last ends at row T - 1
    T2 = row0_last + n_last - GAP
    c2 = dict(c, q=c["q"][GAP:GAP + T2].contiguous(), T=T2, table=[(r - GAP, n, sl, p0) for r, n, sl, p0 in table])
    check_gauss(run_hip(ops, dev, c2, Hq), c2, Hq, "rows 0 .. T - 1")
    # p0 + n == maxb * blk: the last position a table row can hold (slot 0 has 3 blocks)
    full = gauss_case(Hq, Hkv, ((2, MAXB * BLK - 2),))
    check_gauss(run_hip(ops, dev, full, Hq), full, Hq, "p0 + n == maxb * blk")
