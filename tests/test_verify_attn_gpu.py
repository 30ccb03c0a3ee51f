"""Per-element tests of the multi-row verify attention of speculative decoding: csrc/kernels/decode.hip
``verify_attn_kernel`` through ``torch.ops.mxllm.verify_attn`` / ``verify_attn_kv8``.

Every input is built on the CPU from a fixed seed.  Pools [8 blocks, Hkv, 256, 128] behind a
non-monotonic block table (slot 0 -> blocks 5, 2, 7); every pool row that is not in [0, L + nq) of a used
slot is NaN in K and in V (kv8: codes 0x7F under scale inf, which decode to NaN) -- one such row reaching an
MFMA poisons the output.  The q rows j >= nq of the Gaussian cases are NaN too.  ``out`` has 3 rows more than
the batch and is pre-filled with a canary bit pattern.

One launch mixes nq = (1, 3, n, 0): sequence 0 has one row (slot 2, two blocks), sequence 1 three rows (slot
1), sequence 2 all n rows (slot 0), sequence 3 none (its slot's table points at blocks of another slot).
Base lengths L = 0, 62, 63, 254, 255, 256, 575 put the
rows across a wave's 64-key boundary, across a block and split boundary, and give one case with two blocks
behind (the sequence in the two-block slot 2 stops at L = 511, the last position of its second block).
Heads and n: (8, 2) n 4 and (4, 4) n 8 (one column block, group sizes 4 and 1), (16, 1) n 2 and (16, 2) n 4
(two column blocks, group sizes 16 and 8).

Bitwise: row j of a sequence equals ``decode_attn`` / ``decode_attn_kv8`` called with that row as a sequence
of its own -- the same slot, lens = L + j (len_off 1) and the same max_len.  Columns of the MFMA are
independent and a masked probability is exactly 0, so nothing may differ.
fp64 parity (bf16 pools, Gaussian data): every element against the fp64 softmax, bound ``tests/_parity.py``
DECODE_O_MFMA, each head against its own maximum as tests/test_decode_exact_gpu.py applies it.
One-hot exact: q = 64 e0, K = -64 e0 except +64 e0 at chosen keys, distinct V rows; every probability is
exactly 1 or 0 (tests/test_prefill_paged_gpu.py).  (a) +64 at L + j: rows j .. return V[L + j] bit for bit;
(b) +64 at L and at L + j + 1: rows 0 .. j must not see the second key and return V[L] -- an off-by-one in the
per-column key limit fails here.
Padding: rows j >= nq[b] are zeros, the rows of ``out`` past the batch keep the canary.
Refusals: one call on each side of each rule of ``mx::vf_takes`` that a GPU call can reach; a refused call
raises RuntimeError and leaves pools and ``out`` bitwise unchanged.  (The taken side of each rule is a case
above; the 32-bit rules need sizes no test allocates: tests/test_verify_args.py drives them on the host.)
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
D, BLK, NBLOCKS = 128, 256, 8
TABLE = [[5, 2, 7], [1, 6, 3], [4, 0, 0], [4, 4, 4]]  # slot -> blocks (slot 2 holds 2 blocks, slot 3 is never read)
CANARY = 0x7B5A
EXTRA = 3  # rows of out past the batch
SCALE = 1.0 / math.sqrt(D)

HEADS_N = [(8, 2, 4), (4, 4, 8), (16, 1, 2), (16, 2, 4)]
BASE_LENS = [0, 62, 63, 254, 255, 256, 575]


def _ops():
    from mxllm.ops import native

    return native()


def bits(t):
    return t.view(torch.int16)


def batch(n, L):
    """[(slot, base length, nq)] of the mixed launch."""
    return [(2, min(L, 2 * BLK - 1), 1), (1, L, min(3, n)), (0, L, n), (3, 100, 0)]


def scatter(pool, slot, rows):
    """rows [Hkv, L, ...] -> positions [0, L) of ``slot`` through TABLE."""
    L = rows.shape[1]
    for j in range((L + BLK - 1) // BLK):
        e = min(L, (j + 1) * BLK)
        pool[TABLE[slot][j], :, :e - j * BLK] = rows[:, j * BLK:e]


def make_pools(Hkv, seqs, klog, vlog, fp8):
    """Poisoned pools with rows [0, L + nq) of every sequence that has rows scattered in (the one without
    rows shares a block with another slot and must not be read at all).  bf16: (K, V); kv8: (K codes, K
    scales, V codes, V scales)."""
    if not fp8:
        kp = torch.full((NBLOCKS, Hkv, BLK, D), NAN, dtype=BF16)
        vp = torch.full((NBLOCKS, Hkv, BLK, D), NAN, dtype=BF16)
        for (slot, _, m), k, v in zip(seqs, klog, vlog):
            if not m:
                continue
            scatter(kp, slot, k)
            scatter(vp, slot, v)
        return kp, vp
    from mxllm.serve.quant import kv8_dequantize, kv8_quantize

    kc = torch.full((NBLOCKS, Hkv, BLK, D), 0x7F, dtype=torch.uint8)
    vc = torch.full((NBLOCKS, Hkv, BLK, D), 0x7F, dtype=torch.uint8)
    ks = torch.full((NBLOCKS, Hkv, BLK), float("inf"))
    vs = torch.full((NBLOCKS, Hkv, BLK), float("inf"))
    assert kv8_dequantize(kc[0, 0, :1], ks[0, 0, :1]).isnan().all()
    for (slot, _, m), k, v in zip(seqs, klog, vlog):
        if not m:
            continue
        for codes, scales, rows in ((kc, ks, k), (vc, vs, v)):
            cd, sc = kv8_quantize(rows)
            scatter(codes, slot, cd)
            scatter(scales, slot, sc)
    return kc, ks, vc, vs


def run_verify(ops, dev, q, pools, seqs, n, max_len):
    Hq = q.shape[1]
    B = len(seqs)
    out = torch.full((B * n + EXTRA, Hq * D), CANARY, dtype=torch.int16).view(BF16).to(dev)
    bt = torch.tensor(TABLE, dtype=I32, device=dev)
    lens = torch.tensor([s[1] for s in seqs], dtype=I32, device=dev)
    nq = torch.tensor([s[2] for s in seqs], dtype=I32, device=dev)
    slots = torch.tensor([s[0] for s in seqs], dtype=I32, device=dev)
    pl = [t.to(dev) for t in pools]
    if len(pl) == 2:
        r = ops.verify_attn(q.to(dev), pl[0], pl[1], lens, nq, slots, n, max_len, SCALE, bt, out)
    else:
        r = ops.verify_attn_kv8(q.to(dev), pl[0], pl[1], pl[2], pl[3], lens, nq, slots, n, max_len, SCALE, bt, out)
    assert r.data_ptr() == out.data_ptr()
    return out.cpu()


def run_decode_rows(ops, dev, q, pools, seqs, n, max_len):
    """Every row in use as a sequence of its own through the existing decode kernel: {(b, j): [Hq * D]}."""
    rows = [(b, j) for b, (_, _, m) in enumerate(seqs) for j in range(m)]
    qq = torch.stack([q[b * n + j] for b, j in rows]).to(dev)
    lens = torch.tensor([seqs[b][1] + j for b, j in rows], dtype=I32, device=dev)
    slots = torch.tensor([seqs[b][0] for b, _ in rows], dtype=I32, device=dev)
    bt = torch.tensor(TABLE, dtype=I32, device=dev)
    pl = [t.to(dev) for t in pools]
    if len(pl) == 2:
        o = ops.decode_attn(qq, pl[0], pl[1], lens, slots, max_len, SCALE, 1, bt, None)
    else:
        o = ops.decode_attn_kv8(qq, pl[0], pl[1], pl[2], pl[3], lens, slots, max_len, SCALE, 1, bt)
    return {r: o[i].cpu() for i, r in enumerate(rows)}


def check_padding(out, seqs, n, Hq, name):
    for b, (_, _, m) in enumerate(seqs):
        got = bits(out[b * n + m:(b + 1) * n])
        assert_exact(got, torch.zeros_like(got), name=f"{name}: rows >= nq of sequence {b}")
    got = bits(out[len(seqs) * n:])
    assert got.shape[0] == EXTRA
    assert_exact(got, torch.full_like(got, CANARY), name=f"{name}: rows of out past the batch")


@functools.lru_cache(maxsize=None)
def gauss_case(Hq, Hkv, n, L):
    g = torch.Generator().manual_seed(100000 * Hq + 1000 * Hkv + 10 * L + n)
    seqs = batch(n, L)
    q = torch.randn(len(seqs) * n, Hq, D, generator=g).to(BF16)
    klog, vlog, ref = [], [], {}
    G = Hq // Hkv
    for b, (slot, L0, m) in enumerate(seqs):
        q[b * n + m:(b + 1) * n] = NAN  # rows that are not in use: never multiplied
        klog.append(torch.randn(Hkv, L0 + m, D, generator=g).to(BF16))
        vlog.append(torch.randn(Hkv, L0 + m, D, generator=g).to(BF16))
        k64, v64 = klog[-1].to(F64).repeat_interleave(G, 0), vlog[-1].to(F64).repeat_interleave(G, 0)
        for j in range(m):
            s = torch.einsum("hd,hld->hl", q[b * n + j].to(F64), k64[:, :L0 + j + 1]) * SCALE
            ref[(b, j)] = torch.einsum("hl,hld->hd", s.softmax(-1), v64[:, :L0 + j + 1])  # [Hq, D] fp64
    return dict(q=q, seqs=seqs, klog=klog, vlog=vlog, ref=ref, max_len=max(s[1] + s[2] for s in seqs))


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "kv8"])
@pytest.mark.parametrize("L", BASE_LENS)
@pytest.mark.parametrize("Hq,Hkv,n", HEADS_N)
def test_verify_attn_rows_are_decode_attn_bitwise(gpu, Hq, Hkv, n, L, fp8):
    ops, c = _ops(), gauss_case(Hq, Hkv, n, L)
    seqs = c["seqs"]
    pools = make_pools(Hkv, seqs, c["klog"], c["vlog"], fp8)
    out = run_verify(ops, gpu, c["q"], pools, seqs, n, c["max_len"])
    want = run_decode_rows(ops, gpu, c["q"], pools, seqs, n, c["max_len"])
    assert len(want) == sum(s[2] for s in seqs)
    for (b, j), w in want.items():
        assert_exact(bits(out[b * n + j]), bits(w), name=f"sequence {b} (L {seqs[b][1]}, nq {seqs[b][2]}) row {j}")
        if not fp8:
            assert_parity(out[b * n + j].view(Hq, D), c["ref"][(b, j)], P.DECODE_O_MFMA,
                          name=f"fp64 parity, sequence {b} row {j}")
    check_padding(out, seqs, n, Hq, "gaussian")


def onehot_case(Hq, Hkv, n, L, j, second, fp8):
    """+64 e0 at key L0 + j of every sequence (``second``: at L0 and at L0 + j + 1 instead, the latter only
    where it is one of the sequence's rows), -64 e0 elsewhere; q = 64 e0."""
    g = torch.Generator().manual_seed(7 + Hq + Hkv + L + j)
    seqs = batch(n, L)
    q = torch.zeros(len(seqs) * n, Hq, D, dtype=BF16)
    q[:, :, 0] = 64
    klog, vlog = [], []
    for slot, L0, m in seqs:
        k = torch.zeros(Hkv, L0 + m, D, dtype=BF16)
        k[:, :, 0] = -64
        if m:
            if second:
                k[:, L0, 0] = 64
                if j + 1 < m:
                    k[:, L0 + j + 1, 0] = 64
            elif j < m:
                k[:, L0 + j, 0] = 64
            else:
                k[:, L0, 0] = 64  # (the sequence has no row j: every row sees its first key)
        klog.append(k)
        vlog.append(torch.randn(Hkv, L0 + m, D, generator=g).to(BF16))
    pools = make_pools(Hkv, seqs, klog, vlog, fp8)
    if fp8:  # what the rows decode to
        from mxllm.serve.quant import kv8_dequantize, kv8_quantize

        vlog = [kv8_dequantize(*kv8_quantize(v)) for v in vlog]
    return q, seqs, pools, vlog


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "kv8"])
@pytest.mark.parametrize("second", [False, True], ids=["own_key", "next_key_invisible"])
@pytest.mark.parametrize("L", BASE_LENS)
@pytest.mark.parametrize("Hq,Hkv,n", HEADS_N)
def test_verify_attn_onehot_exact(gpu, Hq, Hkv, n, L, second, fp8):
    ops, G = _ops(), Hq // Hkv
    for j in range(n):
        q, seqs, pools, vlog = onehot_case(Hq, Hkv, n, L, j, second, fp8)
        out = run_verify(ops, gpu, q, pools, seqs, n, max(s[1] + s[2] for s in seqs))
        for b, ((slot, L0, m), v) in enumerate(zip(seqs, vlog)):
            if not m:
                continue
            if second:
                lo, hi, key = 0, min(j + 1, m), L0
            elif j < m:
                lo, hi, key = j, m, L0 + j
            else:
                lo, hi, key = 0, m, L0
            want = v[:, key].repeat_interleave(G, 0).reshape(1, Hq * D).expand(hi - lo, Hq * D)
            assert_exact(bits(out[b * n + lo:b * n + hi]), bits(want.contiguous()),
                         name=f"target row {j}: sequence {b} (L {L0}, nq {m}) rows {lo}..{hi - 1}")
        check_padding(out, seqs, n, Hq, f"one-hot, target row {j}")


def test_verify_attn_refusals(gpu):
    ops, dev = _ops(), gpu
    Hq, Hkv, n, L = 16, 2, 4, 255
    c = gauss_case(Hq, Hkv, n, L)
    seqs, B = c["seqs"], len(c["seqs"])
    kp, vp = (t.to(dev) for t in make_pools(Hkv, seqs, c["klog"], c["vlog"], False))
    k8 = [t.to(dev) for t in make_pools(Hkv, seqs, c["klog"], c["vlog"], True)]
    q = c["q"].to(dev)
    bt = torch.tensor(TABLE, dtype=I32, device=dev)
    lens = torch.tensor([s[1] for s in seqs], dtype=I32, device=dev)
    nq = torch.tensor([s[2] for s in seqs], dtype=I32, device=dev)
    slots = torch.tensor([s[0] for s in seqs], dtype=I32, device=dev)
    out = torch.full((B * n + EXTRA, Hq * D), CANARY, dtype=torch.int16).view(BF16).to(dev)
    kp0, vp0 = bits(kp).clone(), bits(vp).clone()
    k80 = [t.clone() for t in k8]

    def call(q=q, kp=kp, vp=vp, n=n, bt=bt, out=out, lens=lens, nq=nq, slots=slots):
        return ops.verify_attn(q, kp, vp, lens, nq, slots, n, c["max_len"], SCALE, bt, out)

    def call8(q=q, pl=k8, n=n, out=out):
        return ops.verify_attn_kv8(q, pl[0], pl[1], pl[2], pl[3], lens, nq, slots, n, c["max_len"], SCALE, bt, out)

    def first(t, b):  # the first b sequences' entries
        return t[:b].contiguous()

    refused = {
        "dtype of q": (call, dict(q=q.to(torch.float16))),
        "dtype of the pools": (call, dict(kp=kp.to(torch.float16), vp=vp.to(torch.float16))),
        "dtype of out": (call, dict(out=out.to(torch.float16))),
        "u8 pools without scale pools": (call, dict(kp=k8[0], vp=k8[2])),
        "bf16 pools with scale pools": (call8, dict(pl=[kp, k8[1], vp, k8[3]])),
        "head_dim": (call, dict(q=q[:, :, :64].contiguous(), kp=kp[..., :64].contiguous(), vp=vp[..., :64].contiguous(),
                                out=out[:, :Hq * 64].contiguous())),
        "Hq % Hkv": (call, dict(q=q[:, :15].contiguous(), out=out[:, :15 * D].contiguous())),
        "n >= 1": (call, dict(n=0)),
        # 5 rows of a group of 8 are 40 columns (n = 4, 32 columns, is the case above)
        "n * group size <= 32": (call, dict(q=torch.zeros(3 * 5, Hq, D, dtype=BF16, device=dev), n=5, lens=first(lens, 3),
                                            nq=first(nq, 3), slots=first(slots, 3))),
        "n * group size <= 32, kv8": (call8, dict(q=torch.zeros(4 * 5, Hq, D, dtype=BF16, device=dev), n=5,
                                                  out=torch.zeros(4 * 5, Hq * D, dtype=BF16, device=dev))),
        "blk % 256": (call, dict(kp=kp[:, :, :128].contiguous(), vp=vp[:, :, :128].contiguous())),
        "B > 0": (call, dict(q=q[:0], lens=lens[:0], nq=nq[:0], slots=slots[:0])),
        "rows a multiple of n": (call, dict(q=q[:B * n - 1].contiguous())),
    }
    for rule, (fn, kw) in refused.items():
        o = kw.get("out", out)
        before = o.clone()
        with pytest.raises(RuntimeError):
            fn(**kw)
        torch.cuda.synchronize()
        assert torch.equal(o.view(torch.int16), before.view(torch.int16)), rule
        assert torch.equal(bits(kp), kp0) and torch.equal(bits(vp), vp0), rule
        assert all(torch.equal(a, b) for a, b in zip(k8, k80)), rule
    assert torch.equal(bits(out.cpu()), torch.full((B * n + EXTRA, Hq * D), CANARY, dtype=torch.int16)), \
        "a refused call wrote into out"
    # the other side: this very call is taken (and right: the bitwise test has this case)
    call()
    torch.cuda.synchronize()
    assert not torch.equal(bits(out[:B * n].cpu()), torch.full((B * n, Hq * D), CANARY, dtype=torch.int16))
