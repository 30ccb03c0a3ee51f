"""Exact and per-element tests of the decode kernels: csrc/kernels/decode.hip (rope_append, decode_attn,
decode_attn_partials) and the split merge of decode_fuse.h (skinny_merge_linear).

One-hot decode attention.  Keys are random +-1 rows, q[b, h] = c * K[target(b, h)], scale 1: the target
score c * D lies >= 200 log2 units above every other one (asserted on the CPU in fp64), so every other
probability and every cross-wave / cross-split merge weight is exp2 of less than -149, an exact fp32
zero, and out[b, h] = V[target] bit for bit.  With the target row copied to a second key (integer V)
both keys weigh 1, l = 2 and out = bf16((v1 + v2) / 2): the merges as sums, not only as selections.

Poison.  Every cache row at or past a sequence's length, every slot that ``slots`` does not name and
every block that the table does not name holds NaN; one such row read anywhere poisons the output.

Every expectation is built on the CPU by plain indexing (through the block table for the paged cache)
or in fp64; none comes from another kernel.  ``tests/test_decode_inputs.py`` asserts the input
conditions and runs the CPU reference paths through the same builders and assertions.
``python -m tests.test_decode_exact_gpu`` prints the measured constants of tests/_parity.py (no GPU).
"""
import functools
import math

import pytest
import torch

from mxllm.ops import reference as ref
from tests import _parity as P
from tests._parity import assert_exact, assert_parity

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
F32 = torch.float32
F64 = torch.float64
I32 = torch.int32
NAN = float("nan")
LOG2E = 1.4426950408889634
SPLIT = 256  # keys per workgroup (decode.hip kSplit); 4 waves of 64 keys
MIN_MARGIN_LOG2 = 200.0  # fp32 exp2 is exactly 0 below -149
MAX_TOP_LOG2 = 3000.0


def _ops():
    from mxllm.ops import native

    return native()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _dev(t, dev):
    return None if t is None else t.to(dev)


# =========================================================================== cache addressing (plain indexing)
def kv_place(bt, block, slot, t):
    """(first index, row) of position ``t`` of ``slot`` in a contiguous (bt None) or paged cache."""
    if bt is None:
        return slot, t
    return int(bt[slot, t // block]), t % block


def kv_logical(cache, bt, slot, L):
    """Rows 0..L-1 of ``slot`` as [Hkv, L, D], gathered by plain indexing (through the table when paged)."""
    if bt is None:
        return cache[slot, :, :L]
    blk = cache.shape[2]
    parts = [cache[int(bt[slot, j])] for j in range((L + blk - 1) // blk)]
    return torch.cat(parts, 1)[:, :L] if parts else cache[0, :, :0]


def make_layout(g, B, cap, paged):
    """slots (a permutation of more slots than sequences) and, paged, a permuted block table over a
    pool with more blocks than the table names.  Returns (n_first, rows, slots, bt)."""
    nslots = B + 2
    slots = torch.randperm(nslots, generator=g)[:B].to(I32)
    if not paged:
        return nslots, cap, slots, None
    maxb = cap // SPLIT
    nblocks = nslots * maxb + 5
    bt = torch.randperm(nblocks, generator=g)[:nslots * maxb].view(nslots, maxb).to(I32)
    return nblocks, SPLIT, slots, bt


def poison_dead_rows(caches, lens, slots, bt):
    """NaN into every row that no live position (slot, t < len) maps to."""
    n0, _, rows, _ = caches[0].shape
    live = torch.zeros(n0, rows, dtype=torch.bool)
    for b, L in enumerate(lens):
        for t0 in range(0, L, rows):
            i0, r = kv_place(bt, rows, int(slots[b]), t0)
            live[i0, r:r + min(rows, L - t0)] = True
    for c in caches:
        c.transpose(1, 2)[~live] = NAN
    return live


# =========================================================================== one-hot / tie cases
ONEHOT_C = {128: 4.0, 64: 16.0, 32: 64.0}
LENS_SHORT = (1, 63, 64, 65, 255, 256, 257, 511, 512, 513)
LENS_D128 = LENS_SHORT + (2049, 2304)  # nsplit 9: the loop path of decode_combine_kernel
LENS_PAGED = (1, 200, 256, 257, 512, 513, 700)  # ends inside the first block, at a block edge, in the third block
GROUPS_128 = [(8, 8), (6, 2), (8, 2), (16, 2), (16, 1)]  # GQA group sizes 1, 3, 4, 8, 16
GROUPS_SCALAR = [(4, 4), (8, 2), (16, 1)]                # 1, 4, 16
# (D, Hq, Hkv, paged, tie)
ONEHOT_CASES = [(128, hq, hkv, pg, tie) for hq, hkv in GROUPS_128 for pg in (False, True) for tie in (False, True)]
ONEHOT_CASES += [(D, hq, hkv, pg, tie) for D in (64, 32) for hq, hkv in GROUPS_SCALAR for pg in (False, True)
                 for tie in (False, True)]


def onehot_id(c):
    D, Hq, Hkv, paged, tie = c
    return f"D{D}-Hq{Hq}-Hkv{Hkv}-{'paged' if paged else 'contig'}-{'tie' if tie else 'onehot'}"


def case_lens(D, paged):
    return LENS_PAGED if paged else (LENS_D128 if D == 128 else LENS_SHORT)


def case_cap(D, paged):
    return 768 if paged else (2304 if D == 128 else 700)


def target_candidates(L):
    """Keys of a sequence of L keys in the order the heads take them: the last key, key 0, the wave and
    split edges, one key of every 64-key wave (at a different lane each), then the rest."""
    first = [L - 1, 0, 63, 64, 255, 256]
    waves = [64 * w + (w * 23 + 5) % 64 for w in range((L + 63) // 64)]
    out, seen = [], set()
    for t in first + waves + [127, 128, 191, 192, 511, 512] + list(range(min(L, 40))):
        if 0 <= t < L and t not in seen:
            out.append(t)
            seen.add(t)
    return out


# where in the candidate list the heads of a case start: over the cases of one head_dim the heads take
# consecutive candidates, so together they hit every edge and every wave of every split
TARGET_START = {(8, 8): 0, (6, 2): 8, (8, 2): 14, (16, 2): 22, (16, 1): 38, (4, 4): 0}
TARGET_START_SCALAR = {(4, 4): 0, (8, 2): 4, (16, 1): 12}


def pick_targets(L, Hq, Hkv, tie, scalar=False):
    """Per q-head a list of one (one-hot) or two (tie) keys; different keys for the heads of a group.
    The second key of a tie lies in another split (even heads) or another wave of the same split."""
    rep = Hq // Hkv
    cands = target_candidates(L)
    n = len(cands)
    start = (TARGET_START_SCALAR if scalar else TARGET_START)[(Hq, Hkv)] + 3 * tie
    tg = []
    for hk in range(Hkv):
        first = [cands[(start + hk * rep + r) % n] for r in range(rep)]  # distinct while rep <= n (L >= 16)
        used = set(first)
        for r, t1 in enumerate(first):
            ts = [t1]
            if tie:
                near = (0, 1, -1, 2, -2, 5, -5)
                other_split = [t1 + s * SPLIT + d for d in near for s in (1, -1, 2, -2)]
                other_wave = [t1 + s * 64 + d for d in near for s in (1, -1, 2, -2)]
                other_wave = [t for t in other_wave if t // SPLIT == t1 // SPLIT and t // 64 != t1 // 64]
                order = other_split + other_wave if r % 2 == 0 else other_wave + other_split
                t2 = next((t for t in order if 0 <= t < L and t not in used), None)
                if t2 is not None:  # no head's first key, no other head's second key: the copy changes no target
                    used.add(t2)
                    ts.append(t2)
            tg.append(ts)
    return tg


@functools.lru_cache(maxsize=2)
def onehot_case(case, lens=None):
    """Everything of one case on the CPU: q, the poisoned caches, lens, slots, table, the expected
    output (plain indexing), the targets and the fp64 margin / top score in log2 units."""
    D, Hq, Hkv, paged, tie = case
    lens = case_lens(D, paged) if lens is None else lens
    B, cap, c, rep = len(lens), case_cap(D, paged), ONEHOT_C[D], Hq // Hkv
    g = _gen(900 + D + 16 * Hq + Hkv + 2 * paged + tie + 1000 * len(lens))
    n0, rows, slots, bt = make_layout(g, B, cap, paged)
    kc = (torch.randint(0, 2, (n0, Hkv, rows, D), generator=g, dtype=torch.int8) * 2 - 1).to(BF16)
    if tie:
        vc = torch.randint(-64, 65, (n0, Hkv, rows, D), generator=g, dtype=torch.int16).to(BF16)
    else:
        vc = torch.randn(n0, Hkv, rows, D, generator=g).to(BF16)
    targets = [pick_targets(L, Hq, Hkv, tie, D != 128) if L else [[] for _ in range(Hq)] for b, L in enumerate(lens)]
    for b, L in enumerate(lens):  # the tie: the target row copied to its second key
        for h, ts in enumerate(targets[b]):
            if len(ts) == 2:
                (i1, r1), (i2, r2) = (kv_place(bt, rows, int(slots[b]), t) for t in ts)
                kc[i2, h // rep, r2] = kc[i1, h // rep, r1]
    q = torch.zeros(B, Hq, D, dtype=BF16)
    want = torch.zeros(B, Hq, D, dtype=BF16)
    margin, top = float("inf"), 0.0
    for b, L in enumerate(lens):
        if not L:
            continue
        K = kv_logical(kc, bt, int(slots[b]), L)
        V = kv_logical(vc, bt, int(slots[b]), L)
        for h, ts in enumerate(targets[b]):
            q[b, h] = c * K[h // rep, ts[0]]
            want[b, h] = (V[h // rep, ts].double().sum(0) / len(ts)).to(BF16)
            s = (K[h // rep].double() @ q[b, h].double()) * LOG2E
            best = s[ts[0]].item()
            assert all(s[t].item() == best for t in ts)
            s[ts] = -float("inf")
            margin = min(margin, best - s.max().item()) if L > len(ts) else margin
            top = max(top, best)
    poison_dead_rows((kc, vc), lens, slots, bt)
    return dict(q=q, kc=kc, vc=vc, lens=torch.tensor(lens, dtype=I32), slots=slots, bt=bt, cap=cap,
                want=want.view(B, Hq * D), targets=targets, margin=margin, top=top, lens_list=tuple(lens))


def assert_onehot_conditions(c):
    assert c["margin"] >= MIN_MARGIN_LOG2, c["margin"]
    assert c["top"] < MAX_TOP_LOG2, c["top"]


def run_attn(ops, c, dev, scale=1.0, counters=None, max_len=None):
    return ops.decode_attn(c["q"].to(dev), c["kc"].to(dev), c["vc"].to(dev), c["lens"].to(dev), c["slots"].to(dev),
                           c["cap"] if max_len is None else max_len, scale, 0, _dev(c["bt"], dev), counters)


def check_onehot(case, ops, dev):
    c = onehot_case(case)
    assert_onehot_conditions(c)
    out = run_attn(ops, c, dev)
    assert_exact(out.cpu(), c["want"], onehot_id(case))


@pytest.mark.parametrize("case", ONEHOT_CASES, ids=onehot_id)
def test_decode_attn_onehot_exact(gpu, case):
    check_onehot(case, _ops(), gpu)


# --------------------------------------------------------------------------- in-launch merge
HANDOFF_CASES = [(128, 8, 2, False, False), (128, 16, 1, False, True), (128, 6, 2, True, True)]


def check_handoff(case, ops, dev, n_calls=2):
    c = onehot_case(case)
    B, Hkv = len(c["lens_list"]), case[2]
    cnt = torch.zeros(B * Hkv + 5, dtype=I32, device=dev)
    for i in range(n_calls):
        out = run_attn(ops, c, dev, counters=cnt)
        assert_exact(out.cpu(), c["want"], f"{onehot_id(case)} call {i}")
        assert int(cnt.abs().sum()) == 0, "arrival counters not back at zero"


@pytest.mark.parametrize("proto", ["0", "1", "2", "3", "4", None], ids=lambda p: f"handoff-{p}")
@pytest.mark.parametrize("case", HANDOFF_CASES, ids=onehot_id)
def test_decode_attn_in_launch_merge_exact(gpu, case, proto, monkeypatch):
    if proto is None:
        monkeypatch.delenv("MXLLM_DECODE_HANDOFF", raising=False)
    else:
        monkeypatch.setenv("MXLLM_DECODE_HANDOFF", proto)
    check_handoff(case, _ops(), gpu)


# --------------------------------------------------------------------------- empty and degenerate
EMPTY_LENS = [(0,), (0, 0, 0), (0, 5, 0, 300), (257, 0, 64)]


def check_empty(D, lens, ops, dev):
    case = (D, 8, 2, False, False)
    c = onehot_case(case, tuple(lens))
    out = run_attn(ops, c, dev).cpu()
    assert_exact(out, c["want"], f"D{D} lens {lens}")
    for b, L in enumerate(lens):
        if L == 0:
            assert not bits(out[b]).any(), f"row {b} (no keys) is not all zero"
    if D == 128:
        cnt = torch.zeros(len(lens) * 2 + 3, dtype=I32, device=dev)
        assert_exact(run_attn(ops, c, dev, counters=cnt).cpu(), c["want"], f"D{D} lens {lens} in-launch merge")
        assert int(cnt.abs().sum()) == 0


@pytest.mark.parametrize("lens", EMPTY_LENS, ids=lambda l: "lens" + "_".join(map(str, l)))
@pytest.mark.parametrize("D", [128, 64, 32])
def test_decode_attn_empty_rows(gpu, D, lens):
    check_empty(D, lens, _ops(), gpu)


REFUSED_HEADS = [(17, 1), (34, 2), (7, 2), (8, 3)]  # group size 17; Hq % Hkv != 0


def check_refused(ops, dev):
    g = _gen(5)
    for D in (128, 64):
        for Hq, Hkv in REFUSED_HEADS:
            q = torch.randn(2, Hq, D, generator=g).to(BF16).to(dev)
            kc = torch.randn(2, Hkv, 300, D, generator=g).to(BF16).to(dev)
            lens = torch.tensor([5, 300], dtype=I32, device=dev)
            with pytest.raises(RuntimeError):
                ops.decode_attn(q, kc, kc, lens, None, 300, 1.0, 0, None, None)
    # a paged cache whose block size is no multiple of the 256-key split
    q = torch.randn(2, 8, 128, generator=g).to(BF16).to(dev)
    for blk in (128, 320):
        pool = torch.randn(8, 2, blk, 128, generator=g).to(BF16).to(dev)
        before = pool.clone()
        bt = torch.arange(8, dtype=I32).view(2, 4).to(dev)
        lens = torch.tensor([5, 300], dtype=I32, device=dev)
        with pytest.raises(RuntimeError):
            ops.decode_attn(q, pool, pool, lens, None, 4 * blk, 1.0, 0, bt, None)
        assert torch.equal(bits(pool), bits(before))


def test_decode_attn_refusals(gpu):
    check_refused(_ops(), gpu)


def test_decode_layout_refusals(gpu):
    """Operands of the wrong layout or type are refused by rope_append, decode_attn and decode_attn_partials
    before anything is written.  Every refused tensor is one whose misreading would stay inside its own
    storage (the 64-wide caches are cut from buffers of the full size)."""
    ops, g = _ops(), _gen(7)
    B, Hq, Hkv, D, S = 2, 8, 2, 128, 300
    q = torch.randn(B, Hq, D, generator=g).to(BF16).to(gpu)
    qkv = torch.randn(B, (Hq + 2 * Hkv) * D, generator=g).to(BF16).to(gpu)
    cos, sin = (t.to(gpu) for t in ref.rope_tables(S, D, ROPE_THETA, None))

    def cache(rows=S, width=D):
        return torch.randn(2, Hkv, rows, width, generator=g).to(BF16).to(gpu)

    def cache64():
        return cache().view(-1)[:2 * Hkv * S * 64].view(2, Hkv, S, 64)

    good = dict(rows=torch.tensor([5, 299], dtype=I32, device=gpu), slots=torch.tensor([1, 0], dtype=I32, device=gpu),
                kc=cache(), vc=cache())
    bad = {
        "rows as a stride-2 view": dict(rows=torch.tensor([5, 7, 299, 9], dtype=I32, device=gpu)[::2]),
        "slots with B + 1 elements": dict(slots=torch.tensor([1, 0, 1], dtype=I32, device=gpu)),
        "int64 slots": dict(slots=good["slots"].long()),
        "fp16 k_cache": dict(kc=good["kc"].to(torch.float16)),
        "v_cache with more rows": dict(vc=cache(rows=S + 1)),
        "non-contiguous k_cache": dict(kc=cache(width=D + 64)[:, :, :, :D]),
        "caches 64 wide under a 128-wide q": dict(kc=cache64(), vc=cache64()),
    }
    calls = {
        "rope_append": lambda a: ops.rope_append(qkv, cos, sin, a["rows"], a["slots"], a["kc"], a["vc"], Hq, Hkv, D, None),
        "decode_attn": lambda a: ops.decode_attn(q, a["kc"], a["vc"], a["rows"], a["slots"], S, 1.0, 0, None, None),
        "decode_attn_partials": lambda a: ops.decode_attn_partials(q, a["kc"], a["vc"], a["rows"], a["slots"], S, 1.0,
                                                                   0, None),
    }
    for call in calls.values():  # the accepted form of the calls below
        call(good)
    for what, change in bad.items():
        a = {**good, **change}
        before = [a[k].clone() for k in ("kc", "vc")]
        for name, call in calls.items():
            with pytest.raises(RuntimeError):
                call(a)
                pytest.fail(f"{name} accepted {what}")
        for k, b in zip(("kc", "vc"), before):
            assert torch.equal(bits(a[k].contiguous()), bits(b.contiguous())), f"{what}: a refused call wrote to {k}"


# --------------------------------------------------------------------------- partials
def check_partials(case, ops, dev):
    """The (m, l, o) partial of the target's split: m = target score * log2 e, l = 1, o = V[target],
    all exactly; splits past the length hold (-inf, 0)."""
    D, Hq, Hkv, paged, tie = case
    assert D == 128 and not tie
    c = onehot_case(case)
    assert_onehot_conditions(c)
    ml, po = ops.decode_attn_partials(c["q"].to(dev), c["kc"].to(dev), c["vc"].to(dev), c["lens"].to(dev),
                                      c["slots"].to(dev), c["cap"], 1.0, 0, _dev(c["bt"], dev))
    ml, po = ml.cpu(), po.cpu()
    nsplit = (c["cap"] + SPLIT - 1) // SPLIT
    assert tuple(ml.shape) == (len(c["lens_list"]), Hq, nsplit, 2) and tuple(po.shape) == (len(c["lens_list"]), Hq, nsplit, D)
    m_want = (torch.tensor(ONEHOT_C[D] * D, dtype=F32) * torch.tensor(LOG2E, dtype=F32)).item()  # fp32, as the kernel
    want = c["want"].view(-1, Hq, D).float()
    for b, L in enumerate(c["lens_list"]):
        live = (L + SPLIT - 1) // SPLIT
        assert (ml[b, :, live:, 0] == -float("inf")).all() and (ml[b, :, live:, 1] == 0).all(), f"row {b}: dead splits"
        for h in range(Hq):
            sp = c["targets"][b][h][0] // SPLIT
            name = f"{onehot_id(case)} row {b} head {h} split {sp}"
            assert ml[b, h, sp, 0].item() == m_want and ml[b, h, sp, 1].item() == 1.0, (name, ml[b, h, sp].tolist())
            assert_exact(po[b, h, sp], want[b, h], name)


@pytest.mark.parametrize("case", [(128, 8, 2, False, False), (128, 16, 1, True, False), (128, 6, 2, False, False)],
                         ids=onehot_id)
def test_decode_attn_partials_exact(gpu, case):
    check_partials(case, _ops(), gpu)


# =========================================================================== skinny_merge_linear (decode_fuse.h)
MERGE_CASES = [(M, Hq, ns) for M in (1, 3, 4) for Hq in (4, 32) for ns in (1, 4, 8, 9) if M * Hq * 128 <= 32768]


def _pow2_parts(total, n):
    parts = [total]
    while len(parts) < n:
        parts.sort()
        big = parts.pop()
        parts += [big // 2, big // 2]
    return parts


@functools.lru_cache(maxsize=2)
def merge_case(M, Hq, ns, exact):
    """Synthetic split partials.  exact: the same m in every live split of a head, l powers of two that
    sum to 16, integer o: acc / L is exact.  Otherwise different integer m (exp2 exact), Gaussian o.
    Dead splits hold (-inf, 0) and NaN in o; the last row's heads (M > 1) or head 1 (M = 1) are all dead."""
    g = _gen(1300 + 64 * M + Hq + 7 * ns + exact)
    ml = torch.zeros(M, Hq, ns, 2)
    po = torch.full((M, Hq, ns, 128), NAN)
    ref64 = torch.zeros(M, Hq, 128, dtype=F64)
    for m in range(M):
        for h in range(Hq):
            alive = torch.rand(ns, generator=g) < 0.7
            alive[int(torch.randint(0, ns, (1,), generator=g))] = True
            if (M > 1 and m == M - 1) or (M == 1 and h == 1):
                alive[:] = False
            idx = alive.nonzero().flatten().tolist()
            ml[m, h, :, 0] = -float("inf")
            if not idx:
                continue
            if exact:
                mm = torch.full((len(idx),), float(torch.randint(-5, 6, (1,), generator=g)))
                ll = torch.tensor(_pow2_parts(16, len(idx)), dtype=F32)[torch.randperm(len(idx), generator=g)]
                oo = torch.randint(-8, 9, (len(idx), 128), generator=g).float()
            else:
                mm = torch.randint(-3, 4, (len(idx),), generator=g).float()
                ll = torch.rand(len(idx), generator=g) * 199 + 1
                oo = torch.randn(len(idx), 128, generator=g) * ll[:, None]
            ml[m, h, idx, 0], ml[m, h, idx, 1], po[m, h, idx] = mm, ll, oo
            w = torch.exp2(mm.double() - mm.double().max())
            ref64[m, h] = (w[:, None] * oo.double()).sum(0) / (w * ll.double()).sum()
    return ml, po, ref64.view(M, Hq * 128)


@functools.lru_cache(maxsize=2)
def identity_weight(K):
    return torch.eye(K, dtype=BF16)


def check_merge_linear(M, Hq, ns, ops, dev):
    K = Hq * 128
    w = identity_weight(K).to(dev)
    ml, po, ref64 = merge_case(M, Hq, ns, True)
    y = ops.skinny_merge_linear(ml.to(dev), po.to(dev), w).cpu()
    want = ref64.to(F32).to(BF16)
    assert torch.equal(want.double(), ref64)  # the merged row is exact in bf16
    assert_exact(y, want, f"merge M{M} Hq{Hq} nsplit{ns}")
    dead = M - 1 if M > 1 else None
    assert not (bits(y[dead]) if dead is not None else bits(y[0, 128:256])).any(), "all splits empty: zeros"
    ml, po, ref64 = merge_case(M, Hq, ns, False)
    y = ops.skinny_merge_linear(ml.to(dev), po.to(dev), w).cpu()
    assert_parity(y, ref64, P.DECODE_O_F32, name=f"merge (different m) M{M} Hq{Hq} nsplit{ns}")


@pytest.mark.parametrize("M,Hq,ns", MERGE_CASES, ids=lambda v: str(v))
def test_skinny_merge_linear_exact(gpu, M, Hq, ns):
    check_merge_linear(M, Hq, ns, _ops(), gpu)


# =========================================================================== rope_append on the whole cache
ROPE_THETA = 500000.0
# (D, Hq, Hkv, B, max_seq, paged, use_slots); the B = 2752 case: 2752 * 12 * 8 items > 1024 * 256 threads
APPEND_CASES = [(D, 8, 2, 5, 300, paged, sl) for D in (128, 64, 32) for paged, sl in ((False, True), (False, False), (True, True))]
APPEND_CASES += [(128, 8, 2, 2752, 8, False, False), (128, 16, 1, 3, 300, True, True)]


def append_id(c):
    D, Hq, Hkv, B, S, paged, sl = c
    return f"D{D}-Hq{Hq}-Hkv{Hkv}-B{B}-S{S}-{'paged' if paged else 'contig'}-{'slots' if sl else 'noslots'}"


def random_bits_cache(g, shape):
    """bf16 of random bits: NaN patterns, infinities, subnormals and both zeros included."""
    return torch.randint(-32768, 32768, shape, generator=g, dtype=torch.int16).view(BF16)


def append_layout(g, B, Hkv, D, S, paged, use_slots):
    """Caches of random bits, positions (0 and the last one included), slots, block table, RoPE tables."""
    if paged:
        blk, maxb = SPLIT, 2
        cap, nslots = blk * maxb, B + 2
        n0 = nslots * maxb + 3
        bt = torch.randperm(n0, generator=g)[:nslots * maxb].view(nslots, maxb).to(I32)
        shape = (n0, Hkv, blk, D)
    else:
        cap, nslots, bt, shape = S, (B + 2 if use_slots else B), None, (B + 2 if use_slots else B, Hkv, S, D)
    slots = torch.randperm(nslots, generator=g)[:B].to(I32) if use_slots else None
    pos = torch.randint(0, cap, (B,), generator=g).to(I32)
    pos[0], pos[B - 1] = 0, cap - 1
    if B > 2:
        pos[1] = cap - 1 if not paged else SPLIT  # the first row of the second block
    kc, vc = random_bits_cache(g, shape), random_bits_cache(g, shape)
    cos, sin = ref.rope_tables(cap, D, ROPE_THETA, None)
    return dict(kc=kc, vc=vc, pos=pos, slots=slots, bt=bt, cos=cos, sin=sin)


@functools.lru_cache(maxsize=2)
def append_case(case):
    D, Hq, Hkv, B, S, paged, use_slots = case
    g = _gen(1700 + D + Hq + B + 2 * paged + use_slots)
    c = append_layout(g, B, Hkv, D, S, paged, use_slots)
    c["qkv"] = torch.randn(B, (Hq + 2 * Hkv) * D, generator=g).to(BF16)
    return c


def rope64(x, cos, sin, pos):
    """fp64 rotation of x [B, H, D] (reference.apply_rope's pairing) at positions pos [B]."""
    D = x.shape[-1]
    c, s = cos.double()[pos.long()].unsqueeze(1), sin.double()[pos.long()].unsqueeze(1)
    x1, x2 = x.double()[..., :D // 2], x.double()[..., D // 2:]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)


def check_append(name, c, qkv_proj, Hq, Hkv, D, run, dev):
    """``run(kc, vc) -> q`` appends in place on ``dev``.  qkv_proj [B, NH * D]: the bf16-rounded projection
    the rotation starts from.  q and the K rows under ROPE_QK against the fp64 rotation; the V rows and
    EVERY other row of both caches bitwise on the whole tensor."""
    B = qkv_proj.shape[0]
    x = qkv_proj.view(B, Hq + 2 * Hkv, D)

    def parity(out, sl, what):
        assert_parity(out, rope64(x[:, sl], c["cos"], c["sin"], c["pos"]), P.ROPE_QK, name=f"{name}: {what}")

    kc, vc = c["kc"].to(dev, copy=True), c["vc"].to(dev, copy=True)
    q = run(kc, vc).cpu()
    kc, vc = kc.cpu(), vc.cpu()
    rows = kc.shape[2]
    parity(q.reshape(B, Hq, D), slice(0, Hq), "q")
    want_k, want_v = c["kc"].clone(), c["vc"].clone()
    where = []
    for b in range(B):
        i0, r = kv_place(c["bt"], rows, int(c["slots"][b]) if c["slots"] is not None else b, int(c["pos"][b]))
        where.append((i0, r))
        want_v[i0, :, r] = x[b, Hq + Hkv:]
        want_k[i0, :, r] = kc[i0, :, r]  # the K rows: checked per element below, excluded from the bitwise check
    assert len(set(where)) == B
    i0 = torch.tensor([w[0] for w in where])
    r = torch.tensor([w[1] for w in where])
    parity(kc[i0, :, r], slice(Hq, Hq + Hkv), "K rows")
    assert_exact(bits(vc), bits(want_v), f"{name}: V cache (appended rows and every other row)")
    assert_exact(bits(kc), bits(want_k), f"{name}: K cache outside the appended rows")


def check_rope_append(case, ops, dev):
    D, Hq, Hkv, B, S, paged, use_slots = case
    c = append_case(case)

    def run(kc, vc):
        return ops.rope_append(c["qkv"].to(dev), c["cos"].to(dev), c["sin"].to(dev), c["pos"].to(dev),
                               _dev(c["slots"], dev), kc, vc, Hq, Hkv, D, _dev(c["bt"], dev))

    check_append(append_id(case), c, c["qkv"], Hq, Hkv, D, run, dev)


@pytest.mark.parametrize("case", APPEND_CASES, ids=append_id)
def test_rope_append_whole_cache(gpu, case):
    check_rope_append(case, _ops(), gpu)


# =========================================================================== Gaussian accuracy
GAUSS_LENS = (5, 300, 640)
GAUSS_CASES = [(D, 8, 2, paged) for D in (128, 64, 32) for paged in (False, True)]


def gauss_id(c):
    return f"D{c[0]}-Hq{c[1]}-Hkv{c[2]}-{'paged' if c[3] else 'contig'}"


@functools.lru_cache(maxsize=2)
def gauss_case(case):
    D, Hq, Hkv, paged = case
    B, cap = len(GAUSS_LENS), 768
    g = _gen(2100 + D + paged)
    n0, rows, slots, bt = make_layout(g, B, cap, paged)
    kc = torch.randn(n0, Hkv, rows, D, generator=g).to(BF16)
    vc = torch.randn(n0, Hkv, rows, D, generator=g).to(BF16)
    q = torch.randn(B, Hq, D, generator=g).to(BF16)
    poison_dead_rows((kc, vc), GAUSS_LENS, slots, bt)
    return dict(q=q, kc=kc, vc=vc, lens=torch.tensor(GAUSS_LENS, dtype=I32), slots=slots, bt=bt, cap=cap,
                lens_list=GAUSS_LENS)


def attn_model(q, K, V, scale, dt, D):
    """The documented algorithm for one sequence: q [Hq, D], K / V [Hkv, L, D] -> (O [Hq, D] in ``dt``
    before the output rounding).  Online softmax in the exp2 domain per 64-key wave (D = 128: P rounded
    to bf16 before the PV product) or per 256-key split (the scalar kernel, P in fp32), the waves merged
    per split, the splits merged, one division.  dt = fp64: the reference (same result as a plain softmax)."""
    Hq, Hkv = q.shape[0], K.shape[0]
    rep, L = Hq // Hkv, K.shape[1]
    kk, vv = K.to(dt).repeat_interleave(rep, 0), V.to(dt).repeat_interleave(rep, 0)
    if dt == F64:  # the reference: a plain softmax
        return torch.einsum("hl,hld->hd", torch.softmax(torch.einsum("hd,hld->hl", q.to(dt), kk) * scale, -1), vv)
    sl = torch.tensor(scale, dtype=F32) * torch.tensor(LOG2E, dtype=F32)  # the launcher's fp32 product
    s = torch.einsum("hd,hld->hl", q.to(dt), kk) * sl

    def part(a, b):
        m = s[:, a:b].amax(1)
        p = torch.exp2(s[:, a:b] - m[:, None])
        pv = p.to(BF16).to(dt) if (D == 128 and dt != F64) else p
        return m, p.sum(1), torch.einsum("hl,hld->hd", pv, vv[:, a:b])

    def merge(parts):
        M = torch.stack([p[0] for p in parts]).amax(0)
        f = [torch.exp2(p[0] - M) for p in parts]
        return M, sum(fi * p[1] for fi, p in zip(f, parts)), sum(fi[:, None] * p[2] for fi, p in zip(f, parts))

    splits = []
    for a in range(0, L, SPLIT):
        b = min(L, a + SPLIT)
        step = 64 if D == 128 else SPLIT
        splits.append(merge([part(w, min(b, w + step)) for w in range(a, b, step)]))
    _, Lsum, acc = merge(splits)
    return acc / Lsum[:, None]


def gauss_reference(c, dt, D):
    out = []
    for b, L in enumerate(c["lens_list"]):
        K = kv_logical(c["kc"], c["bt"], int(c["slots"][b]), L)
        V = kv_logical(c["vc"], c["bt"], int(c["slots"][b]), L)
        out.append(attn_model(c["q"][b], K, V, 1.0 / math.sqrt(D), dt, D).reshape(-1))
    return torch.stack(out)


def gauss_bound(D):
    return P.DECODE_O_MFMA if D == 128 else P.DECODE_O_F32


def check_gauss(case, ops, dev, in_launch=False):
    D, Hq, Hkv, paged = case
    c = gauss_case(case)
    cnt = torch.zeros(len(GAUSS_LENS) * Hkv + 2, dtype=I32, device=dev) if in_launch else None
    out = run_attn(ops, c, dev, scale=1.0 / math.sqrt(D), counters=cnt, max_len=max(GAUSS_LENS)).cpu()
    assert cnt is None or int(cnt.abs().sum()) == 0, "arrival counters not back at zero"
    r64 = gauss_reference(c, F64, D)
    # per (row, head): the bound's row is one head's output
    assert_parity(out.view(-1, D), r64.view(-1, D), gauss_bound(D), name=gauss_id(case) + (" in-launch" if in_launch else ""))
    return out, r64


@pytest.mark.parametrize("case", GAUSS_CASES, ids=gauss_id)
def test_decode_attn_gaussian_parity(gpu, case):
    check_gauss(case, _ops(), gpu)
    if case[0] == 128:
        check_gauss(case, _ops(), gpu, in_launch=True)


# =========================================================================== yardstick
def _meas(acc, name, y32, r64, out_dtype=BF16):
    from tests.test_rowwise_strict_gpu import _meas as m

    m(acc, name, y32, r64, out_dtype)


def measure():
    """Error of the fp32 model of the documented algorithm (attn_model) against fp64 at the Gaussian
    inputs above, and of the fp32 split merge at the inputs of the different-m merge cases: the
    ``DECODE_O_*_MEASURED`` constants of tests/_parity.py."""
    acc = {}
    for case in GAUSS_CASES:
        D = case[0]
        c = gauss_case(case)
        y32, r64 = gauss_reference(c, F32, D), gauss_reference(c, F64, D)
        _meas(acc, "DECODE_O_MFMA" if D == 128 else "DECODE_O_F32", y32.view(-1, D), r64.view(-1, D))
    for M, Hq, ns in MERGE_CASES:
        ml, po, r64 = merge_case(M, Hq, ns, False)
        m = ml[..., 0]
        w = torch.exp2(m - m.amax(-1, keepdim=True))
        w = torch.where(torch.isfinite(m), w, torch.zeros_like(w))
        y32 = (w[..., None] * torch.nan_to_num(po)).sum(2) / (w * ml[..., 1]).sum(-1, keepdim=True).clamp_min(1e-30)
        _meas(acc, "DECODE_O_F32", y32.view(M, -1), r64)
    return acc


if __name__ == "__main__":
    for name, (rel, ab) in sorted(measure().items()):
        print(f"{name}_MEASURED = ({rel:.3g}, {ab:.3g})")
    for case in ONEHOT_CASES:
        c = onehot_case(case)
        print(f"{onehot_id(case)}: margin {c['margin']:.0f}, top score {c['top']:.0f} (log2 units)")
