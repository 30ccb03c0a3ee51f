"""The exact and per-element decode-path tests (tests/test_decode_exact_gpu.py, tests/test_skinny_exact_gpu.py)
on the CPU: every input condition they rest on, the CPU reference paths through the very same builders
and assertions (a wrong test fails here, not on the GPU), and localized corruptions that the norm
thresholds of tests/test_model_gpu.py (``_rel < 2e-2``) and tests/test_kernels_gpu.py (``rel_err < 1e-2``)
accept and these checks reject."""
import math

import pytest
import torch

from mxllm.ops import decode as dops
from mxllm.ops.linear import sk_takes
from mxllm.serve.quant import dequantize_e4m3
from tests import _parity as P
from tests import test_decode_exact_gpu as TD
from tests import test_skinny_exact_gpu as TS
from tests._parity import assert_exact, assert_parity

BF16, F32, F64, I32 = torch.bfloat16, torch.float32, torch.float64, torch.int32
CPU = torch.device("cpu")


def _assert_measured(name, rel, ab):
    """The recorded pair follows the rule of tests/_parity.py, and a fresh measurement agrees with it.
    The abs term is the error of an fp32 matmul, whose summation order (the BLAS blocking) differs from
    one CPU to the next: the recorded value is reproduced to 3 digits on the machine it was taken on
    (``python -m tests.test_..._exact_gpu``), elsewhere within the factor 2 the bound itself allows."""
    rel0, ab0 = getattr(P, name + "_MEASURED")
    assert getattr(P, name) == (max(2 * rel0, P.ULP_BF16), float(f"{2 * ab0:.3g}")), name
    assert abs(rel - rel0) <= 1e-4 and ab0 / 2 <= ab <= 2 * ab0, (name, rel, ab)


def _norm_ratio(out, ref):
    return ((out.double() - ref.double()).norm() / ref.double().norm()).item()


# =========================================================================== reference ops (plain PyTorch)
class RefDecode:
    """The contracts of rope_append, decode_attn, decode_attn_partials and skinny_merge_linear in plain
    fp32 PyTorch, refusals included.  ``edit``: hooks for the corruption tests."""

    def __init__(self, table_edit=None, p_edit=None, head_edit=None):
        self.table_edit, self.p_edit, self.head_edit = table_edit, p_edit, head_edit

    def _check(self, q, kc, bt):
        Hq, Hkv = q.shape[1], kc.shape[1]
        if Hq % Hkv or Hq // Hkv > 16 or (bt is not None and kc.shape[2] % 256):
            raise RuntimeError("decode_attn: refused")

    def decode_attn(self, q, kc, vc, lens, slots, max_len, scale, len_off=0, bt=None, counters=None):
        self._check(q, kc, bt)
        B, Hq, D = q.shape
        rep = Hq // kc.shape[1]
        bt = self.table_edit(bt) if self.table_edit and bt is not None else bt
        out = torch.zeros(B, Hq, D)
        for b in range(B):
            L, slot = int(lens[b]) + len_off, int(slots[b]) if slots is not None else b
            if L <= 0:
                continue
            K = TD.kv_logical(kc, bt, slot, L).float().repeat_interleave(rep, 0)
            V = TD.kv_logical(vc, bt, slot, L).float().repeat_interleave(rep, 0)
            p = torch.softmax(torch.einsum("hd,hld->hl", q[b].float(), K) * scale, -1)
            if self.p_edit:
                p = self.p_edit(b, p)
            out[b] = torch.einsum("hl,hld->hd", p, V)
            if self.head_edit:
                out[b] = self.head_edit(b, out[b])
        return out.to(BF16).view(B, Hq * D)

    def decode_attn_partials(self, q, kc, vc, lens, slots, max_len, scale, len_off=0, bt=None):
        self._check(q, kc, bt)
        B, Hq, D = q.shape
        rep = Hq // kc.shape[1]
        cap = kc.shape[2] * (bt.shape[1] if bt is not None else 1)
        ns = max(1, (min(max_len, cap) + 255) // 256)
        ml = torch.zeros(B, Hq, ns, 2)
        ml[..., 0] = -float("inf")
        po = torch.full((B, Hq, ns, D), float("nan"))
        sl = torch.tensor(scale, dtype=F32) * torch.tensor(TD.LOG2E, dtype=F32)
        for b in range(B):
            L, slot = int(lens[b]) + len_off, int(slots[b]) if slots is not None else b
            K = TD.kv_logical(kc, bt, slot, L).float().repeat_interleave(rep, 0)
            V = TD.kv_logical(vc, bt, slot, L).float().repeat_interleave(rep, 0)
            for s, a in enumerate(range(0, L, 256)):
                x = torch.einsum("hd,hld->hl", q[b].float(), K[:, a:a + 256]) * sl
                m = x.amax(1)
                p = torch.exp2(x - m[:, None])
                ml[b, :, s, 0], ml[b, :, s, 1] = m, p.sum(1)
                po[b, :, s] = torch.einsum("hl,hld->hd", p, V[:, a:a + 256])
        return ml, po

    def skinny_merge_linear(self, ml, po, w):
        M, Hq, ns, _ = ml.shape
        if not sk_takes("merge", M, w.shape[0], Hq * 128, ldw=w.stride(0), ldy=w.shape[0], merge={"nsplit": ns}):
            raise RuntimeError("skinny_merge_linear: refused")
        m = ml[..., 0]
        wgt = torch.where(torch.isfinite(m), torch.exp2(m - m.amax(-1, keepdim=True)), torch.zeros_like(m))
        Ls = (wgt * ml[..., 1]).sum(-1, keepdim=True)
        acc = (wgt[..., None] * torch.nan_to_num(po)).sum(2)
        x = torch.where(Ls > 0, acc / Ls.clamp_min(1e-30), torch.zeros_like(acc)).to(BF16).view(M, Hq * 128)
        return (x.float() @ w.float().t()).to(BF16)

    def rope_append(self, qkv, cos, sin, pos, slots, kc, vc, Hq, Hkv, D, bt=None):
        """mxllm.ops.decode.decode_attention's append (its CPU path), the attention output dropped."""
        B = qkv.shape[0]
        sl = slots if slots is not None else torch.arange(B, dtype=I32)
        dops.decode_attention(qkv, cos, sin, kc, vc, pos, sl, Hq, Hkv, D, 0, bt)
        x = qkv.view(B, Hq + 2 * Hkv, D).float()
        c, s = cos[pos.long()].unsqueeze(1), sin[pos.long()].unsqueeze(1)
        q1, q2 = x[:, :Hq, :D // 2], x[:, :Hq, D // 2:]
        return torch.cat([q1 * c - q2 * s, q2 * c + q1 * s], -1).to(BF16)


REF = RefDecode()


# =========================================================================== decode: the cases on the CPU
@pytest.mark.parametrize("case", TD.ONEHOT_CASES, ids=TD.onehot_id)
def test_onehot_cases_hold_their_conditions(case):
    """Margin >= 200 and top score < 3000 log2 units (asserted inside, fp64); q really c * the target row;
    the heads of a group on different keys; the second key of a tie in another wave or split; NaN in
    every dead row; and the fp32 reference is exactly one-hot."""
    D, Hq, Hkv, paged, tie = case
    c = TD.onehot_case(case)
    TD.check_onehot(case, REF, CPU)
    rep = Hq // Hkv
    for b, L in enumerate(c["lens_list"]):
        K = TD.kv_logical(c["kc"], c["bt"], int(c["slots"][b]), L)
        assert torch.isfinite(K).all()
        for hk in range(Hkv):
            grp = c["targets"][b][hk * rep:(hk + 1) * rep]
            keys = [t for ts in grp for t in ts]
            assert L < 16 or len(set(keys)) == len(keys)
            for r, ts in enumerate(grp):
                assert torch.equal(c["q"][b, hk * rep + r], (TD.ONEHOT_C[D] * K[hk, ts[0]]).to(BF16))
                assert len(ts) == 2 if tie and L >= 192 else len(ts) <= 1 + tie
                if len(ts) == 2:
                    assert ts[0] // 64 != ts[1] // 64
    live = sum(c["lens_list"])
    assert int(torch.isfinite(c["kc"][:, 0, :, 0]).sum()) == live and int(torch.isfinite(c["vc"][:, 0, :, 0]).sum()) == live
    if paged:
        named = set(c["bt"].flatten().tolist())
        assert len(named) < c["kc"].shape[0] and len(named) == c["bt"].numel()  # spare blocks, no block twice


def test_onehot_targets_cover_every_wave_and_edge():
    hit, ties = set(), {"wave": 0, "split": 0}
    for case in TD.ONEHOT_CASES:
        if case[0] != 128 or case[3]:
            continue
        for b, L in enumerate(TD.case_lens(128, False)):
            for ts in TD.pick_targets(L, case[1], case[2], case[4]):
                hit.add(ts[0] // 64)
                if L == 2304:
                    hit.add(("t", ts[0]))
                if len(ts) == 2:
                    ties["split" if ts[0] // 256 != ts[1] // 256 else "wave"] += 1
                if ts[0] == L - 1:
                    hit.add(("last", L))
    assert {w for w in hit if isinstance(w, int)} == set(range(36))  # every wave quarter of every split
    assert {("t", t) for t in (0, 63, 64, 255, 256, 2303)} <= hit
    assert {("last", L) for L in TD.LENS_D128} <= hit
    assert ties["wave"] > 20 and ties["split"] > 20


@pytest.mark.parametrize("case", TD.HANDOFF_CASES, ids=TD.onehot_id)
def test_handoff_cases(case):
    TD.check_handoff(case, REF, CPU)


@pytest.mark.parametrize("lens", TD.EMPTY_LENS)
@pytest.mark.parametrize("D", [128, 32])
def test_empty_rows_cases(D, lens):
    TD.check_empty(D, lens, REF, CPU)


def test_refusal_cases():
    TD.check_refused(REF, CPU)


@pytest.mark.parametrize("case", [(128, 8, 2, False, False), (128, 16, 1, True, False)], ids=TD.onehot_id)
def test_partials_cases(case):
    TD.check_partials(case, REF, CPU)


@pytest.mark.parametrize("M,Hq,ns", TD.MERGE_CASES)
def test_merge_linear_cases(M, Hq, ns):
    TD.check_merge_linear(M, Hq, ns, REF, CPU)
    ml, po, _ = TD.merge_case(M, Hq, ns, True)
    assert torch.isnan(po[~torch.isfinite(ml[..., 0])]).all()  # dead splits: NaN in o
    L = torch.where(torch.isfinite(ml[..., 0]), ml[..., 1], torch.zeros(())).sum(-1)
    assert set(L.unique().tolist()) <= {0.0, 16.0}


@pytest.mark.parametrize("case", TD.APPEND_CASES, ids=TD.append_id)
def test_rope_append_cases(case):
    D, Hq, Hkv, B, S, paged, use_slots = case
    TD.check_rope_append(case, REF, CPU)
    c = TD.append_case(case)
    assert int(c["pos"].min()) == 0 and int(c["pos"].max()) == (512 if paged else S) - 1
    assert torch.isnan(c["kc"]).any() and torch.isnan(c["vc"]).any()
    if B > 1000:
        assert B * (Hq + 2 * Hkv) * D // 16 > 1024 * 256  # a second grid-stride pass


@pytest.mark.parametrize("case", TD.GAUSS_CASES, ids=TD.gauss_id)
def test_gaussian_cases_and_model(case):
    """The plain fp32 reference, mxllm.ops.decode.decode_attention and the fp32 model of the documented
    algorithm all meet the bound the kernel is held to."""
    D, Hq, Hkv, paged = case
    TD.check_gauss(case, REF, CPU)
    c = TD.gauss_case(case)
    r64 = TD.gauss_reference(c, F64, D)
    assert_parity(TD.gauss_reference(c, F32, D).to(BF16).view(-1, D), r64.view(-1, D), TD.gauss_bound(D), name="model")
    # decode_attention (RoPE tables of a zero angle, the row at len - 1 re-appended: the cache is unchanged)
    B = len(TD.GAUSS_LENS)
    pos = c["lens"] - 1
    rows = c["kc"].shape[2]
    last = [TD.kv_place(c["bt"], rows, int(c["slots"][b]), int(pos[b])) for b in range(B)]
    qkv = torch.cat([c["q"].view(B, -1)] + [torch.stack([t[i0, :, r].reshape(-1) for i0, r in last]) for t in (c["kc"], c["vc"])], 1)
    kc, vc = c["kc"].clone(), c["vc"].clone()
    out = dops.decode_attention(qkv, torch.ones(768, D // 2), torch.zeros(768, D // 2), kc, vc, pos, c["slots"], Hq,
                                Hkv, D, 768, c["bt"])
    assert torch.equal(TD.bits(kc), TD.bits(c["kc"])) and torch.equal(TD.bits(vc), TD.bits(c["vc"]))
    assert_parity(out.view(-1, D), r64.view(-1, D), TD.gauss_bound(D), name="decode_attention")


def test_decode_constants_are_the_measured_ones():
    acc = TD.measure()
    assert set(acc) == {"DECODE_O_MFMA", "DECODE_O_F32"}
    for name, (rel, ab) in acc.items():
        _assert_measured(name, rel, ab)


# =========================================================================== decode: corruptions
GAUSS = (128, 8, 2, True)


def _gauss_norm(out, case=GAUSS):
    r64 = TD.gauss_reference(TD.gauss_case(case), F64, case[0])
    return max(_norm_ratio(out.view(3, -1)[b], r64[b]) for b in range(3))


def test_rejects_two_q_heads_of_a_group_swapped():
    """An O(1) error in two heads of one sequence.  With independent Gaussian queries the norm ratio of
    test_decode_kernels sees it as well (asserted: the ratio is far above 2e-2); the one-hot check names
    the two heads' columns."""
    def swap(b, o):
        o = o.clone()
        o[[1, 2]] = o[[2, 1]]
        return o

    bad = RefDecode(head_edit=lambda b, o: swap(b, o) if b == 1 else o)
    out = TD.run_attn(bad, TD.gauss_case(GAUSS), CPU, scale=1 / math.sqrt(128), max_len=640)
    assert _gauss_norm(out) > 2e-2
    with pytest.raises(AssertionError, match=r"columns 128\.\.383"):
        TD.check_onehot((128, 8, 2, False, False), bad, CPU)
    with pytest.raises(AssertionError):
        TD.check_gauss(GAUSS, bad, CPU)


def test_rejects_the_last_key_of_a_split_dropped():
    """Keys 255 and 511 (the last of a split) without their probability for ONE q-head, the one whose
    one-hot target is key 255 -- one column of the 16-head MFMA tile.  (Dropped for all eight heads the
    ratio of the 300- and 640-key rows is 0.03 to 0.04 at these inputs: that the old threshold does see.)"""
    case = (128, 8, 8, False, False)
    c = TD.onehot_case(case)
    heads = {h for b in range(len(c["lens_list"])) for h, ts in enumerate(c["targets"][b]) if ts[0] == 255}
    assert 4 in heads  # key 255 is the fifth candidate of every sequence longer than 256 keys

    def dropper(h):
        def drop(b, p):
            p = p.clone()
            for key in (255, 511):
                if p.shape[1] > key:
                    p[h, key] = 0
            return p
        return RefDecode(p_edit=drop)

    out = TD.run_attn(dropper(3), TD.gauss_case(GAUSS), CPU, scale=1 / math.sqrt(128), max_len=640)
    assert 1e-3 < _gauss_norm(out) < 2e-2  # test_decode_kernels' threshold accepts it (0.018 in the 300-key row)
    with pytest.raises(AssertionError):
        TD.check_gauss(GAUSS, dropper(3), CPU)
    with pytest.raises(AssertionError, match="columns 512"):
        TD.check_onehot(case, dropper(4), CPU)


def test_rejects_two_block_table_entries_exchanged():
    """Whole blocks of another position: an O(1) error that a norm ratio against a reference sees too --
    but the only paged test compared the paged kernel with the contiguous one, through the same kv_row."""
    def edit(bt):
        bt = bt.clone()
        bt[:, [0, 1]] = bt[:, [1, 0]]
        return bt

    bad = RefDecode(table_edit=edit)
    for case in [(128, 8, 2, True, False), (64, 8, 2, True, True)]:
        with pytest.raises(AssertionError):
            TD.check_onehot(case, bad, CPU)
    with pytest.raises(AssertionError):
        TD.check_gauss(GAUSS, bad, CPU)


def test_rejects_one_cache_row_outside_the_append_target_overwritten():
    case = (128, 8, 2, 5, 300, False, True)

    class Spill(RefDecode):
        def rope_append(self, qkv, cos, sin, pos, slots, kc, vc, Hq, Hkv, D, bt=None):
            q = super().rope_append(qkv, cos, sin, pos, slots, kc, vc, Hq, Hkv, D, bt)
            s, p = int(slots[2]), int(pos[2])
            kc[s, 1, (p + 1) % kc.shape[2]] = kc[s, 1, p]  # the row also lands one position later
            return q

    with pytest.raises(AssertionError, match="K cache outside the appended rows"):
        TD.check_rope_append(case, Spill(), CPU)


# =========================================================================== decode GEMMs: reference ops
def _asked(op, entry, x, w, ldy=0, **kw):
    """The refusal of the ops: whatever ``mxllm.ops.linear.sk_takes`` (the mirror of the launchers' one check)
    refuses, and 2-D rows with a unit inner stride, M >= 1."""
    rows = all(t.dim() == 2 and t.stride(1) == 1 for t in (x, w)) and x.shape[0] >= 1 and x.shape[1] == w.shape[1]
    if not (rows and sk_takes(entry, x.shape[0], w.shape[0], x.shape[1], x.stride(0), w.stride(0), ldy, **kw)):
        raise RuntimeError(f"{op}: the kernel does not take this call")


def _delta_kw(op, h, delta):
    if delta is None:
        return {}
    if delta.shape != h.shape or delta.stride(1) != 1:
        raise RuntimeError(f"{op}: delta must have h's shape")
    return dict(delta=1, ldd=delta.stride(0))


def _qkv_operands(h, gamma, cos, sin, pos, slots, kc, vc, Hkv, bt):
    """The tensor checks of skinny_qkv_rope (csrc/bindings.cpp sk_rope, sk_norm), on whatever device h is on."""
    def need(ok, what):
        if not ok:
            raise RuntimeError(f"skinny_qkv_rope: {what}")

    dev, (M, K) = h.device, h.shape
    for c in (kc, vc):
        need(c.device == dev and c.dtype == BF16 and c.dim() == 4 and c.is_contiguous(), "K and V pools must be "
             "contiguous bf16 [rows, Hkv, SEQ, D] on the query's device")
    need(kc.shape[3] == 128 and kc.shape[1] == Hkv, "the pools' heads and last dimension")
    need(vc.shape == kc.shape, "the K and V pools differ in shape")
    for t in (cos, sin):
        need(t.device == dev and t.dtype == F32 and t.dim() == 2 and t.is_contiguous() and t.shape[1] == 64,
             "cos / sin must be contiguous float32 [positions, 64] on h's device")
    for name, t in (("pos", pos), ("slots", slots)):
        need(t is not None or name == "slots", name)
        need(t is None or (t.device == dev and t.dtype == I32 and t.is_contiguous() and t.numel() == M),
             f"{name} must be a contiguous int32 [B] tensor on the query's device")
    if bt is not None:
        need(bt.dtype == I32 and bt.dim() == 2 and bt.is_contiguous(), "block_table int32 [slots, max_blocks]")
        need(kc.shape[2] % 256 == 0, "paged KV: the block size must be a multiple of 256 tokens")
    if gamma is not None:
        need(gamma.device == dev and gamma.dtype == BF16 and gamma.is_contiguous() and gamma.numel() == K,
             "gamma must be contiguous bf16 [K] on h's device")


class RefSkinny:
    """The contracts of the decode GEMMs in plain fp32 PyTorch (integers and selections: exact)."""

    def skinny_linear(self, x, w):
        _asked("skinny_linear", "plain", x, w, w.shape[0])
        return (x.float() @ w.float().t()).to(BF16)

    def skinny_linear_swiglu(self, x, w):
        F = w.shape[0] // 2
        _asked("skinny_linear_swiglu", "swiglu", x, w, F)
        gu = (x.float() @ w.float().t()).to(BF16).float()
        return (torch.nn.functional.silu(gu[:, :F]) * gu[:, F:]).to(BF16)

    def _norm(self, h, delta, gamma, eps):
        hb = (h.float() + delta.float()).to(BF16) if delta is not None else h
        hf = hb.float()
        return (hf * torch.rsqrt(hf.pow(2).mean(-1, keepdim=True) + eps) * gamma.float()).to(BF16), hb

    def skinny_norm_linear(self, h, delta, gamma, eps, w, swiglu):
        if gamma.numel() != h.shape[1]:
            raise RuntimeError("skinny_norm_linear: gamma")
        _asked("skinny_norm_linear", "norm", h, w, w.shape[0] // 2 if swiglu else w.shape[0], swiglu=swiglu,
               **_delta_kw("skinny_norm_linear", h, delta))
        xn, hb = self._norm(h, delta, gamma, eps)
        return (self.skinny_linear_swiglu(xn, w) if swiglu else self.skinny_linear(xn, w)), hb

    def skinny_qkv_rope(self, h, delta, gamma, eps, w, cos, sin, pos, slots, kc, vc, Hq, Hkv, bt=None):
        norm = gamma is not None
        _qkv_operands(h, gamma, cos, sin, pos, slots, kc, vc, Hkv, bt)
        _asked("skinny_qkv_rope", "rope", h, w, norm=norm, **(_delta_kw("skinny_qkv_rope", h, delta) if norm else {}),
               rope=dict(Hq=Hq, Hkv=Hkv, max_seq=kc.shape[2], bt=bt is not None, maxb=0 if bt is None else bt.shape[1]))
        xn, hb = self._norm(h, delta, gamma, eps) if norm else (h, h)
        qkv = (xn.float() @ w.float().t()).to(BF16)
        return REF.rope_append(qkv, cos, sin, pos, slots, kc, vc, Hq, Hkv, 128, bt), hb

    def w8_dequant(self, q, scale):
        return dequantize_e4m3(q, scale).to(BF16)

    def w8_linear(self, x, q, scale):
        if not sk_takes("w8", x.shape[0], q.shape[0], x.shape[1], x.stride(0), ldy=q.shape[0]):  # dequantise + GEMM
            return TS.w8_fallback_products(x, q, scale)[0].to(BF16)
        y32 = TS.w8_products(x, q, torch.ones_like(scale))[0] * scale.float()
        return y32.to(BF16)

    def quant_rows_e4m3(self, x):
        return TS.quant_rows_expected(x)


RS = RefSkinny()


# =========================================================================== decode GEMMs: the cases on the CPU
@pytest.mark.parametrize("kind", ["perm", "int"])
@pytest.mark.parametrize("M,N,K", [c for c in TS.LIN_CASES if c[0] in (1, 17, 32)])
def test_linear_cases(M, N, K, kind):
    TS.check_linear(kind, M, N, K, RS.skinny_linear, CPU)
    x, w, want, _ = TS.lin_expected(kind, M, N, K)
    if kind == "perm":
        assert (w.sum(1) == 1).all() and (w.abs().sum(1) == 1).all()
        xb = TS.bits(x)
        assert (xb == -32768).any() and (xb == 0).any()  # both zeros
        assert (x.float().abs() == TS.BF16_MAX).any() and (x.float().abs() == TS.BF16_TINY).any() and torch.isfinite(x).all()
    buf = TS.padded(x, 24, 3)
    assert torch.isnan(buf[:, K:]).all() and torch.isnan(buf[M:]).all()


def test_permutations_visit_every_k_position():
    for K in TS.LIN_K:
        pi = torch.cat([TS.perm_map(N, K) for N in TS.LIN_N])
        kq = K // 8
        assert set((pi % 64).tolist()) == set(range(64))                       # every position of a 64-k chunk
        assert set((pi // kq).tolist()) == set(range(8))                        # every wave's K part
        assert set(((pi % kq) // 64).tolist()) == set(range(kq // 64))          # every chunk of the batch and the tail
        assert set(TS.perm_map(4096, K).tolist()) == set(range(K)) or K > 4096
    assert torch.equal(TS.perm_map(1040, 512).unique(), torch.arange(512))      # N > K: repeats, every column


@pytest.mark.parametrize("M,N,K", TS.GAUSS_LIN_CASES)
def test_gaussian_linear_cases(M, N, K):
    TS.check_linear("gauss", M, N, K, RS.skinny_linear, CPU)


def test_linear_refusal_cases():
    TS.check_linear_refusals(RS.skinny_linear, CPU)
    TS.check_norm_refusals(RS.skinny_norm_linear, CPU)


@pytest.mark.parametrize("op", TS.RULE_CHECKS)
def test_refusals_by_rule_cases(op):
    """The reference ops refuse exactly what the launchers' check refuses: they ask its mirror."""
    TS.RULE_CHECKS[op](getattr(REF if op == "skinny_merge_linear" else RS, op), CPU)


def test_qkv_rope_operand_cases():
    TS.check_qkv_operands(RS.skinny_qkv_rope, CPU)
    assert len({m for _, m, _ in TS.qkv_bad_operands(CPU)}) == 7  # pos, slots, cos / sin, pools, block_table, gamma, delta


def test_channel_group_cases():
    """The child's cases on the CPU reference; the shapes keep the requested group count."""
    for nc, N in TS.NC_SHAPES.items():
        assert N % (16 * nc) == 0 and N // (16 * nc) >= 128
    TS.run_nc_cases(2, RS.skinny_linear, CPU)


@pytest.mark.parametrize("M,F,K", [c for c in TS.SWIGLU_CASES if c[0] in (1, 17)])
def test_swiglu_cases(M, F, K):
    TS.check_swiglu(M, F, K, RS.skinny_linear_swiglu, CPU)


@pytest.mark.parametrize("M,K,resid,swiglu", [c for c in TS.NORM_CASES if c[0] in (1, 4)])
def test_norm_linear_cases(M, K, resid, swiglu):
    TS.check_norm_linear(M, K, resid, swiglu, RS.skinny_norm_linear, CPU)
    assert M * K <= 32768


@pytest.mark.parametrize("case", TS.QKV_CASES, ids=TS.qkv_id)
def test_qkv_rope_cases(case):
    TS.check_qkv_rope(case, RS.skinny_qkv_rope, CPU)


def test_w8_dequant_case():
    TS.check_w8_dequant(RS.w8_dequant, CPU)


@pytest.mark.parametrize("kind", ["int", "gauss"])
@pytest.mark.parametrize("case", [c for c in TS.W8_CASES if c[1] * c[2] <= 40_000_000], ids=TS.w8_id)
def test_w8_linear_cases(case, kind):
    TS.check_w8_linear(kind, case[0], case[1], case[2], RS.w8_linear, CPU)


@pytest.mark.parametrize("M,N,K", TS.W8_FALLBACK)
def test_w8_fallback_cases(M, N, K):
    TS.check_w8_fallback(M, N, K, RS.w8_linear, RS.w8_dequant, CPU)
    x, q, scale = TS.w8_case("gauss", M, N, K)
    with pytest.raises(AssertionError):  # the weights' bf16 rounding is not within the decode kernel's bound
        assert_parity(RS.w8_linear(x, q, scale), TS.w8_products(x, q, scale)[1], P.W8_Y)


def test_w8_cases_reach_every_branch():
    """mx_w8a16_gemm's dispatch, restated: the case list names every branch."""
    def branch(M, N, K, force):
        if force == 4 and M <= 16 and N % 64 == 0 and N // 64 >= 128:
            return "four groups forced"
        if M <= 16 and N % 32 == 0 and ((force == 2 and N // 32 >= 128) or
                                         (not force and N // 32 >= 256 and (M >= 6 or (M >= 4 and K >= 16384)))):
            if force:
                return "two groups forced"
            return "two groups (6..16 tokens)" if M >= 6 else "two groups (4 tokens, K >= 16384)"
        return "one group" if M <= 16 else "two token blocks"

    for M, N, K, nc, name in TS.W8_CASES:
        assert branch(M, N, K, int(nc or 0)) == name and K % 512 == 0 and N % 16 == 0
    assert {c[4] for c in TS.W8_CASES} == {"one group", "two groups (6..16 tokens)", "two groups (4 tokens, K >= 16384)",
                                          "two groups forced", "four groups forced", "two token blocks"}
    assert {c[2] for c in TS.W8_CASES} >= {512, 4096, 4608}
    for M, N, K in TS.W8_FALLBACK:
        assert M > 32 or K % 512


def test_quantize_e4m3_emits_only_the_238_codes():
    """The contract fp8_gemm.hip's four-instruction decode rests on: no zero, subnormal or NaN code."""
    from mxllm.serve.quant import quantize_e4m3

    g = torch.Generator().manual_seed(4)
    w = torch.randn(8, 256, generator=g)
    w[0, :8] = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 1e-38, -1e-38, 1e-45, -1e-45])
    w[1] = 0.0                                  # an all-zero row
    w[2, 0], w[2, 1] = 1e30, -1e30              # one huge outlier: everything else far below 2^-6 of it
    w[3, :4] = torch.tensor([w[3].abs().max() * 2.0 ** -7, -w[3].abs().max() * 2.0 ** -9, 0.0, w[3].abs().max() * 2.0 ** -6])
    w[4] = w[4].abs().max()                     # +max everywhere
    w[5] = -w[5].abs().max()
    w[6] *= 1e-20
    w[7] *= 1e20
    allowed = set(TS.emittable_codes().tolist())
    assert len(allowed) == 238
    for t in (w, w.to(BF16)):
        q, s = quantize_e4m3(t)
        assert set(q.flatten().tolist()) <= allowed
        assert torch.isfinite(s).all() and (s > 0).all()
        assert (q[4] == 0x7E).all() and (q[5] == 0xFE).all()  # +-448
    assert set(quantize_e4m3(torch.randn(64, 512, generator=g))[0].flatten().tolist()) <= allowed


@pytest.mark.parametrize("K", TS.QUANT_K)
def test_quant_rows_cases(K):
    """The tie facts: 448 * fl(1 / 448) == 1 in fp32, the tie row's scale is exactly 1 and its ties round to even."""
    assert TS.inv448_is_exact()
    q = TS.check_quant_rows(K, RS.quant_rows_e4m3, CPU)
    x = TS.quant_rows_input(K)
    _, sc = TS.quant_rows_expected(x)
    assert sc[2].item() == 1.0 and not q[1].any()
    dec = q[2].view(torch.float8_e4m3fn).float()
    for v, want in ((1.0625, 1.0), (1.1875, 1.25), (-1.0625, -1.0), (-1.1875, -1.25), (17.0, 16.0), (19.0, 20.0),
                    (1.5 * 2.0 ** -9, 2.0 ** -8), (2.0 ** -10, 0.0)):
        hit = x[2].float() == v
        assert hit.any() or K == 8
        assert (dec[hit] == want).all(), (v, want)
    buf = TS.padded(x, 16, 1, fill=3e38)
    assert (buf[:, K:].float() > 1e38).all()


def test_gemm_constants_are_the_measured_ones():
    acc = TS.measure()
    assert set(acc) == {"SKINNY_Y", "W8_Y", "W8_DEQ_Y"}
    for name, (rel, ab) in acc.items():
        _assert_measured(name, rel, ab)


# =========================================================================== decode GEMMs: corruptions
def rel_err(a, b):  # tests/test_kernels_gpu.py
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def test_rejects_two_halves_of_a_k_chunk_swapped_in_x():
    """One workgroup (16 channels) reads k 8..15 and 0..7 of one 64-k chunk of x in exchanged order."""
    def bad(x, w):
        y = RS.skinny_linear(x, w).clone()
        xs = x.clone()
        xs[:, 64:72], xs[:, 72:80] = x[:, 72:80], x[:, 64:72]
        n0 = 16 * ((w.shape[0] // 16) // 2)
        y[:, n0:n0 + 16] = RS.skinny_linear(xs, w[n0:n0 + 16])
        return y

    y, r64 = TS.check_linear("gauss", 16, 4096, 4608, RS.skinny_linear, CPU)
    x, w, _, _ = TS.lin_expected("gauss", 16, 4096, 4608)
    assert 1e-4 < rel_err(bad(x, w), r64) < 1e-2  # test_skinny_linear_vs_fp32's threshold accepts it
    for kind in ("gauss", "int"):
        with pytest.raises(AssertionError):
            TS.check_linear(kind, 16, 4096, 4608, bad, CPU)
    hit = [N for N in TS.LIN_N if N >= 1040 and ((TS.perm_map(N, 4608)[16 * (N // 32):16 * (N // 32) + 16] - 64) // 16 == 0).any()]
    for N in hit:  # a permutation row sees it when its 1.0 lies in the chunk
        with pytest.raises(AssertionError):
            TS.check_linear("perm", 16, N, 4608, bad, CPU)


def test_rejects_a_scale_group_taken_from_its_neighbour():
    def bad(x, q, scale):
        s = scale.clone()
        s[40:44] = scale[44:48]
        return RS.w8_linear(x, q, s)

    M, N, K = 6, 8192, 512  # N of test_w8_linear_wide
    x, q, scale = TS.w8_case("gauss", M, N, K)
    assert 1e-4 < rel_err(bad(x, q, scale), TS.w8_products(x, q, scale)[1]) < 1e-2  # its threshold accepts it
    with pytest.raises(AssertionError, match=r"columns 4[0-3]\.\.4[0-3]"):
        TS.check_w8_linear("int", M, N, K, bad, CPU)


def test_rejects_gate_and_up_rows_of_one_block_exchanged():
    """One workgroup's 8 gate rows and 8 up rows exchanged, for one of its tokens (one lane of the
    lane ^ 32 shuffle) -- with all tokens the ratio at F = 1024 is above the old threshold."""
    M, F, K = 17, 1024, 4608

    def bad(x, w):
        y = RS.skinny_linear_swiglu(x, w).clone()
        sw = torch.cat([w[F + 64:F + 72], w[64:72]])
        y[3, 64:72] = RS.skinny_linear_swiglu(x[3:4], sw)[0]
        return y

    y, r64 = TS.check_swiglu(M, F, K, RS.skinny_linear_swiglu, CPU)
    x = TS.finite_x(M, K, 3400 + 64 * M + F + K, extremes=False)
    assert 1e-4 < rel_err(bad(x, TS.perm_weight(2 * F, K)), r64) < 1e-2
    with pytest.raises(AssertionError, match=r"worst at \(3, (6[4-9]|7[01])\)"):
        TS.check_swiglu(M, F, K, bad, CPU)
