"""The exact and per-element MFMA tests (tests/test_mfma_exact_gpu.py, tests/test_attention_strict_gpu.py)
on the CPU: every input condition they rest on, the reference ops through the very same builders and
assertions (a wrong test fails here, not on the GPU), and four localized corruptions that the norm
thresholds of tests/test_gemm8_gpu.py and tests/test_kernels_gpu.py accept and these checks reject."""
import math

import pytest
import torch

from tests import _parity as P
from tests import test_attention_strict_gpu as TA
from tests import test_mfma_exact_gpu as TE
from tests._parity import assert_exact, assert_parity

BF16, F32 = torch.bfloat16, torch.float32
CPU = torch.device("cpu")


# --------------------------------------------------------------------------- reference ops
def _ab(a, a_kc, b, b_kc):
    return (a.float() if a_kc else a.float().t()), (b.float().t() if b_kc else b.float())


def ref_gemm8(a, a_kc, b, b_kc, out, beta, alpha_t, alpha):
    """mx_gemm8's contract in plain fp32 PyTorch (integers: exact), its shape refusals included."""
    A, B = _ab(a, a_kc, b, b_kc)
    if A.shape[0] % 256 or B.shape[1] % 256 or ((a_kc or b_kc) and A.shape[1] % 64):
        return False
    acc = (A @ B) * (alpha * (1.0 if alpha_t is None else float(alpha_t)))
    out.copy_((acc + out.float()) if beta else acc)
    return True


def ref_gemm8_tail(a, a_kc, b, b_kc, out, at, rows):
    A, B = _ab(a, a_kc, b, b_kc)
    lim = A.shape[0] if rows else B.shape[1]
    if A.shape[1] < 128 or at <= 0 or at >= lim or at % 256 or (lim - at) % 256:
        return False
    return ref_gemm8(a, a_kc, b, b_kc, out, 0.0, None, 1.0)


def ref_lora_xwt(kern):
    def run(x, v, out, alpha, rows):
        T, K = x.shape
        path = TE.xwt_path(kern, T, K)
        if path == "refused":
            raise RuntimeError("lora_xwt: T % 64")
        y = alpha * (x.float() @ v.float().t())
        if path == "tile":
            y[:, rows:] = 0
        out[:, :v.shape[0]] = y.to(out.dtype)
    return run


def ref_lora_grads(x, dy, g, st, ga, gb, splits, r, acc):
    R = len(splits) * r
    da = g[:, :R].float().t() @ x.float()
    ga.copy_(da + ga.float() if acc else da)
    off = 0
    for i, ni in enumerate(splits):
        blk = (slice(off, off + ni), slice(i * r, (i + 1) * r))
        db = dy[:, off:off + ni].float().t() @ st[:, i * r:(i + 1) * r].float()
        gb[blk] = (db + gb[blk].float() if acc else db).to(gb.dtype)
        off += ni


def model_fwd(q, k, v, causal, scale):
    """The fp32 model of attn_fwd (tests/test_attention_strict_gpu.py) with the kernel's output layout."""
    o, lse = TA.attn_fwd_model(q, k, v, causal, scale, F32, True)
    return TA.tok(o).to(BF16), lse


def model_bwd(do, q, k, v, o, lse, causal, scale, mode):
    B, Hq, S, D = q.shape
    oh = o.view(B, S, Hq, D).transpose(1, 2)
    return TA.attn_bwd_model(do, q, k, v, oh, lse, causal, scale, F32, True)


# --------------------------------------------------------------------------- the exact cases on the CPU
@pytest.mark.parametrize("case", TE.GEMM_CASES, ids=TE.gemm_id)
def test_gemm_cases_hold_their_conditions(case):
    """< 2^24, >= 10 % of the bf16 outputs need rounding at K >= 640 (both asserted inside), poison in
    every pad column and in the rows past K of a token-major operand."""
    (a_kc, b_kc), (M, N), K = case
    TE.check_gemm(case, ref_gemm8, CPU, TE.VARIANTS + TE.ALPHA_VARIANTS)
    c = TE.gemm_case(case)
    for buf, shape, kc in ((c["a_buf"], c["a_shape"], a_kc), (c["b_buf"], c["b_shape"], b_kc)):
        assert (buf[:, shape[1]:] == TE.POISON).all() and buf.shape[1] > shape[1]
        if not kc:
            assert buf.shape[0] >= (K + 63) // 64 * 64 + 64 and (buf[K:] == TE.POISON).all()
        assert TE.view(buf, shape).abs().max() <= 3


@pytest.mark.parametrize("case", TE.PERSIST_CASES, ids=TE.gemm_id)
def test_persistent_gemm_cases_hold_their_conditions(case):
    TE.check_gemm(case, ref_gemm8, CPU, TE.VARIANTS)


@pytest.mark.parametrize("rows", [False, True])
@pytest.mark.parametrize("case", TE.TAIL_CASES, ids=TE.gemm_id)
def test_tail_gemm_cases(case, rows):
    TE.check_gemm_tail(case, rows, ref_gemm8_tail, CPU)
    tiles = case[2] // 64
    assert tiles in (1, 2, 11)  # declined; an even and an odd K-tile count to split


@pytest.mark.parametrize("rows", [16, 32, 48, 64])
@pytest.mark.parametrize("kern", ["lds", "reg", "tile"])
@pytest.mark.parametrize("T,K", TE.XWT_SHAPES)
def test_lora_xwt_cases(T, K, kern, rows):
    TE.check_lora_xwt(T, K, kern, rows, ref_lora_xwt(kern), CPU)


@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("K,splits,r", TE.GRADS_CONFIGS)
def test_lora_grads_cases(K, splits, r, acc):
    TE.check_lora_grads(K, splits, r, acc, ref_lora_grads, CPU)


@pytest.mark.parametrize("case", TE.ONEHOT_CASES, ids=TA.case_id)
def test_onehot_cases_hold_their_conditions(case):
    """The 300-unit gap (asserted inside), pi inside the causal mask with every third query on its
    diagonal key, q really the chosen key's code -- and the fp32 model is exactly one-hot."""
    B, Hq, Hkv, S, Sk, D, _ = case
    q, k, pi, v_int, _, do = TE.onehot_case(case)
    i = torch.arange(S).view(1, 1, S)
    assert (pi >= 0).all() and (pi <= i + Sk - S).all()
    assert (pi[:, :, ::3] == (i + Sk - S)[:, :, ::3]).all()
    kk = k.repeat_interleave(Hq // Hkv, 1)
    assert torch.equal(q, torch.gather(kk, 2, pi.unsqueeze(-1).expand(-1, -1, -1, D)))
    assert v_int.abs().max() <= 4 and do.abs().max() <= 2 and set(k.abs().unique().tolist()) == {TE.onehot_c(D)}
    TE.check_onehot(case, model_fwd, model_bwd, CPU, modes=(3,))


def test_onehot_reference_attention_is_bitwise():
    """mxllm.ops.reference.attention at one-hot inputs: O = V[pi] bit for bit (D = 32, 64, 128; Sk = S, Sk > S)."""
    from mxllm.ops.reference import attention

    for case in [(2, 4, 1, 65, 65, 32, True), (2, 4, 1, 129, 129, 64, True), (1, 8, 2, 257, 257, 128, True),
                 (2, 2, 2, 65, 200, 128, True)]:
        q, k, _, _, v, _ = TE.onehot_case(case)
        o = attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), causal=True)
        assert_exact(o.reshape(case[0], case[3], -1), TE.onehot_expected(case, v)[0], TA.case_id(case))


@pytest.mark.parametrize("case", TA.ATTN_CASES + [TA.DS_BUDGET_CASE], ids=TA.case_id)
def test_attention_model_meets_its_own_bound(case):
    TA.check_attention(case, model_fwd, model_bwd, CPU, modes=(3,))


def test_attention_constants_are_the_measured_ones():
    acc = TA.measure()
    assert set(acc) == {"ATTN_O", "ATTN_LSE", "ATTN_DQ", "ATTN_DK", "ATTN_DV", "ATTN_ROPE_DQKV"}
    for name, (rel, ab) in acc.items():
        assert getattr(P, name + "_MEASURED") == (float(f"{rel:.3g}"), float(f"{ab:.3g}")), name


def test_attention_cases_cover_the_list():
    assert len(TA.ATTN_CASES) == 2 + 18 + 7 and len(set(TA.ATTN_CASES)) == len(TA.ATTN_CASES)
    assert len(TA.ROPE_CASES) == 9  # S = Sk, D = 128
    assert {h for _, h in TA.HPW_CASES} == {1, 2, 4}


# --------------------------------------------------------------------------- assert_exact
def test_assert_exact_message_names_the_box():
    want = torch.arange(64 * 48, dtype=F32).view(64, 48)
    assert_exact(want.clone(), want)
    bad = want.clone()
    bad[16:32, 32:48] += 1
    bad[20, 40] += 100
    with pytest.raises(AssertionError) as e:
        assert_exact(bad, want, "c")
    msg = str(e.value)
    assert "c: 256 of 3072 elements differ" in msg and "first at (16, 32)" in msg and "worst at (20, 40)" in msg
    assert "rows 16..31, columns 32..47" in msg
    assert f"out {bad[20, 40].item():.9g}, expected {want[20, 40].item():.9g}" in msg
    with pytest.raises(AssertionError):
        assert_exact(want.to(BF16), want)  # dtype
    with pytest.raises(AssertionError):
        assert_exact(want[:, :-1], want)  # shape
    nan = want.clone()
    nan[3, 5] = float("nan")
    with pytest.raises(AssertionError, match=r"1 of 3072 .*first at \(3, 5\)"):
        assert_exact(nan, want)
    assert_exact(torch.tensor([0.0, -0.0]), torch.tensor([-0.0, 0.0]))  # dQ = dK = 0 of either sign


# --------------------------------------------------------------------------- the four corruptions
def _norm_ratio(out, ref):
    return ((out.double() - ref.double()).norm() / ref.double().norm()).item()


def test_rejects_one_k_tile_dropped_from_one_fragment():
    """One 64-deep K-tile's contribution missing from one 16 x 16 fragment of a 512 x 768 product."""
    case = ((True, True), (512, 768), 640)
    c = TE.gemm_case(case)
    ref, want = TE.gemm_expected(c, False, 0.0, 1.0)
    A, B = TE.view(c["a_buf"], c["a_shape"]).double(), TE.view(c["b_buf"], c["b_shape"]).double().t()
    bad = ref.clone()
    bad[272:288, 400:416] -= A[272:288, 128:192] @ B[128:192, 400:416]
    bad = bad.to(F32).to(BF16)
    assert _norm_ratio(bad, ref) < 5e-3  # tests/test_gemm8_gpu.py's bf16 threshold accepts it
    with pytest.raises(AssertionError, match=r"rows 272\.\.287, columns 400\.\.415"):
        assert_exact(bad, want, "c")


def _o64(case, edit):
    """fp64 O [B,S,Hq,D] of a real-valued case with ``edit(p)`` applied to the probabilities, as bf16."""
    q, k, v, _ = TA.attn_inputs(case)
    G = case[1] // case[2]
    x, vis = TA._scores(q, k, case[6], 1.0 / math.sqrt(case[5]), torch.float64)
    p = torch.softmax(x.masked_fill(~vis, float("-inf")) / TA.LOG2E, -1)
    o = edit(p) @ v.double().repeat_interleave(G, 1)
    return o.transpose(1, 2)


CORRUPT_CASE = (1, 8, 2, 257, 257, 128, True)


def test_rejects_two_adjacent_keys_swapped_for_one_query():
    ref = _o64(CORRUPT_CASE, lambda p: p)
    assert_parity(ref.to(BF16), ref, P.ATTN_O)

    def swap(p):
        p = p.clone()
        j = int(p[0, 3, 200].argmax())
        j = j if j < 200 else j - 1
        p[0, 3, 200, [j, j + 1]] = p[0, 3, 200, [j + 1, j]]
        return p

    bad = _o64(CORRUPT_CASE, swap).to(BF16)
    assert _norm_ratio(bad, ref) < 2e-2  # tests/test_kernels_gpu.py's forward threshold accepts it
    with pytest.raises(AssertionError, match=r"worst at \(0, 200, 3, "):
        assert_parity(bad, ref, P.ATTN_O, name="O")


def test_rejects_the_diagonal_key_masked_for_one_row_per_tile():
    ref = _o64(CORRUPT_CASE, lambda p: p)
    rows = [63, 127, 191, 255]  # the last row of every 64-row query tile

    def mask(p):
        p = p.clone()
        for i in rows:
            p[:, :, i, i] = 0
        return p / p.sum(-1, keepdim=True)

    bad = _o64(CORRUPT_CASE, mask).to(BF16)
    assert _norm_ratio(bad, ref) < 2e-2
    with pytest.raises(AssertionError) as e:
        assert_parity(bad, ref, P.ATTN_O, name="O")
    assert int(str(e.value).split("first at (0, ")[1].split(",")[0]) == 63


def test_rejects_rows_past_k_read_from_the_same_allocation():
    """A token-major operand read to the end of its last 64-row K-tile instead of to row K: the poison
    rows behind row K are in the same allocation, so only the operand's range keeps them out."""
    case = ((False, False), (256, 256), 100)

    def overread(a, a_kc, b, b_kc, out, beta, alpha_t, alpha):
        K, M = a.shape
        a = a.as_strided(((K + 63) // 64 * 64, M), a.stride(), a.storage_offset())
        b = torch.cat([b, torch.zeros(a.shape[0] - K, b.shape[1], dtype=b.dtype)])
        b[K:, 7] = 1
        return ref_gemm8(a, a_kc, b, b_kc, out, beta, alpha_t, alpha)

    with pytest.raises(AssertionError, match=r"columns 7\.\.7"):
        TE.check_gemm(case, overread, CPU, TE.VARIANTS[:1])


def test_rejects_one_pad_column_overwritten():
    """A store that spills into the first pad column of the output: the product itself is right (any
    norm of it passes), the sentinel check of every exact GEMM case fails."""
    case = ((False, False), (256, 256), 100)

    def spill(a, a_kc, b, b_kc, out, beta, alpha_t, alpha):
        ok = ref_gemm8(a, a_kc, b, b_kc, out, beta, alpha_t, alpha)
        out.as_strided((out.shape[0], 1), (out.stride(0), 1), out.storage_offset() + out.shape[1])[5:21] = 1.0
        return ok

    TE.check_gemm(case, ref_gemm8, CPU, TE.VARIANTS)
    with pytest.raises(AssertionError, match="output pad columns written"):
        TE.check_gemm(case, spill, CPU, TE.VARIANTS)
