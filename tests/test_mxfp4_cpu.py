"""MXFP4 projection weights without a GPU: the quantiser's properties (mxllm/serve/quant.py), the model
quantiser and the serving engine on the CPU path, the refusals, and the checks of tests/test_mxfp4_gpu.py
run with the Python reference in place of the HIP ops (their inputs are valid, the reference passes)."""
import pytest
import torch

from mxllm.models import Llama, get_config
from mxllm.models.llama import FusedLinear
from mxllm.serve import quant
from mxllm.serve.engine import Engine
from mxllm.serve.quant import MXFP4_GRID, W4Linear, dequantize_mxfp4, quantize_mxfp4, quantize_model_mxfp4_
from tests import _mxfp4 as X
from tests import test_mxfp4_gpu as G

BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
CPU = torch.device("cpu")
GRID = torch.tensor(MXFP4_GRID)


def block(vals, top=4.0):
    """One block [1, 32]: ``top`` first (it fixes the scale: 4 -> e = 0), then ``vals``, then zeros."""
    t = torch.zeros(1, 32)
    t[0, 0] = top
    t[0, 1:1 + len(vals)] = torch.tensor(vals, dtype=F32)
    return t


def nibbles(codes):
    return torch.stack((codes & 0xF, codes >> 4), -1).reshape(codes.shape[0], -1)


def rows(seed=0, N=48, K=256):
    """Gaussian rows, row r scaled by 2^(r - 24), with exact zeros, a zero block and -0.0."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, K, generator=g) * torch.exp2(torch.arange(N, dtype=F32) - 24)[:, None]
    w[torch.rand(N, K, generator=g) < 0.05] = 0.0
    w[2, 32:64] = 0.0
    w[3, 5] = -0.0
    return w


# =========================================================================== quantiser properties
def test_every_code_round_trips():
    code = torch.arange(16).repeat(2)[None, :]          # one block: every code twice
    code[0, 8] = 0                                       # (a sign bit on magnitude 0 is never emitted)
    code[0, 24] = 0
    for byte in (1, 100, 127, 200, 252):
        codes, scales = X.pack(code), torch.tensor([[byte]], dtype=U8)
        w = dequantize_mxfp4(codes, scales)
        assert float(w.abs().max()) == 6.0 * 2.0 ** (byte - 127)
        c2, s2 = quantize_mxfp4(w)
        assert torch.equal(c2, codes) and torch.equal(s2, scales), byte


def test_ties_go_to_the_even_code():
    ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    want = [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0]
    for sign in (1.0, -1.0):
        for e in (-20, 0, 9):
            t = block([sign * v for v in ties]) * 2.0 ** e
            codes, scales = quantize_mxfp4(t)
            assert int(scales[0, 0]) == 127 + e
            got = dequantize_mxfp4(codes, scales)[0, 1:8] / 2.0 ** e
            assert got.tolist() == [sign * v if v else 0.0 for v in want], (sign, e, got)
    # just off a tie: to the nearer neighbour
    eps = 2.0 ** -20
    t = block([0.25 + eps, 0.75 - eps, 1.25 + eps, 2.5 - eps, 5.0 + eps])
    assert dequantize_mxfp4(*quantize_mxfp4(t))[0, 1:6].tolist() == [0.5, 0.5, 1.5, 2.0, 6.0]


def test_saturation_above_six():
    for top in (6.0, 6.5, 7.0, 7.999):
        for e in (-3, 0, 5):
            t = block([-top, 5.5, 4.9], top=top) * 2.0 ** e
            codes, scales = quantize_mxfp4(t)
            assert int(scales[0, 0]) == 127 + e  # amax / 2^e in [4, 8): floor(log2 amax) - 2 = e
            assert (dequantize_mxfp4(codes, scales)[0, :4] / 2.0 ** e).tolist() == [6.0, -6.0, 6.0, 4.0]


def test_zero_block_and_no_negative_zero():
    w = rows()
    codes, scales = quantize_mxfp4(w)
    assert int(scales[2, 1]) == 127 and int(codes[2, 16:32].max()) == 0
    nib = nibbles(codes)
    assert not bool((nib == 8).any())  # sign bit only on a non-zero magnitude
    small = torch.tensor([[4.0, -0.2, -0.0, 0.2] + [0.0] * 28])
    assert nibbles(quantize_mxfp4(small)[0])[0, :4].tolist() == [6, 0, 0, 0]
    z = quantize_mxfp4(torch.zeros(3, 64))
    assert bool((z[0] == 0).all()) and bool((z[1] == 127).all())


def test_scale_bytes_stay_inside_1_254():
    big, tiny = torch.finfo(F32).max, 2.0 ** -149
    w = torch.stack([block([1.0], top=big)[0], block([tiny], top=tiny)[0], block([2.0 ** -126], top=2.0 ** -120)[0],
                     block([], top=2.0 ** -127)[0]])
    codes, scales = quantize_mxfp4(w)
    assert scales[:, 0].tolist() == [252, 1, 5, 1]  # e = 125; clamped at -126; -122; clamped (f32 subnormal)
    w = rows(1, 64, 512) * 2.0 ** 60
    for t in (w, w * 2.0 ** -150, rows(2)):
        s = quantize_mxfp4(t)[1]
        assert 1 <= int(s.min()) and int(s.max()) <= 254
    with pytest.raises(ValueError):
        quantize_mxfp4(torch.zeros(4, 48))


def test_quantiser_is_idempotent_and_its_output_is_bf16():
    for seed in range(3):
        codes, scales = quantize_mxfp4(rows(seed))
        dq = dequantize_mxfp4(codes, scales)
        assert dq.dtype == F32 and torch.equal(dq, dq.to(BF16).float())
        c2, s2 = quantize_mxfp4(dq)
        assert torch.equal(c2, codes) and torch.equal(s2, scales)
        c3, s3 = quantize_mxfp4(dq.to(BF16))  # ... from a bf16 weight as well
        assert torch.equal(c3, codes) and torch.equal(s3, scales)


def test_error_bound_per_element():
    """Derived, not measured: the grid's spacing is 0.5 on [0, 2], 1 on [2, 4], 2 on [4, 6], so rounding to
    nearest is off by at most half of it; a saturated value lies in (6, 8) 2^e."""
    w = rows(4, 64, 1024)
    codes, scales = quantize_mxfp4(w)
    dq = dequantize_mxfp4(codes, scales).double()
    s = torch.exp2(scales.double() - 127).repeat_interleave(32, 1)
    v, err = w.double().abs() / s, (w.double() - dq).abs() / s
    live = torch.ones_like(v, dtype=torch.bool)
    live[2, 32:64] = False  # the zero block
    assert float(v.max()) < 8 and bool((v[live].view(-1, 32).amax(-1) >= 4).all())
    for lo, hi, lim in ((0, 2, 0.25), (2, 4, 0.5), (4, 6, 1.0)):
        sel = (v >= lo) & ((v < hi) if hi < 6 else (v <= hi))
        assert int(sel.sum()) > 100 and float(err[sel].max()) <= lim, (lo, hi)
    sat = v > 6
    assert 0.005 < float(sat.double().mean()) < 0.05 and float(err[sat].max()) < 2
    assert bool((dq[sat].abs() / s[sat] == 6).all())
    assert bool((torch.sign(dq) * torch.sign(w.double()) >= 0).all())


def test_packing_is_low_nibble_first():
    t = block([0.5, -1.0, 6.0])
    codes, _ = quantize_mxfp4(t)
    assert codes[0, :2].tolist() == [6 | (1 << 4), (2 | 8) | (7 << 4)]
    if hasattr(torch, "float4_e2m1fn_x2"):
        assert codes.view(torch.float4_e2m1fn_x2).view(U8).data_ptr() == codes.data_ptr()


# =========================================================================== model level
def _greedy(eng, prompt, n=8):
    return eng.generate([prompt], max_new_tokens=n, temperature=0.0)[0]


def test_model_engine_is_bitwise_the_dequantised_bf16_model():
    cfg = get_config("tiny-d128")
    m4, m16 = X.quantized_pair(cfg, CPU, seed=5)
    assert all(isinstance(getattr(l, n), W4Linear) for l in m4.layers for n in ("wqkv", "wo", "wgu", "wd"))
    assert isinstance(m4.layers[0].wqkv.codes, torch.Tensor) and m4.layers[0].wqkv.codes.dtype == U8
    prompt = list(range(3, 40))
    e4, e16 = (Engine(m, max_batch=2, max_seq=128) for m in (m4, m16))
    assert torch.equal(e4.prefill(0, prompt), e16.prefill(0, prompt))
    assert _greedy(e4, prompt) == _greedy(e16, prompt) and len(_greedy(e4, prompt)) == 8


def test_model_engine_with_one_request_on_an_adapter():
    from tests import _lora_serve as L

    cfg = get_config("tiny-d128")
    ad = L.random_adapter(cfg, 8, 5)
    m4, m16 = X.quantized_pair(cfg, CPU, seed=6)
    prompt = [5, 9, 77, 1, 300, 12, 44]
    engs = [Engine(m, max_batch=2, max_seq=128, max_adapters=1) for m in (m4, m16)]
    for e in engs:
        e.load_adapter("a", ad)
    la = [e.prefill_batch([0, 1], [prompt, prompt], ["a", None]) for e in engs]
    assert torch.equal(la[0], la[1])
    assert not torch.equal(la[0][0], la[0][1])  # the adapter is applied to its row alone
    assert torch.equal(la[0][1], Engine(m4, max_batch=2, max_seq=128).prefill(0, prompt))
    outs = [e.generate([prompt, prompt], max_new_tokens=8, adapters=["a", None]) for e in engs]
    assert outs[0] == outs[1] and [len(o) for o in outs[0]] == [8, 8]


def test_bytes_saved_and_merged_lora():
    cfg = get_config("tiny-d128")
    m = Llama(cfg, seed=3, lora_r=8).eval()
    n = sum(getattr(l, p).weight.numel() for l in m.layers for p in ("wqkv", "wo", "wgu", "wd"))
    saved = quantize_model_mxfp4_(m)
    assert saved == 2 * n - n // 2 - n // 32
    assert isinstance(m.head_weight, torch.Tensor) and m.head_weight.dtype == BF16 and m.tok_emb.dtype == BF16


# =========================================================================== refusals and the interface
def test_model_quantiser_leaves_k_not_multiple_of_32_in_bf16():
    cfg = get_config("tiny").replace(ffn=528)  # wd: K = 528 = 16.5 x 32
    m = Llama(cfg, seed=1).eval()
    quantize_model_mxfp4_(m)
    for layer in m.layers:
        assert type(layer.wd) is FusedLinear and layer.wd.weight.dtype == BF16
        assert all(isinstance(getattr(layer, n), W4Linear) for n in ("wqkv", "wo", "wgu"))
    assert len(Engine(m, max_batch=1, max_seq=64).generate([[1, 2, 3]], max_new_tokens=3)[0]) == 3


def test_w4linear_refuses_scale_bytes_0_and_255():
    codes, scales = quantize_mxfp4(rows(7))
    W4Linear(codes=codes, scales=scales)
    for byte in (0, 255):
        s = scales.clone()
        s[5, 3] = byte
        with pytest.raises(ValueError):
            W4Linear(codes=codes, scales=s)
    with pytest.raises(ValueError):
        W4Linear(codes=codes, scales=scales[:, :4])
    with pytest.raises(ValueError):
        W4Linear(codes=codes.to(torch.int32), scales=scales)
    with pytest.raises(ValueError):
        W4Linear(torch.zeros(4, 32), codes=codes, scales=scales)


def test_server_and_local_take_weights_mxfp4(monkeypatch):
    from mxllm.serve import server

    assert server.parse_args(["--weights", "mxfp4"]).weights == "mxfp4"
    monkeypatch.setenv("MXLLM_ENGINE_WEIGHTS", "mxfp4")
    assert server.parse_args([]).weights == "mxfp4"
    eng, _ = server.build_default("tiny", "cpu", max_batch=2, max_seq=64, weights="mxfp4")
    assert isinstance(eng.model.layers[0].wgu, W4Linear)
    assert len(eng.generate([[1, 2, 3]], max_new_tokens=3)[0]) == 3


def test_module_passes_its_stream_m_to_the_op(monkeypatch):
    """On the native path W4Linear.forward is one w4_linear call with aligned rows and quant.STREAM_M."""
    seen = []

    class Ops:
        def w4_linear(self, x, codes, scales, stream_m):
            seen.append((x.stride(), stream_m))
            return X.reference_linear(x, codes, scales)

    monkeypatch.setattr(quant, "use_native", lambda t: True)
    monkeypatch.setattr(quant, "native", lambda: Ops())
    monkeypatch.setattr(quant, "STREAM_M", 96)
    lin = W4Linear(rows(8))
    x = torch.randn(2, 3, 260).to(BF16)[..., :256]  # row stride 260: not 16-B aligned
    y = lin(x)
    assert y.shape == (2, 3, 48) and seen == [((256, 1), 96)]
    monkeypatch.undo()
    assert torch.equal(y, lin(x)) and quant.STREAM_M >= 32


# =========================================================================== the GPU checks, on the reference
def test_reference_passes_every_code_check():
    X.check_every_code(X.reference_dequant, CPU)


@pytest.mark.parametrize("kind", ["int", "gauss"])
@pytest.mark.parametrize("case", G.W4_CASES + [c + ("", "") for c in G.W4_PASSES], ids=G.w4_id)
def test_reference_passes_linear_checks(case, kind):
    M, N, K = case[:3]
    X.check_linear(kind, M, N, K, X.reference_linear, CPU, G.W4_Y)


@pytest.mark.parametrize("M,N,K", G.W4_FALLBACK)
def test_reference_passes_fallback_check(M, N, K):
    X.check_fallback(M, N, K, X.reference_linear, X.reference_dequant, CPU, G.W4_DEQ_Y)


def test_cases_name_their_launcher_branch():
    """The branch written beside each case is the one the launcher's rules give (csrc/kernels/w4_args.h
    w4_waves, mxfp4_gemm.hip w4_groups with its defaults)."""
    for M, N, K, nc, branch in G.W4_CASES:
        nw = 8 if K % 1024 == 0 else 4
        assert K % 512 == 0 and N % 16 == 0 and 1 <= M <= 32
        assert branch.startswith(f"<{1 if M <= 16 else 2}, {nw}, "), (M, N, K, branch)
        if nc:
            assert N % (16 * int(nc)) == 0 and N // (16 * int(nc)) >= 128 and branch.endswith(f"{nc}>")
    branches = {b for *_, b in G.W4_CASES}
    assert branches == {f"<{mb}, {nw}, {nc}>" for mb in (1, 2) for nw in (4, 8) for nc in (1, 2, 4)}  # every kernel


def test_engine_check_passes_on_the_cpu_path():
    pairs = X.check_engine(CPU, expect_graphs=False)
    assert len(pairs) == 1 + 2 + 16
