"""Helpers of the fp8 (kv8) KV-cache tests: tests/test_kv8_cpu.py and tests/test_kv8_gpu.py.

The CPU codec (mxllm/serve/quant.py kv8_quantize / kv8_dequantize) is the reference of every
expectation.  The case builders are those of tests/test_decode_exact_gpu.py, imported, not copied:
a bf16 case becomes a kv8 case by ``quantize_case`` below.
"""
import functools

import torch

from mxllm.serve.quant import kv8_dequantize, kv8_quantize
from tests import test_decode_exact_gpu as X

BF16, F32, F64, I32, U8 = torch.bfloat16, torch.float32, torch.float64, torch.int32, torch.uint8
NAN_CODE = 0x7F  # an e4m3fn NaN: the poison of dead code rows (their scales hold NaN)


def e4m3_values():
    """The value of every code 0..255 as torch.float8_e4m3fn defines it (f32; 0x7F / 0xFF are NaN)."""
    return torch.arange(256, dtype=torch.int16).to(U8).view(torch.float8_e4m3fn).float()


def random_rows(g, R, lo=-40, hi=40):
    """bf16 rows [R, 128]: Gaussian, row r scaled by 2^k with k cycling through [lo, hi].  Row 1 (when
    there is one) is all zero; the largest magnitudes of rows 0, 2 and 3 are 1, 1.75 and the next bf16
    above 1.75 (the mantissa edges of the scale rule)."""
    k = torch.arange(R) % (hi - lo + 1) + lo
    x = (torch.randn(R, 128, generator=g) * torch.exp2(k.float())[:, None]).to(BF16)
    for r, top in ((0, 1.0), (2, -1.75), (3, 1.7578125)):
        if r < R:
            x[r] = (x[r].float() * torch.exp2(-k[r].float())).clamp(-1, 1).to(BF16)
            x[r, 5 + r] = top
    if R > 1:
        x[1] = 0
    return x


def quantize_cache(kc, vc):
    """A poisoned bf16 cache pair [n0, Hkv, rows, 128] (dead rows all NaN, X.poison_dead_rows) as kv8
    pools: dead rows become zeros before quantising and hold code 0x7F and scale NaN afterwards.
    Returns (k_codes, k_scale, v_codes, v_scale, dead [n0, Hkv, rows])."""
    dead = kc.isnan().all(-1)
    assert torch.equal(dead, vc.isnan().all(-1)) and not kc[~dead].isnan().any() and not vc[~dead].isnan().any()
    out = []
    for c in (kc, vc):
        codes, scale = kv8_quantize(torch.where(dead[..., None], torch.zeros_like(c), c))
        codes[dead] = NAN_CODE
        scale[dead] = float("nan")
        out += [codes, scale]
    return (*out, dead)


@functools.lru_cache(maxsize=2)
def onehot_kv8(case, lens=None):
    """X.onehot_case as a kv8 case: the codec's codes, V replaced by its dequantised quantisation and
    ``want`` rebuilt from it by plain indexing (mean of the target rows, exact in bf16)."""
    D, Hq, Hkv, paged, tie = case
    assert D == 128
    c = dict(X.onehot_case(case, lens))
    kq, ks, vq, vs, dead = quantize_cache(c["kc"], c["vc"])
    # keys of +-1 quantise exactly: scale 2^-8, codes 0x78 / 0xF8
    live = ~dead
    assert (ks[live] == 2.0 ** -8).all() and ((kq[live] == 0x78) | (kq[live] == 0xF8)).all()
    assert torch.equal(kv8_dequantize(kq, ks)[live], c["kc"][live])
    vdq = kv8_dequantize(vq, vs)
    rep, B = Hq // Hkv, len(c["lens_list"])
    want = torch.zeros(B, Hq, D, dtype=BF16)
    for b, L in enumerate(c["lens_list"]):
        if not L:
            continue
        V = X.kv_logical(vdq, c["bt"], int(c["slots"][b]), L)
        for h, ts in enumerate(c["targets"][b]):
            mean = V[h // rep, ts].double().sum(0) / len(ts)
            want[b, h] = mean.to(BF16)
            assert torch.equal(want[b, h].double(), mean)
    c.update(kq=kq, ks=ks, vq=vq, vs=vs, vdq=vdq, want=want.view(B, Hq * D))
    return c


@functools.lru_cache(maxsize=2)
def gauss_kv8(case):
    """X.gauss_case as a kv8 case; ``kc`` / ``vc`` become the dequantised cache (a bf16 cache, NaN in
    the dead rows: 0x7F codes times NaN scales), so X.gauss_reference applies unchanged."""
    assert case[0] == 128
    c = dict(X.gauss_case(case))
    kq, ks, vq, vs, _ = quantize_cache(c["kc"], c["vc"])
    c.update(kq=kq, ks=ks, vq=vq, vs=vs, kc=kv8_dequantize(kq, ks), vc=kv8_dequantize(vq, vs))
    return c


def run_attn_kv8(ops, c, dev, scale=1.0, max_len=None):
    return ops.decode_attn_kv8(c["q"].to(dev), c["kq"].to(dev), c["ks"].to(dev), c["vq"].to(dev), c["vs"].to(dev),
                               c["lens"].to(dev), c["slots"].to(dev), c["cap"] if max_len is None else max_len,
                               scale, 0, X._dev(c["bt"], dev))
