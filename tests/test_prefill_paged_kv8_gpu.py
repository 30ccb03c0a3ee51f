"""csrc/kernels/prefill_paged_kv8.hip through ``torch.ops.mxllm.prefill_attn_paged_kv8``, per element.

The cases of tests/test_prefill_paged_gpu.py (imported), their bf16 pools quantised by the CPU codec (tests/_kv8.py
``quantize_cache``): every row outside [0, p0 + n) of a used slot holds code 0x7F (an e4m3 NaN) under a NaN scale.
Gaussian: against the fp64 softmax over the DEQUANTISED rows, bound ``_parity.ATTN_O`` (the bf16 kernel's tile body
and rounding points), and bit for bit against ``prefill_attn_paged`` over the dequantised pools.  One-hot: keys of
+-64 e0 quantise exactly (asserted); V, its rows scaled over 80 binades, is its own dequantised quantisation, and the
targeted rows return that V row bit for bit.  Refusals: the failing side of each rule ``mx::pp8_takes`` adds and one
it inherits; a refused call raises and leaves ``out`` and the four pools bitwise unchanged.
"""
import functools

import pytest
import torch

from mxllm.serve.quant import kv8_dequantize
from tests import test_prefill_paged_gpu as PG
from tests._kv8 import NAN_CODE, quantize_cache
from tests._parity import assert_exact

pytestmark = pytest.mark.gpu

F64, I32 = torch.float64, torch.int32
POOLS = ("kq", "ks", "vq", "vs")


def kv8_case(c, spread=False):
    """A bf16 case as a kv8 case: the four pools, and ``kp`` / ``vp`` replaced by the dequantised pools (NaN dead
    rows).  ``spread``: row r of every V block times 2^(r % 81 - 40) first (exact in bf16): scales over 80 binades."""
    vp = c["vp"]
    if spread:
        vp = (vp.float() * torch.exp2(torch.arange(PG.BLK) % 81 - 40.0).view(1, 1, -1, 1)).to(vp.dtype)
    kq, ks, vq, vs, dead = quantize_cache(c["kp"], vp)
    assert dead.any() and (kq[dead] == NAN_CODE).all() and ks[dead].isnan().all()
    return dict(c, kq=kq, ks=ks, vq=vq, vs=vs, kp=kv8_dequantize(kq, ks), vp=kv8_dequantize(vq, vs), live=~dead)


def logical(pool, slot, L):
    """Positions [0, L) of ``slot`` as [Hkv, L, D] through TABLE (plain indexing)."""
    return torch.cat([pool[PG.TABLE[slot][j], :, :min(PG.BLK, L - j * PG.BLK)] for j in range((L + PG.BLK - 1) // PG.BLK)], 1)


@functools.lru_cache(maxsize=None)
def gauss_case(Hq, Hkv, segs):
    c = kv8_case(PG.gauss_case(Hq, Hkv, segs))
    c["ref"] = []
    for row0, n, slot, p0 in c["table"]:
        L, G = p0 + n, Hq // Hkv
        k64 = logical(c["kp"], slot, L).to(F64).repeat_interleave(G, 0)
        v64 = logical(c["vp"], slot, L).to(F64).repeat_interleave(G, 0)
        s = torch.einsum("nhd,hld->hnl", c["q"][row0:row0 + n].to(F64), k64) * PG.SCALE
        dead = torch.arange(L).view(1, 1, L) > (torch.arange(n).view(1, n, 1) + p0)
        c["ref"].append(torch.einsum("hnl,hld->nhd", s.masked_fill(dead, float("-inf")).softmax(-1), v64))
    return c


def run_kv8(ops, dev, c, Hq):
    out = PG.canary_out(c["T"], Hq).to(dev)
    r = ops.prefill_attn_paged_kv8(c["q"].to(dev), *(c[k].to(dev) for k in POOLS),
                                   torch.tensor(PG.TABLE, dtype=I32, device=dev), torch.tensor(c["table"], dtype=I32),
                                   PG.SCALE, out)
    assert r.data_ptr() == out.data_ptr()
    return out.cpu()


@pytest.mark.parametrize("segs", PG.SEGMENTS, ids=PG.seg_id)
@pytest.mark.parametrize("Hq,Hkv", PG.HEADS)
def test_kv8_gaussian_parity_and_identity_with_bf16_kernel(gpu, Hq, Hkv, segs):
    c = gauss_case(Hq, Hkv, segs)
    out = run_kv8(PG._ops(), gpu, c, Hq)
    PG.check_gauss(out, c, Hq, "kv8")
    assert_exact(PG.bits(out), PG.bits(PG.run_hip(PG._ops(), gpu, c, Hq)), name="kv8 against bf16 over the dequantised pools")


@pytest.mark.parametrize("second", [False, True], ids=["diagonal", "next_key_invisible"])
@pytest.mark.parametrize("segs", PG.SEGMENTS, ids=PG.seg_id)
@pytest.mark.parametrize("Hq,Hkv", PG.HEADS)
def test_kv8_onehot_exact(gpu, Hq, Hkv, segs, second):
    per_seg = [PG.onehot_ts(n, p0) for n, p0 in segs]
    for i in range(max(len(x) for x in per_seg)):
        ts = [x[min(i, len(x) - 1)] for x in per_seg]
        b = PG.onehot_case(Hq, Hkv, segs, ts, second)
        c = kv8_case(b, spread=True)
        assert torch.equal(c["kp"][c["live"]], b["kp"][c["live"]])  # keys of +-64 e0 quantise exactly
        c["vlog"] = [logical(c["vp"], slot, p0 + n) for _, n, slot, p0 in c["table"]]
        PG.check_onehot(run_kv8(PG._ops(), gpu, c, Hq), c, Hq, Hkv, ts, second, "kv8")


def test_kv8_refusals(gpu):
    ops, dev, Hq = PG._ops(), gpu, 8
    c = gauss_case(Hq, 2, ((3, 0), (128, 300), (200, 17)))
    q, bt = c["q"].to(dev), torch.tensor(PG.TABLE, dtype=I32, device=dev)
    pools = {k: c[k].to(dev) for k in POOLS}
    before = {k: v.clone() for k, v in pools.items()}
    out = PG.canary_out(c["T"], Hq).to(dev)
    refused = {
        "codes uint8": dict(kq=pools["kq"].view(torch.int8)),
        "scales float32": dict(vs=pools["vs"].double()),
        "scale shape is the code shape without D": dict(ks=pools["ks"][:, :, :255].contiguous()),
        "K and V pools of one shape": dict(vq=pools["vq"][:7].contiguous(), vs=pools["vs"][:7].contiguous()),
        "blk % 256 (inherited)": {k: v[:, :, :128].contiguous() for k, v in pools.items()},
    }
    for rule, kw in refused.items():
        with pytest.raises(RuntimeError):
            ops.prefill_attn_paged_kv8(q, *({**pools, **kw}[k] for k in POOLS), bt, torch.tensor(c["table"], dtype=I32),
                                       PG.SCALE, out)
        torch.cuda.synchronize()
        assert torch.equal(PG.bits(out.cpu()), PG.bits(PG.canary_out(c["T"], Hq))), rule
        for k in POOLS:  # bitwise: NaN scales compare as integers
            assert torch.equal(pools[k].view(torch.uint8), before[k].view(torch.uint8)), (rule, k)
