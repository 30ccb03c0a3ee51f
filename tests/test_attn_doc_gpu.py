"""Document-masked attention kernels (csrc/kernels/attn_doc.hip) on the MI355X.

1. Against fp64 (visibility doc_start[i] <= j <= i): O, lse, dQ, dK, dV.  The bound of each tensor is
   twice the error of the EXISTING attn_fwd / attn_bwd (split mode) run on each document alone -- the
   factor 2 covers the different accumulation order of the 64- / 128-key tiles relative to a document's
   start; a masking error is O(1).
2. Isolation, bit for bit: replacing one document's q, k, v, dO rows leaves the other document's rows of
   every output unchanged -- also through the chunked (small dS^T budget) backward.
"""
import math

import pytest
import torch

from tests.test_attention_strict_gpu import LOG2E, attn_inputs

pytestmark = pytest.mark.gpu

# (B, Hq, Hkv, S, D, document lengths per batch row)
CASES = [
    (2, 8, 2, 257, 128, ([257], [257])),  # one document: the plain causal function
    (2, 8, 2, 257, 128, ([63, 1, 1, 62, 1, 1, 128], [100, 157])),  # ends at 63/64/65, 127/128/129; a document
    (2, 4, 2, 129, 64, ([60] + [1] * 8 + [61], [129])),            # across two q blocks; length-1 run over a tile edge
    (2, 4, 2, 257, 64, ([200, 57], [64, 64, 64, 65])),
    (1, 4, 2, 129, 32, ([65, 64],)),
    (1, 4, 2, 257, 32, ([127, 1, 1, 128],)),
]


def tables(lens, dev):
    """(doc_start, doc_end) int32 [B, S] of per-row document lengths."""
    ds = torch.tensor([[s0 for s0, n in zip(_starts(row), row) for _ in range(n)] for row in lens], dtype=torch.int32)
    de = torch.tensor([[s0 + n for s0, n in zip(_starts(row), row) for _ in range(n)] for row in lens], dtype=torch.int32)
    return ds.to(dev), de.to(dev)


def _starts(row):
    return [sum(row[:i]) for i in range(len(row))]


def ref64(q, k, v, do, ds, scale):
    """fp64 O [B,S,Hq*D], lse (log2 domain), dQ, dK, dV of the bf16 inputs."""
    B, Hq, S, D = q.shape
    G = Hq // k.shape[1]
    q, k, v = q.double(), k.double().repeat_interleave(G, 1), v.double().repeat_interleave(G, 1)
    i, j = torch.arange(S, device=q.device).view(S, 1), torch.arange(S, device=q.device).view(1, S)
    vis = (j <= i) & (j >= ds.long().view(B, 1, S, 1))
    x = (q @ k.transpose(-1, -2) * (scale * LOG2E)).masked_fill(~vis, float("-inf"))
    lse = torch.log2(torch.exp2(x - x.amax(-1, keepdim=True)).sum(-1)) + x.amax(-1)
    p = torch.exp2(x - lse.unsqueeze(-1))
    o = p @ v
    doh = do.double().view(B, S, Hq, D).transpose(1, 2)
    dsc = p * (doh @ v.transpose(-1, -2) - (doh * o).sum(-1, keepdim=True))
    dq = dsc @ k * scale
    dk = (dsc.transpose(-1, -2) @ q).view(B, -1, G, S, D).sum(2) * scale
    dv = (p.transpose(-1, -2) @ doh).view(B, -1, G, S, D).sum(2)
    return o.transpose(1, 2).reshape(B, S, Hq * D), lse, dq, dk, dv


def group_sum(part, Hkv):
    B, _, S, D = part.shape
    return part.double().view(B, Hkv, -1, S, D).sum(2)


def per_document(ops, q, k, v, do, lens, scale):
    """The existing kernels on each document alone, assembled: O, lse, dQ, dK, dV (fp64)."""
    B, Hq, S, D = q.shape
    Hkv = k.shape[1]
    o = torch.zeros(B, S, Hq * D, dtype=torch.float64, device=q.device)
    lse, dq = torch.zeros(B, Hq, S, dtype=torch.float64, device=q.device), torch.zeros_like(q, dtype=torch.float64)
    dk, dv = torch.zeros_like(k, dtype=torch.float64), torch.zeros_like(k, dtype=torch.float64)
    for b, row in enumerate(lens):
        for s, n in zip(_starts(row), row):
            e = s + n
            qs, ks, vs = (t[b:b + 1, :, s:e].contiguous() for t in (q, k, v))
            dos = do[b:b + 1, s:e].contiguous()
            od, ld = ops.attn_fwd(qs, ks, vs, True, scale)
            dqd, dkd, dvd = ops.attn_bwd(dos, qs, ks, vs, od, ld, True, scale, 3)
            o[b, s:e], lse[b, :, s:e], dq[b, :, s:e] = od[0].double(), ld[0].double(), dqd[0].double()
            dk[b, :, s:e], dv[b, :, s:e] = group_sum(dkd, Hkv)[0], group_sum(dvd, Hkv)[0]
    return o, lse, dq, dk, dv


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"B{c[0]}-Hq{c[1]}-Hkv{c[2]}-S{c[3]}-D{c[4]}-{len(c[5][0])}docs")
def test_attn_doc_against_fp64(gpu, case):
    from mxllm.ops import native

    ops = native()
    B, Hq, Hkv, S, D, lens = case
    scale = 1.0 / math.sqrt(D)
    q, k, v, do = [t.to(gpu) for t in attn_inputs((B, Hq, Hkv, S, S, D, True))]
    ds, de = tables(lens, gpu)
    ref = ref64(q, k, v, do, ds, scale)
    o, lse = ops.attn_doc_fwd(q, k, v, ds, scale)
    dq, dkp, dvp = ops.attn_doc_bwd(do, q, k, v, o, lse, ds, de, scale)
    new = (o.double(), lse.double(), dq.double(), group_sum(dkp, Hkv), group_sum(dvp, Hkv))
    old = per_document(ops, q, k, v, do, lens, scale)
    bad = []
    for name, n, p, r in zip(("O", "lse", "dQ", "dK", "dV"), new, old, ref):
        en, eo = (n - r).abs().max().item(), (p - r).abs().max().item()
        print(f"{name}: new {en:.3e} per-document existing {eo:.3e} ratio {en / max(eo, 1e-300):.2f}")
        if not en <= 2 * eo:
            bad.append((name, en, eo))
    assert not bad, bad


@pytest.mark.parametrize("replaced,budget_gb", [("A", None), ("B", None), ("A", 1e-4), ("B", 1e-4)])
def test_attn_doc_documents_are_isolated_bitwise(gpu, replaced, budget_gb, monkeypatch):
    from mxllm.ops import attention, native

    B, Hq, Hkv, S, D, nA = 2, 8, 2, 257, 128, 100  # [A | B]: the boundary inside a 64-key tile and a q block
    if budget_gb is not None:  # the chunked backward: per (sequence, 4 heads) at this budget
        monkeypatch.setattr(attention, "_DS_BUDGET", budget_gb * 2**30)
    scale = 1.0 / math.sqrt(D)
    ds, de = tables(([nA, S - nA],) * B, gpu)
    rows = slice(0, nA) if replaced == "A" else slice(nA, S)
    kept = slice(nA, S) if replaced == "A" else slice(0, nA)

    def run(inputs):
        q, k, v, do = [t.to(gpu) for t in inputs]
        o, lse = native().attn_doc_fwd(q, k, v, ds, scale)
        dq, dkp, dvp = attention.attn_bwd(do, q, k, v, o, lse, True, scale, 3, (ds, de))
        return [o[:, kept], lse[:, :, kept], dq[:, :, kept], dkp[:, :, kept], dvp[:, :, kept]]

    base = attn_inputs((B, Hq, Hkv, S, S, D, True))
    g = torch.Generator().manual_seed(77)
    swapped = []
    for t, dim in zip(base, (2, 2, 2, 1)):
        t2 = t.clone()
        idx = [slice(None)] * t.dim()
        idx[dim] = rows
        t2[tuple(idx)] = torch.randn(t2[tuple(idx)].shape, generator=g).to(t.dtype)
        swapped.append(t2)
    for name, a, b in zip(("O", "lse", "dQ", "dK", "dV"), run(base), run(swapped)):
        assert torch.equal(a, b), name
