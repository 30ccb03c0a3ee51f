"""The document mask off the GPU: the tables (``ops.doc_bounds``), the CPU route of
``attention_block(doc=...)`` against per-document calls, the refusal with sequence parallelism, and the
native launch check (csrc/kernels/attn_doc_args.h) in a stand-alone host program."""
import os
import shutil
import subprocess

import pytest
import torch

from mxllm import ops
from mxllm.ops import reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EOS = 2


@pytest.mark.parametrize("ids", [
    [5, 6, 7, 8, 9, 3],            # no EOS
    [EOS, 5, 6, EOS, 7, 8],        # EOS first
    [5, 6, EOS, 7, 8, EOS],        # EOS last
    [5, EOS, EOS, EOS, 6, 7, EOS, EOS],  # consecutive EOS
], ids=["none", "first", "last", "consecutive"])
def test_doc_bounds_against_loop(ids):
    start, end, s0 = [], [], 0
    for i, t in enumerate(ids):
        start.append(s0)
        if t == EOS:
            end += [i + 1] * (i + 1 - s0)
            s0 = i + 1
    end += [len(ids)] * (len(ids) - len(end))
    ds, de = ops.doc_bounds(torch.tensor([ids, ids[::-1]]), EOS)
    assert ds.dtype == de.dtype == torch.int32 and ds.shape == (2, len(ids))
    assert ds[0].tolist() == start and de[0].tolist() == end


@pytest.mark.parametrize("D,lens", [(32, [7, 1, 1, 20, 4]), (64, [33]), (128, [16, 17])])
def test_cpu_attention_block_equals_per_document_calls(D, lens):
    B, Hq, Hkv, S = 2, 4, 2, sum(lens)
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(B * S, (Hq + 2 * Hkv) * D, generator=g)
    cos, sin = ref.rope_tables(S, D, 10000.0, None)
    bounds = [(sum(lens[:i]), sum(lens[:i + 1])) for i in range(len(lens))]
    ds = torch.tensor([[s for s, e in bounds for _ in range(e - s)]] * B, dtype=torch.int32)
    de = torch.tensor([[e for s, e in bounds for _ in range(e - s)]] * B, dtype=torch.int32)
    got = ops.attention_block(qkv, cos, sin, B, S, Hq, Hkv, D, doc=(ds, de)).view(B, S, Hq * D)
    x = qkv.view(B, S, -1)
    # The expression and the numbers are the same; torch's CPU reductions (the D-term score dot, the
    # softmax sum and the P V sum of at most S terms) pick their summation order by shape, so the two
    # agree to fp32 reordering error, not bitwise (observed: 0 to 3.6e-7).  Reordering an n-term fp32 sum
    # moves it by at most n 2^-23 of its magnitude sum; a score error dx moves p by dx relatively, and
    # |x| <= |q| |k| / sqrt(D) (the rotation keeps norms); |o| <= max |v|.  A masking error is O(max |v|).
    heads = x.view(B, S, Hq + 2 * Hkv, D)
    smax = (heads[:, :, :Hq].norm(dim=-1).max() * heads[:, :, Hq:Hq + Hkv].norm(dim=-1).max() / D ** 0.5).item()
    tol = (D + 2 * S) * 2.0 ** -23 * max(1.0, smax) * heads[:, :, Hq + Hkv:].abs().max().item()
    for s, e in bounds:  # the same rotated q / k: the tables' rows of the document's positions
        want = ops.attention_block(x[:, s:e].reshape(B * (e - s), -1), cos[s:e], sin[s:e], B, e - s, Hq, Hkv, D)
        err = (got[:, s:e] - want.view(B, e - s, Hq * D)).abs().max().item()
        assert err <= tol, (s, e, err, tol)


def test_document_mask_refuses_sequence_parallel():
    from mxllm.models import Llama, get_config

    m = Llama(get_config("tiny"), init=False)
    m.set_document_mask(EOS)
    with pytest.raises(ValueError):
        m.set_sequence_parallel(object())
    with pytest.raises(ValueError):
        m.set_context_parallel(object())
    m.set_document_mask(None)
    m.seq_parallel = object()
    with pytest.raises(ValueError):
        m.set_document_mask(EOS)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_native_attn_doc_args(tmp_path):
    exe = str(tmp_path / "test_attn_doc_args")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "csrc"),
                    os.path.join(ROOT, "tests", "native", "test_attn_doc_args.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout
