"""Calls the training attention ops refuse: each raises, names its op, and leaves preallocated outputs
bit-unchanged -- the operand checks of the binding (``attn_fill``, csrc/bindings.cpp) and ``mx::ab_takes``
(csrc/kernels/attn_args.h) run before anything is allocated or enqueued.  Shapes: B1 Hq2 Hkv1 S = Sk = 65 D32
(nothing is launched on a refusal); the same shape is taken by ``attn_fwd`` and by ``attn_bwd`` in every
dq mode, checked against fp64 with the attention bounds of tests/_parity.py."""
import math

import pytest
import torch

from tests.test_attention_strict_gpu import attn_inputs, check_attention

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
CASE = (1, 2, 1, 65, 65, 32, True)  # (B, Hq, Hkv, S, Sk, D, causal)
SENTINEL = -123456.75


def _ops():
    from mxllm.ops import native

    return native()


def _call(gpu, D=32, Hq=2, Hkv=1):
    """A valid backward call at the base shape: (dout, q, k, v, o, lse, causal, scale)."""
    B, S = 1, 65
    g = torch.Generator().manual_seed(77 + D + Hq)
    q = torch.randn(B, Hq, S, D, generator=g).to(BF16).to(gpu)
    k = torch.randn(B, Hkv, S, D, generator=g).to(BF16).to(gpu)
    v = torch.randn(B, Hkv, S, D, generator=g).to(BF16).to(gpu)
    do = torch.randn(B, S, Hq * D, generator=g).to(BF16).to(gpu)
    o = torch.zeros(B, S, Hq * D, dtype=BF16, device=gpu)
    lse = torch.zeros(B, Hq, S, dtype=torch.float32, device=gpu)
    return [do, q, k, v, o, lse, True, 1.0 / math.sqrt(D)]


def test_the_base_shape_is_taken_in_every_mode(gpu):
    ops = _ops()
    assert attn_inputs(CASE)[0].shape == (1, 2, 65, 32)
    check_attention(CASE, ops.attn_fwd, ops.attn_bwd, gpu)


DO, Q, K, V, O, LSE = range(6)


def _f16_q(a):
    a[Q] = a[Q].to(torch.float16)


def _k_batch(a):
    a[K] = torch.cat([a[K], a[K]], 0)
    a[V] = torch.cat([a[V], a[V]], 0)


def _v_shape(a):
    a[V] = a[V][:, :, :64].contiguous()


def _lse_short(a):
    a[LSE] = a[LSE].flatten()[:-1].contiguous()


@pytest.mark.parametrize("name,change,mode", [("float16 q", _f16_q, 3), ("k of another batch size", _k_batch, 3),
                                              ("v of another shape than k", _v_shape, 3), ("lse one element short", _lse_short, 3),
                                              ("dq_mode 4", lambda a: None, 4)])
def test_attn_bwd_refuses_and_leaves_the_outputs(gpu, name, change, mode):
    ops = _ops()
    a = _call(gpu)
    change(a)
    outs = [torch.full((1, 2, 65, 32), SENTINEL, device=gpu) for _ in range(3)]
    with pytest.raises(RuntimeError, match="attn_bwd"):
        ops.attn_bwd(*a, mode)
    if mode == 3:
        with pytest.raises(RuntimeError, match="attn_bwd"):
            ops.attn_bwd(*a, mode, *outs)
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t == SENTINEL).all()), name


@pytest.mark.parametrize("Hq,Hkv,D", [(3, 2, 32), (2, 1, 48)])
def test_attn_bwd_refuses_shapes_the_kernels_do_not_take(gpu, Hq, Hkv, D):
    ops = _ops()
    a = _call(gpu, D=D, Hq=Hq, Hkv=Hkv)
    outs = [torch.full((1, Hq, 65, D), SENTINEL, device=gpu) for _ in range(3)]
    for extra in ((3,), (3, *outs), (1,), (2,)):
        with pytest.raises(RuntimeError, match="attn_bwd.*do not take this call"):
            ops.attn_bwd(*a, *extra)
    with pytest.raises(RuntimeError, match="attn_fwd.*do not take this call"):
        ops.attn_fwd(a[Q], a[K], a[V], True, a[7])
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t == SENTINEL).all())


def test_attn_bwd_refuses_preallocated_outputs_with_one_missing(gpu):
    ops = _ops()
    a = _call(gpu)
    dq, dk = [torch.full((1, 2, 65, 32), SENTINEL, device=gpu) for _ in range(2)]
    with pytest.raises(RuntimeError, match="attn_bwd.*all three"):
        ops.attn_bwd(*a, 3, dq, dk, None)
    with pytest.raises(RuntimeError, match="attn_bwd.*all three"):
        ops.attn_bwd(*a, 2, dq, dk, dq.clone())  # all three, but not the split mode
    torch.cuda.synchronize()
    assert bool((dq == SENTINEL).all()) and bool((dk == SENTINEL).all())


def test_attn_bwd_rope_refusals(gpu):
    ops = _ops()
    a = _call(gpu, D=64)
    cs = torch.rand(65, 32, device=gpu)
    with pytest.raises(RuntimeError, match="attn_bwd_rope"):
        ops.attn_bwd_rope(*a, cs, cs, 0)
    a = _call(gpu, D=128)
    cs = torch.rand(65, 64, device=gpu)
    with pytest.raises(RuntimeError, match="attn_bwd_rope.*cos"):
        ops.attn_bwd_rope(*a, cs.cpu(), cs, 0)
    with pytest.raises(RuntimeError, match="attn_bwd_rope.*sin"):
        ops.attn_bwd_rope(*a, cs, cs.cpu(), 0)
    with pytest.raises(RuntimeError, match="attn_bwd_rope"):
        ops.attn_bwd_rope(*a, cs[:64], cs, 0)  # a table row short
