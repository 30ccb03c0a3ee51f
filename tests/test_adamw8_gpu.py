"""``adamw8_kernel`` (csrc/kernels/elementwise.hip) through ``ops.adamw_step_``: the cases and checks of
tests/test_adamw8_cpu.py on the GPU."""
import pytest
import torch

from mxllm import ops
from mxllm.ops import reference as ref
from tests import test_adamw8_cpu as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("split", [False, True], ids=["master32", "splitmaster"])
@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16], ids=["gradf32", "gradbf16"])
@pytest.mark.parametrize("n,off", [(n, 0) for n in C.SIZES] + [(320, 128)], ids=["n64", "n320", "2passes", "slice"])
def test_step(gpu, n, off, gdt, split):
    """One step against fp64 from the decoded old state (ZERO variant with the split master); ``slice``: blocks
    2..6 of a 9-block buffer, whose other blocks keep their bytes."""
    P, G, M, V = C.make_case(n + 2 * off, gdt, gpu)
    sl = slice(off, off + n)
    p, g, m, v = P[sl], G[sl], M[sl], V[sl]
    parts = [(q.codes, 1) for q in (M, V)] + [(q.exps, 64) for q in (M, V)]
    outside = lambda: [torch.cat([t[:off // k], t[(off + n) // k:]]) for t, k in parts]
    before = outside()
    p0, m0, s0, g0 = p.clone(), m.float(), ref.q8_decode(v.codes, v.exps), g.clone()
    master = ops.SplitMaster(torch.empty_like(p, dtype=torch.bfloat16)) if split else p
    master.copy_(p0)
    ops.adamw_step_(master, g, m, v, None, grad_scale=torch.tensor([C.GS], device=gpu), zero_grad=split, **C.ADAM)
    C.check_step(p0, g0, m0, s0, master.float(), m, v, n >= 320 and not off)
    assert m.base == off and all(torch.equal(x, y) for x, y in zip(outside(), before))
    assert not g.any() if split else torch.equal(g, g0)


def test_rules_match_the_reference(gpu):
    C.run_exact_halving(gpu)
    C.run_chunked(gpu)
    # zero gradients: sqrt(beta2 s^2) is the same IEEE arithmetic on both sides, so the kernel's hash and rounding
    # reproduce the Python rule bit for bit over all K steps
    v, w = C.run_decay(gpu), C.run_decay()
    assert torch.equal(v.codes.cpu(), w.codes) and torch.equal(v.exps.cpu(), w.exps)
