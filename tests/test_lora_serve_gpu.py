"""GPU tests of multi-adapter LoRA serving: csrc/kernels/lora_serve.hip (lora_gather_shrink,
lora_gather_expand_add_), ``ops.lora_delta_rows_`` (decode rows and the segmented prefill path) and
the engine's adapter mode (mixed batches, hipGraph replay, both KV cache formats).

Inputs, references and how every bound was obtained: tests/_lora_serve.py.
``python -m tests.test_lora_serve_gpu`` (no GPU) prints the error of the fp32 models of the documented
algorithms against fp64 and asserts that it stays within the recorded measurements.
"""
import functools

import pytest
import torch

from tests import _lora_serve as L
from tests._parity import assert_exact, assert_parity

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
CASES = [(si, M) for si in range(len(L.SHAPES)) for M in L.MS]


def case_id(c):
    K, sp, r = L.SHAPES[c[0]]
    return f"K{K}-s{len(sp)}-r{r}-M{c[1]}"


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16)


@functools.lru_cache(maxsize=None)
def _case(si: int, M: int, kind: str):
    K, sp, r = L.SHAPES[si]
    c = L.make_case(K, sp, r, M, kind=kind)
    c["ref"] = L.ref_fp64(c)
    return c


@functools.lru_cache(maxsize=None)
def _tables(si: int, kind: str, dev: str):
    return L.tables_of(_case(si, L.MAX_M, kind), dev)


def _padded(t: torch.Tensor, pad: int, gen: torch.Generator) -> torch.Tensor:
    """A [M, W + pad] buffer of a random bit pattern whose left part holds ``t``."""
    buf = torch.randint(-32768, 32767, (t.shape[0], t.shape[1] + pad), generator=gen, dtype=torch.int16).view(BF16)
    buf[:, :t.shape[1]] = t
    return buf


def run_delta(c, t, gpu, strided: bool):
    """(y after the call as the whole CPU buffer, the fill it started from, N)."""
    from mxllm.ops import lora_delta_rows_

    g = torch.Generator().manual_seed(77)
    N = c["y0"].shape[1]
    ybuf = _padded(c["y0"], 24 if strided else 0, g)
    xbuf = _padded(c["x"], 8 if strided else 0, g)
    yd, xd = ybuf.to(gpu), xbuf.to(gpu)
    lora_delta_rows_(yd[:, :N], xd[:, :c["K"]], c["ids"].to(gpu), t)
    return yd.cpu(), ybuf, N


def check_untouched(c, out, fill, N, name):
    dead = c["ids"] < 0
    assert_exact(bits(out[dead]), bits(fill[dead]), f"{name}: rows without an adapter")
    assert_exact(bits(out[:, N:]), bits(fill[:, N:]), f"{name}: padding columns of y")


# =========================================================================== 1. parity, 3. untouched memory
@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "strided"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_delta_rows_parity(gpu, case, strided):
    c, t = _case(*case, "gauss"), _tables(case[0], "gauss", str(gpu))
    out, fill, N = run_delta(c, t, gpu, strided)
    live = c["ids"] >= 0
    assert_parity(out[:, :N][live], c["ref"][live], L.LORA_DELTA_Y, name=case_id(case))
    check_untouched(c, out, fill, N, case_id(case))


# =========================================================================== 2. exact routing
@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "strided"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_delta_rows_exact_routing(gpu, case, strided):
    """Small-integer inputs: every fp32 operation is exact, so the kernels must give the bits of the
    fp32 model, which equals fp64 -- any wrong adapter, split, column or partial shows."""
    c, t = _case(*case, "int"), _tables(case[0], "int", str(gpu))
    _, st = L._by_formula(c, torch.float64, None)
    assert max(st["t"], st["acc"], 2 * float(c["ref"].abs().max())) < 2 ** 24  # intermediates are exact in fp32
    m32 = L.model_fp32(c)
    assert torch.equal(m32.double(), c["ref"])
    out, fill, N = run_delta(c, t, gpu, strided)
    assert_exact(out[:, :N], m32.to(BF16), case_id(case))
    check_untouched(c, out, fill, N, case_id(case))


@pytest.mark.parametrize("si", range(len(L.SHAPES)), ids=lambda i: f"K{L.SHAPES[i][0]}")
def test_delta_rows_no_adapter_at_all(gpu, si):
    K, sp, r = L.SHAPES[si]
    c = L.make_case(K, sp, r, 5, all_none=True)
    out, fill, N = run_delta(c, _tables(si, "gauss", str(gpu)), gpu, True)
    assert_exact(bits(out), bits(fill), "all rows -1")


# =========================================================================== 4. batch invariance
@pytest.mark.parametrize("case", [c for c in CASES if c[1] > 1], ids=case_id)
def test_delta_rows_batch_invariant(gpu, case):
    from mxllm.ops import lora_delta_rows_

    c, t = _case(*case, "gauss"), _tables(case[0], "gauss", str(gpu))
    x, ids = c["x"].to(gpu), c["ids"].to(gpu)
    y1, y2 = c["y0"].to(gpu), c["y0"].to(gpu)
    lora_delta_rows_(y1, x, ids, t)
    lora_delta_rows_(y2, x, ids, t)
    assert_exact(bits(y2.cpu()), bits(y1.cpu()), "two identical calls")
    rows = range(c["M"]) if c["M"] <= 8 else (0, 2, 3, 31, 62, 63)
    for b in rows:
        ya = c["y0"][b:b + 1].to(gpu)
        lora_delta_rows_(ya, x[b:b + 1], ids[b:b + 1], t)
        assert_exact(bits(ya.cpu()), bits(y1[b:b + 1].cpu()), f"{case_id(case)}: row {b} alone")


# =========================================================================== 5. operand check
def test_operand_check(gpu):
    from mxllm.ops import native

    c, t = _case(0, 5, "gauss"), _tables(0, "gauss", str(gpu))
    x, y, ids = c["x"].to(gpu), c["y0"].to(gpu), c["ids"].to(gpu)
    part = t.partials(5)
    ok_s = lambda **kw: dict(dict(x=x, ids=ids, a_tab=t.a, partials=part), **kw)  # noqa: E731
    ok_e = lambda **kw: dict(dict(y=y, partials=part, ids=ids, b_tab=t.b, s_tab=t.s, splits=t.splits, K=t.K), **kw)  # noqa: E731
    wide = torch.zeros(5, 264, dtype=BF16, device=gpu)  # [:, 1:257]: rows that are not 16-byte aligned
    bad_shrink = {
        "x dtype": ok_s(x=x.float()), "x device": ok_s(x=x.cpu()), "x stride": ok_s(x=wide[:, 1:257]),
        "x row stride": ok_s(x=torch.zeros(5, 258, dtype=BF16, device=gpu)[:, :256]), "x width": ok_s(x=x[:, :248]),
        "x transposed": ok_s(x=x.t().contiguous().t()), "ids dtype": ok_s(ids=ids.long()), "ids device": ok_s(ids=ids.cpu()),
        "ids length": ok_s(ids=ids[:4]), "ids stride": ok_s(ids=torch.stack([ids, ids], 1)[:, 0]),
        "table dtype": ok_s(a_tab=t.a.float()), "table rank": ok_s(a_tab=t.a[:, :40]),
        "table contiguity": ok_s(a_tab=t.a.transpose(1, 2).contiguous().transpose(1, 2)),
        "table dims": ok_s(a_tab=t.a[0]), "partials dtype": ok_s(partials=part.double()),
        "partials rows": ok_s(partials=t.partials(4)), "partials device": ok_s(partials=part.cpu()),
    }
    for name, kw in bad_shrink.items():
        before = part.clone()
        with pytest.raises(RuntimeError):
            native().lora_gather_shrink(**kw)
        assert torch.equal(part, before), name
    ywide = torch.zeros(5, 386, dtype=BF16, device=gpu)
    bad_expand = {
        "y dtype": ok_e(y=y.float()), "y device": ok_e(y=y.cpu()), "y row stride": ok_e(y=ywide[:, :384]),
        "y transposed": ok_e(y=y.t().contiguous().t()), "y width": ok_e(y=y[:, :376].contiguous()),
        "ids dtype": ok_e(ids=ids.long()), "ids length": ok_e(ids=ids[:3]), "table dtype": ok_e(b_tab=t.b.float()),
        "table rank": ok_e(b_tab=t.b[:, :, :12].contiguous()), "table contiguity": ok_e(b_tab=t.b[:, :, :8]),
        "s dtype": ok_e(s_tab=t.s.double()), "s length": ok_e(s_tab=t.s[:2]), "s device": ok_e(s_tab=t.s.cpu()),
        "splits sum": ok_e(splits=[256, 64]), "splits multiple": ok_e(splits=[252, 68, 64]),
        "splits count": ok_e(splits=[128, 128, 64, 64]), "partials K": ok_e(K=1024), "K multiple": ok_e(K=252),
        "partials columns": ok_e(partials=part[:, :, :32].contiguous()), "partials dtype": ok_e(partials=part.double()),
    }
    for name, kw in bad_expand.items():
        before = y.clone()
        with pytest.raises(RuntimeError):
            native().lora_gather_expand_add_(**kw)
        assert torch.equal(y, before), name


# =========================================================================== 6. prefill path
def test_prefill_segments(gpu):
    from mxllm.ops import lora_delta_rows_

    c = L.prefill_case()
    t = L.tables_of(c, gpu)
    segs = L.segments_of(c["ids"])
    assert [(e - s, a) for s, e, a in segs] == [(5, 0), (3, -1), (1, 1)]
    g = torch.Generator().manual_seed(78)
    fill = _padded(c["y0"], 16, g)
    N = c["y0"].shape[1]
    yd = fill.to(gpu)
    lora_delta_rows_(yd[:, :N], c["x"].to(gpu), None, t, segments=segs)
    out, live = yd.cpu(), c["ids"] >= 0
    assert_parity(out[:, :N][live], L.ref_fp64(c)[live], L.LORA_PREFILL_Y, name="prefill segments")
    check_untouched(c, out, fill, N, "prefill segments")


# =========================================================================== 7. / 8. engine
PROMPT_LENS, STEPS = (19, 40, 7), 4
ROW_ADAPTERS = ("a0", "a1", None)


@functools.lru_cache(maxsize=None)
def _engine_inputs():
    from mxllm.models import get_config

    cfg = get_config("tiny-d128")
    g = torch.Generator().manual_seed(5)
    prompts = [torch.randint(3, cfg.vocab_size, (n,), generator=g).tolist() for n in PROMPT_LENS]
    forced = [torch.randint(3, cfg.vocab_size, (STEPS,), generator=g).tolist() for _ in prompts]
    ads = {"a0": L.random_adapter(cfg, 16, 1), "a1": L.random_adapter(cfg, 8, 2), "a2": L.random_adapter(cfg, 16, 3)}
    return cfg, prompts, forced, ads


@functools.lru_cache(maxsize=None)
def _ref_logits(row: int, name):
    """fp64 logits [STEPS + 1, V] of the prefill's last position and every forced decode step."""
    from mxllm.models import Llama

    cfg, prompts, forced, ads = _engine_inputs()
    m = Llama(cfg, device="cpu", seed=9).eval()
    n = len(prompts[row])
    return L.forward_fp64(m, prompts[row] + forced[row], ads.get(name))[n - 1:n + STEPS]


def teacher_forced(eng, names):
    """Logits [rows, STEPS + 1, V] (f32, CPU) of prefill_batch + STEPS forced decode steps."""
    _, prompts, forced, _ = _engine_inputs()
    slots = list(range(len(prompts)))
    outs = [eng.prefill_batch(slots, prompts, list(names) if eng.lora is not None else None).cpu()]
    for st in range(STEPS):
        # read back before the next step, as the scheduler does: a graphed step refills its pinned input
        outs.append(eng.decode(slots, torch.tensor([f[st] for f in forced])).float().cpu())
    for s in slots:
        eng.kv.release(s)
        eng.lens[s] = 0
        eng.slot_adapter[s] = -1
    return torch.stack(outs, 1)


def make_engine(gpu, graphs: bool, kv: str, max_adapters: int):
    from mxllm.models import Llama
    from mxllm.serve.engine import Engine

    cfg = _engine_inputs()[0]
    model = Llama(cfg, device="cpu", seed=9).eval().to(gpu)  # the CPU generator's weights: those of _ref_logits
    return Engine(model, max_batch=4, max_seq=512, use_graphs=graphs, kv_dtype=kv, max_adapters=max_adapters,
                  max_lora_rank=16)


def engine_error(out, names) -> float:
    """max |out - ref| / row-max |ref| over every row, position and token."""
    err = 0.0
    for i, n in enumerate(names):
        ref = _ref_logits(i, n)
        err = max(err, float(((out[i].double() - ref).abs() / ref.abs().amax(-1, keepdim=True)).max()))
    return err


def check_rows(out, names, kv, what):
    for i, n in enumerate(names):
        assert_parity(out[i], _ref_logits(i, n), L.engine_logits_bound(kv), name=f"{what}: row {i} ({n})")


def test_engine_references_tell_adapters_apart():
    """On the fp64 references: an adapter row's logits differ from the base model's and from the other
    adapter's by at least 10 x the bound, so an ignored or swapped adapter cannot pass."""
    for kv in ("bf16", "fp8"):
        need = 10 * L.engine_logits_bound(kv)[1]
        for i in range(len(PROMPT_LENS)):
            for a, b in (("a0", None), ("a1", None), ("a2", None), ("a0", "a1"), ("a2", "a0"), ("a2", "a1")):
                ra, rb = _ref_logits(i, a), _ref_logits(i, b)
                d = (ra - rb).abs().amax(-1) / torch.maximum(ra.abs().amax(-1), rb.abs().amax(-1))
                assert float(d.min()) >= need, (kv, i, a, b, float(d.min()), need)


@pytest.mark.parametrize("kv", ["bf16", "fp8"])
@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "graphed"])
def test_engine_teacher_forced(gpu, graphs, kv):
    _, _, _, ads = _engine_inputs()
    eng = make_engine(gpu, graphs, kv, 3)
    eng.load_adapter("a0", ads["a0"])
    eng.load_adapter("a1", ads["a1"])
    out = teacher_forced(eng, ROW_ADAPTERS)
    print(f"engine logits error, graphs {graphs}, kv {kv}: adapters {engine_error(out, ROW_ADAPTERS):.4g}, "
          f"bound {L.engine_logits_bound(kv)[1]:.4g}")
    check_rows(out, ROW_ADAPTERS, kv, "mixed batch")
    if not graphs:
        return
    # 8. graph behaviour: a third adapter loaded after capture adds no graph; its rows pass the same check
    assert {k[2] for k in eng._graphs} == {True}
    before = {k: id(v[2]) for k, v in eng._graphs.items()}
    eng.load_adapter("a2", ads["a2"])
    swapped = ("a2", None, "a2")
    out = teacher_forced(eng, swapped)
    assert {k: id(v[2]) for k, v in eng._graphs.items()} == before
    check_rows(out, swapped, kv, "adapter loaded after capture")
    base = teacher_forced(eng, (None, None, None))  # a base-only step: the any_adapter = False graph
    assert {k[2] for k in eng._graphs} == {True, False} and all(id(eng._graphs[k][2]) == v for k, v in before.items())
    check_rows(base, (None, None, None), kv, "base-only steps")
    assert eng.stats()["lora_adapters"] == ["a0", "a1", "a2"]


def _main():
    rel, ab = L.measure(L.model_fp32, L.decode_cases())
    print(f"LORA_DELTA_Y measured (rel, abs) = ({rel:.3g}, {ab:.3g}); recorded {L.LORA_DELTA_Y_MEASURED}")
    assert rel <= L.LORA_DELTA_Y_MEASURED[0] * 1.001 and ab <= L.LORA_DELTA_Y_MEASURED[1] * 1.001
    rel, ab = L.measure(L.prefill_model_fp32, [L.prefill_case()])
    print(f"LORA_PREFILL_Y measured (rel, abs) = ({rel:.3g}, {ab:.3g}); recorded {L.LORA_PREFILL_Y_MEASURED}")
    assert rel <= L.LORA_PREFILL_Y_MEASURED[0] * 1.001 and ab <= L.LORA_PREFILL_Y_MEASURED[1] * 1.001
    for c in L.decode_cases("int"):
        assert torch.equal(L.model_fp32(c).double(), L.ref_fp64(c))
    print("integer inputs: the fp32 model equals fp64 at every shape")
    print(f"ENGINE_LOGITS_MEASURED (base engine on the GPU, see tests/_lora_serve.py) = {L.ENGINE_LOGITS_MEASURED}")


if __name__ == "__main__":
    _main()
