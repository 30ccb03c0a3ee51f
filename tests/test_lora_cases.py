"""The strict LoRA tests (tests/test_lora_strict_gpu.py, tests/_lora_cases.py) on the CPU: every case builds
and covers what its module says, the exactness preconditions hold, the fp64 references agree with an
independent formulation, reference implementations and the CPU path of ``lora_linear_aug`` pass the very
checks (at the very bounds) the kernels meet, and subtly wrong tensors fail them."""
import pytest
import torch

from tests import _lora_cases as LC
from tests import _parity as P

BF16, F32 = torch.bfloat16, torch.float32
CPU = torch.device("cpu")


# =========================================================================== A. the cases
def test_launcher_mirror_gives_the_documented_clamps():
    for (T, req), want in LC.RBW_EXPECTED.items():
        assert LC.rbw_of(T, req) == want, (T, req)
    assert LC.rbw_of(64, None) == 2 and LC.rbw_of(16, None) == 1
    assert LC.split_ranges(5, 2) == [(0, 2), (2, 5)] and LC.split_ranges(3, 2) == [(0, 1), (1, 3)]
    assert LC.cs_of(16, 128, None, 1) == 1 and LC.cs_of(48, 384, None, 1) == 3 and LC.cs_of(64, 128, 2, 2) == 1
    assert LC.cs_of(160, 640, 5, 2) == 5 and LC.cs_of(4096, 28672, None, 2) == 4


def test_tail_cases_cover_the_list():
    cases = LC.TAIL_CASES
    assert len(set(cases)) == len(cases) == 40 and len({LC.tail_id(c) for c in cases}) == 40
    for c in cases:
        assert LC.RBW_EXPECTED.get((c.T, c.rbw_req), 2 if c.T == 64 else 1) == LC.tail_rbw(c)
        assert c.pad in (64, 16 * c.nrb) and sum(LC.tail_trips(c)) == c.F // 128
    # every <BWD, NRB, RBW> instantiation meets an uneven split with more than one trip per workgroup
    multi = {(c.bwd, c.nrb, LC.tail_rbw(c)) for c in cases
             if min(LC.tail_trips(c)) > 1 and len(set(LC.tail_trips(c))) > 1}
    assert multi == {(b, n, r) for b in (False, True) for n in (1, 2, 3, 4) for r in (1, 2, 4)}
    assert {c.T for c in cases} == {16, 48, 64, 160} and {c.F for c in cases} == {128, 384, 640}
    assert {c.rbw_req for c in cases} == {None, 1, 2, 4}
    for bwd in (False, True):
        mine = [c for c in cases if c.bwd == bwd]
        assert {tuple(LC.tail_trips(c)) for c in mine} >= {(1,), (3,), (5,), (1, 2), (2, 3), (1, 1, 1), (1,) * 5}
        assert {(c.F, c.cs_req) for c in mine} >= {(384, None), (384, 1), (384, 2), (640, None), (640, 1), (640, 2),
                                                   (640, 5)}
        for nrb in (1, 2, 3, 4):
            assert {c.pad for c in mine if c.nrb == nrb} == {64, 16 * nrb}
        assert any(c.sat for c in mine)


def test_sat_inputs_saturate_the_sigmoid_both_ways():
    for c in LC.TAIL_CASES:
        if c.sat:
            gate = LC.tail_inputs(c)[0][:, :c.F].float()
            assert bool((torch.sigmoid(gate) == 1).any()) and bool((torch.sigmoid(gate) < 2.0 ** -40).any())
            full = LC.ref_swiglu_lora(LC.tail_inputs(c)[1], LC.tail_inputs(c)[0], c.pad,
                                      LC.tail_v_gauss(c)[:, :LC.tail_width(c)], c.nrb, LC.S_TAIL)
            assert bool(torch.isfinite(full.float()).all())
            assert bool((full[:, :LC.tail_width(c)].float().abs() >= torch.finfo(BF16).tiny).all())  # normal numbers


def test_onehot_rows_visit_every_chunk_of_every_width():
    """Across the cases of one (direction, F): every (tile, 32-column wave slice, 8-column lane group), of the
    dg and of the du half, is selected by some row -- and every position inside a chunk."""
    seen, lanes = {}, {}
    for c in LC.TAIL_CASES:
        for k in range(LC.NSHIFT):
            cols = LC.route_columns(c, k)
            assert len(cols) == 16 * c.nrb and all(0 <= x < LC.tail_width(c) for x in cols)
            seen.setdefault((c.bwd, c.F), set()).update(x // 8 for x in cols)
            lanes.setdefault((c.bwd, c.F), set()).update(x % 8 for x in cols)
            buf, _ = LC.tail_v_onehot(c, k)
            v = buf[:16 * c.nrb, :LC.tail_width(c)]
            assert bool((v.sum(1) == 1).all()) and bool(((v == 0) | (v == 1)).all())
            assert bool((buf[16 * c.nrb:] == LC.POISON).all()) and bool((buf[:, LC.tail_width(c):] == LC.POISON).all())
            assert buf.stride(0) % 8 == 0 and buf.stride(0) > LC.tail_width(c)
    assert set(seen) == {(b, f) for b in (False, True) for f in (128, 384, 640)}
    for (bwd, F), chunks in seen.items():
        nch = (2 * F if bwd else F) // 8
        assert chunks == set(range(nch)), (bwd, F, sorted(set(range(nch)) - chunks))
        if bwd:  # both halves: (half, tile, slice, group)
            assert {(q // (F // 8), q % (F // 8) // 16, q % 16 // 4, q % 4) for q in chunks} == {
                (h, t, s, g) for h in (0, 1) for t in range(F // 128) for s in range(4) for g in range(4)}
        assert lanes[(bwd, F)] == set(range(8))


@pytest.mark.parametrize("case", [c for c in LC.TAIL_CASES if LC.tail_cs(c) > 1], ids=LC.tail_id)
def test_split_rows_have_one_nonzero_per_split_and_exact_sums(case):
    c = case
    _, vals = LC.tail_v_splits(c)
    F, W = c.F, LC.tail_width(c)
    for sp, (t0, t1) in enumerate(LC.split_ranges(F // 128, LC.tail_cs(c))):
        tile = (torch.arange(W) % F) // 128
        assert bool(((vals != 0) & (tile >= t0) & (tile < t1)).sum(1).eq(1).all()), sp
    assert bool((vals != 0).sum(1).eq(LC.tail_cs(c)).all())
    if c.bwd:
        assert bool((vals[:, :F] != 0).any()) and bool((vals[:, F:] != 0).any())
    gu, dm = LC.tail_inputs(c, "bounded")
    out = LC.swiglu_plain_ref(dm, gu).double()
    assert 0.5 <= float(out.abs().min()) and float(out.abs().max()) < 8.0  # within 2^-1 .. 2^3
    idx = vals.abs().argsort(dim=1, descending=True)[:, :LC.tail_cs(c)]
    assert LC.exact_sum_ok(out[:, idx] * vals.double().gather(1, idx))


def test_exact_sum_ok_rejects_a_sum_that_needs_rounding():
    assert LC.exact_sum_ok(torch.tensor([[1.0, 2.0 ** 16, -3.0]]))
    assert not LC.exact_sum_ok(torch.tensor([[1.0, 2.0 ** 24]]))
    assert not LC.exact_sum_ok(torch.tensor([[2.0 ** -20, 1.0, 1.5 * 2.0 ** 4]]))


@pytest.mark.parametrize("case", LC.TAIL_CASES, ids=LC.tail_id)
def test_tail_reference_passes_the_checks(case):
    LC.check_tail_case(case, LC.ref_swiglu_lora, LC.swiglu_plain_ref, CPU)


@pytest.mark.parametrize("rid", [r for r in LC.REFUSALS if r not in LC.GPU_ONLY_REFUSALS])
def test_tail_refusal_cases_build_and_the_contract_refuses_them(rid):
    LC.check_tail_refusal(rid, LC.ref_swiglu_lora, CPU, pytest.raises)


def test_refusal_list_covers_every_operand_rule():
    ids = set(LC.REFUSALS)
    assert ids >= {"T-not-16", "F-not-128", "gu-odd-width", "gu-odd-width-bwd", "nrb-0", "nrb-5", "pad-below-16nrb",
                   "pad-not-8", "v-too-few-rows", "v-wrong-width-fwd", "v-wrong-width-bwd", "v-row-stride-not-8",
                   "dm-wrong-size", "gu-fp16", "v-fp32", "dm-fp32", "gu-on-cpu", "v-on-cpu", "dm-on-cpu"}
    # the hole: an odd width passes F = width / 2, F % 128 == 0
    assert (257 // 2) % 128 == 0 and (513 // 2) % 128 == 0


# =========================================================================== B. the cases
@pytest.mark.parametrize("case", LC.PROJ_CASES, ids=LC.proj_id)
def test_adapter_terms_are_as_large_as_the_base_terms(case):
    d = LC.proj_case(case)
    for a, b in ((d["a0"], d["b0"]), (d["a1"], d["b1"])):
        yw, yl, dxw, dxl = LC.term_rms(d["x"], d["w"], a, b, d["dy"], LC.S_LORA)
        assert yl >= yw and dxl >= dxw and yl > 1.0 and dxl > 0.5, (yw, yl, dxw, dxl)
        assert (yw == 0.0) == case.wzero
        mask = LC.block_mask(case.splits, case.r)
        assert bool((b[~mask] == 0).all()) and bool((b[mask] != 0).float().mean() > 0.99)  # block-diagonal
    assert LC.rms(d["a1"].double() - d["a0"].double()) > LC.rms(d["a0"])  # an update a stale copy cannot pass
    assert bool((d["ga0"] != 0).all()) and bool((d["gb0"] != 0).all())


def test_projection_cases_cover_the_list():
    cs = LC.PROJ_CASES
    assert {c.T for c in cs} == {48, 128, 192} and {c.K for c in cs} == {256}
    assert {(c.splits, c.r) for c in cs} == {((256, 128, 128), 16), ((192,), 32), ((128, 128), 32), ((256,), 64)}
    assert {len(c.splits) * c.r for c in cs} == {32, 48, 64} and any(c.wzero for c in cs)


@pytest.mark.parametrize("case", LC.MLP_CASES, ids=LC.mlp_id)
def test_mlp_adapter_terms_are_as_large_as_the_base_terms(case):
    d = LC.mlp_case(case)
    z = torch.zeros(case.T, 2 * case.F)
    yw, yl, _, _ = LC.term_rms(d["x"], d["wgu"], d["agu"], d["bgu"], z, LC.S_LORA)
    assert yl >= yw > 0
    m = LC.swiglu_plain_ref(None, LC.proj_fwd_model(d["x"], d["wgu"], d["agu"], d["bgu"], LC.S_LORA)[0].to(BF16))
    yw, yl, dxw, dxl = LC.term_rms(m, d["wd"], d["ad"], d["bd"], d["dy"], LC.S_LORA)
    assert yl >= yw > 0 and dxl >= dxw > 0


@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("K,splits,r", LC.GRADS_TAIL_END_CONFIGS)
def test_grads_tail_end_configs_build_and_end_with_the_tail(K, splits, r, acc):
    from tests import test_mfma_exact_gpu as TE
    from tests.test_mfma_inputs import ref_lora_grads

    R = len(splits) * r
    assert R == 64 and r > 16 and 16 * ((len(splits) - 1) * r // 16) + 64 > 64  # the window would leave the tail
    assert TE.grads_case(K, splits, r)[0].shape[1] == K + 64
    TE.check_lora_grads(K, splits, r, acc, ref_lora_grads, CPU)


# --------------------------------------------------------------------------- references, independently
@pytest.mark.parametrize("case", LC.PROJ_CASES, ids=LC.proj_id)
def test_projection_reference_agrees_with_the_two_gemm_formulation(case):
    """mxllm/ops/linear.py ``_LoRALinearFn`` (t = x A^T, y = s t B^T + x W^T and its hand-written backward)
    run in fp64."""
    from mxllm.ops.linear import lora_linear

    d = LC.proj_case(case)
    x, w, a, b, dy = [d[k].double() for k in ("x", "w", "a0", "b0", "dy")]
    x.requires_grad_(True), a.requires_grad_(True), b.requires_grad_(True)
    y = lora_linear(x, w, a, b, case.splits, LC.S_LORA)
    y.backward(dy)
    ry, rdx, rda, rdb = LC.proj_ref64(d["x"], d["w"], d["a0"], d["b0"], d["dy"], LC.S_LORA, case.splits, case.r)
    for got, ref in [(y.detach(), ry), (x.grad, rdx), (a.grad, rda)] + [
            (b.grad[rows, cols], rdb[i]) for i, (rows, cols) in enumerate(LC._blocks(case.splits, case.r))]:
        assert float((got - ref).abs().max()) <= 1e-11 * float(ref.abs().max() + 1)
    assert not b.grad[~LC.block_mask(case.splits, case.r)].any()


@pytest.mark.parametrize("case", LC.MLP_CASES, ids=LC.mlp_id)
def test_mlp_reference_agrees_with_the_chained_closed_forms(case):
    auto, chain = LC.mlp_ref64(case), LC.mlp_ref64_chained(case)
    flat = lambda t: list(t) if isinstance(t, (list, tuple)) else [t]  # noqa: E731
    for got, ref in zip(auto, chain):
        for g, r in zip(flat(got), flat(ref)):
            assert g.shape == r.shape and float((g - r).abs().max()) <= 1e-11 * float(r.abs().max() + 1)


def test_lora_constants_are_the_measured_ones():
    acc = LC.measure()
    assert set(acc) == {"SWIGLU_LORA_TAIL", "LORA_PROJ_Y", "LORA_PROJ_DX", "LORA_PROJ_DA", "LORA_PROJ_DB", "LORA_MLP_Y",
                        "LORA_MLP_DX", "LORA_MLP_DA", "LORA_MLP_DB"}
    for name, (rel, ab) in acc.items():
        assert getattr(P, name + "_MEASURED") == (float(f"{rel:.3g}"), float(f"{ab:.3g}")), name
        assert getattr(P, name) == (max(2 * float(f"{rel:.3g}"), P.ULP_BF16), pytest.approx(2 * ab, rel=5e-3)), name


# --------------------------------------------------------------------------- the CPU path through the checks
@pytest.mark.parametrize("acc", [False, True], ids=["autograd", "accumulate"])
@pytest.mark.parametrize("layout", LC.LAYOUTS)
@pytest.mark.parametrize("case", LC.PROJ_CASES, ids=LC.proj_id)
def test_cpu_projection_meets_the_bounds(case, layout, acc):
    LC.check_projection(case, layout, acc, CPU)


@pytest.mark.parametrize("layout", LC.LAYOUTS)
def test_cpu_projection_after_adapter_update(layout):
    lin = LC.check_projection(LC.PROJ_CASES[0], layout, True, CPU, update=True)
    d, c = LC.proj_case(LC.PROJ_CASES[0]), LC.PROJ_CASES[0]
    N, K, R = sum(c.splits), c.K, len(c.splits) * c.r
    for _, dst in lin.adapter_copies():  # every copy holds the new values
        assert torch.equal(dst, d["a1"]) or torch.equal(dst, d["b1"])
    assert len(lin.adapter_copies()) == {"row": 3, "image": 4, "tr": 4}[layout]
    assert lin.wbuf.shape == ((K + 64, N + 64) if layout == "tr" else (N + 64, K + 64)) and R == 48


@pytest.mark.parametrize("case", LC.MLP_CASES, ids=LC.mlp_id)
def test_cpu_mlp_block_meets_the_bounds(case):
    outs, wrote = LC.run_mlp(case, CPU)
    assert wrote == (False, False)  # the producer-written tails are the HIP kernel's
    LC.check_mlp_outputs(case, outs, f"mlp {LC.mlp_id(case)} cpu")


# =========================================================================== sensitivity
# A correct tensor, one localized defect of the kind a kernel could have, and the matching check must raise.
SENS = next(c for c in LC.TAIL_CASES if not c.bwd and c.nrb == 3 and c.T == 64 and c.F == 640 and c.rbw_req == 2)
ROWS = slice(16, 32)  # the second 16-row block


def _tail_of(out, v, R, extra=None):
    acc = out.float() @ v[:R].float().t()
    if extra is not None:
        acc = acc + extra
    return (LC.S_TAIL * acc).to(BF16)


def _sens_setup(kind, k=0):
    c, R, W = SENS, 16 * SENS.nrb, SENS.F
    gu, dm = LC.tail_inputs(c, "bounded" if kind == "splits" else "gauss")
    out = LC.swiglu_plain_ref(dm, gu)
    if kind == "gauss":
        v, aux = LC.tail_v_gauss(c)[:, :W], None
    elif kind == "onehot":
        buf, aux = LC.tail_v_onehot(c, k)
        v = buf[:, :W]
    else:
        buf, aux = LC.tail_v_splits(c)
        v = buf[:, :W]
    return out, v, R, aux


def _check(kind, tail, out, v, R, aux):
    if kind == "gauss":
        LC.check_tail_parity(tail, out, v, R, "t")
    elif kind == "onehot":
        LC.check_tail_routing(tail, out, aux, "t")
    else:
        LC.check_tail_splits(tail, out, aux, "t")


COL0 = LC.route_columns(SENS, 0)[5]  # a column the one-hot rows select: its chunk, slice and tile get the defects


def _defect(name, out, v, R):
    """The tail a kernel with defect ``name`` would store, from the correct ``out``."""
    q, tile, sl = COL0 // 8, COL0 // 128, COL0 % 128 // 32
    bad = out.clone()
    if name == "wrong-chunk":  # one 8-column chunk of the LDS image read from its neighbour, one row block
        bad[ROWS, 8 * q:8 * q + 8] = out[ROWS, 8 * (q ^ 1):8 * (q ^ 1) + 8]
    elif name == "slices-swapped":  # two waves read each other's 32 columns of one tile
        a, b = 128 * tile + 32 * sl, 128 * tile + 32 * (sl ^ 1)
        bad[ROWS, a:a + 32], bad[ROWS, b:b + 32] = out[ROWS, b:b + 32], out[ROWS, a:a + 32]
    elif name == "tile-dropped":  # a split's range one tile short
        bad[ROWS, 128 * tile:128 * tile + 128] = 0
    elif name == "split-twice":  # the reduce adds split 0 (tiles 0, 1) twice
        t0, t1 = LC.split_ranges(SENS.F // 128, LC.tail_cs(SENS))[0]
        cols = slice(128 * t0, 128 * t1)
        return _tail_of(out, v, R, out[:, cols].float() @ v[:R, cols].float().t())
    elif name == "rank-block-shifted":  # rank block 1 stored where block 2 belongs and back
        t = _tail_of(out, v, R)
        return torch.cat([t[:, :16], t[:, 32:48], t[:, 16:32]], 1)
    elif name == "s-twice":
        return (LC.S_TAIL * _tail_of(out, v, R).float()).to(BF16)
    return _tail_of(bad, v, R)


@pytest.mark.parametrize("kind", ["gauss", "onehot", "splits"])
def test_correct_tail_passes(kind):
    out, v, R, aux = _sens_setup(kind)
    _check(kind, _tail_of(out, v, R), out, v, R, aux)
    assert LC.tail_trips(SENS) == [2, 3]


@pytest.mark.parametrize("kind,name", [
    ("gauss", "wrong-chunk"), ("onehot", "wrong-chunk"), ("gauss", "slices-swapped"), ("onehot", "slices-swapped"),
    ("gauss", "tile-dropped"), ("onehot", "tile-dropped"), ("splits", "tile-dropped"), ("gauss", "split-twice"),
    ("splits", "split-twice"), ("gauss", "rank-block-shifted"), ("onehot", "rank-block-shifted"),
    ("splits", "rank-block-shifted"), ("gauss", "s-twice"), ("onehot", "s-twice"), ("splits", "s-twice")])
def test_tail_checks_reject(kind, name):
    out, v, R, aux = _sens_setup(kind)
    bad = _defect(name, out, v, R)
    localized = name in ("wrong-chunk", "slices-swapped", "tile-dropped")
    with pytest.raises(AssertionError) as e:
        _check(kind, bad, out, v, R, aux)
    if localized and kind != "gauss":  # assert_exact names the box: the corrupted row block
        assert "rows 16..31" in str(e.value), str(e.value)
    if localized:  # and nothing else moved: the same tensor with the row block restored passes
        good = _tail_of(out, v, R)
        assert torch.equal(bad[:16], good[:16]) and torch.equal(bad[32:], good[32:])


def test_nonzero_pad_column_is_rejected():
    out, v, R, _ = _sens_setup("gauss")
    tail = torch.cat([_tail_of(out, v, R), torch.zeros(out.shape[0], 16, dtype=BF16)], 1)
    LC.check_tail_parity(tail, out, v, R, "t")
    tail[40, R + 3] = 2.0 ** -20
    with pytest.raises(AssertionError, match="pad columns"):
        LC.check_tail_parity(tail, out, v, R, "t")


def _proj_model_outputs(c, a_dx=None, s_tail=1.0, acc=False):
    """(y, dx, dA, dB [N, R]) of the fp32 model in bf16 at the updated adapters; ``a_dx``: the A the input
    gradient's image holds; ``s_tail``: a further factor on the stored forward tail."""
    d = LC.proj_case(c)
    a, b = d["a1"], d["b1"]
    y32, t = LC.proj_fwd_model(d["x"], d["w"], a, b, LC.S_LORA)
    if s_tail != 1.0:
        t2 = (s_tail * t.float()).to(BF16)
        y32 = torch.cat([d["x"].float(), t2.float()], 1) @ torch.cat([d["w"].float(), b.float()], 1).t()
    ga0, gb0 = (d["ga0"], d["gb0"]) if acc else (None, None)
    dx32, da32, db32 = LC.proj_bwd_model(d["dy"], d["x"], t, d["w"], a, b, LC.S_LORA, c.splits, c.r, ga0, gb0)
    if a_dx is not None:
        dx32 = LC.proj_bwd_model(d["dy"], d["x"], t, d["w"], a_dx, b, LC.S_LORA, c.splits, c.r)[0]
    db = gb0.clone() if acc else torch.zeros(sum(c.splits), len(c.splits) * c.r, dtype=BF16)
    for i, (rows, cols) in enumerate(LC._blocks(c.splits, c.r)):
        db[rows, cols] = db32[i].to(BF16)
    ref = LC.proj_ref64(d["x"], d["w"], a, b, d["dy"], LC.S_LORA, c.splits, c.r)
    return (y32.to(BF16), dx32.to(BF16), da32.to(BF16), db), ref, (gb0, ga0)


@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("case", LC.PROJ_CASES, ids=LC.proj_id)
def test_projection_model_meets_its_own_bounds(case, acc):
    outs, ref, starts = _proj_model_outputs(case, acc=acc)
    LC.check_proj_outputs(outs, ref, case.splits, case.r, "model", *starts)


def test_projection_checks_reject_a_stale_a_column_block_in_dx():
    c = LC.PROJ_CASES[0]
    d = LC.proj_case(c)
    stale = d["a1"].clone()
    stale[16:32] = d["a0"][16:32]  # rank block 1 of the dX image still holds the previous A
    outs, ref, starts = _proj_model_outputs(c, a_dx=stale)
    with pytest.raises(AssertionError, match="model: dx"):
        LC.check_proj_outputs(outs, ref, c.splits, c.r, "model", *starts)


def test_projection_checks_reject_the_scale_applied_twice():
    c = LC.PROJ_CASES[0]
    outs, ref, starts = _proj_model_outputs(c, s_tail=LC.S_LORA)
    with pytest.raises(AssertionError, match="model: y"):
        LC.check_proj_outputs(outs, ref, c.splits, c.r, "model", *starts)


@pytest.mark.parametrize("acc", [False, True])
def test_projection_checks_reject_a_touched_off_diagonal_block(acc):
    c = LC.PROJ_CASES[0]
    outs, ref, starts = _proj_model_outputs(c, acc=acc)
    db = outs[3].clone()
    # row 300: split 1, column 5: rank block 0; one bf16 ulp of the start value, or 2^-30 on the zero
    db[300, 5] = db[300, 5] * (1.0 + 2.0 ** -7) if acc else 2.0 ** -30
    assert not LC.block_mask(c.splits, c.r)[300, 5]
    with pytest.raises(AssertionError, match=r"off-diagonal.*first at \(300, 5\)"):
        LC.check_proj_outputs(outs[:3] + (db,), ref, c.splits, c.r, "model", *starts)
    if acc:  # an accumulating backward that zero-fills first
        with pytest.raises(AssertionError, match="untouched"):
            LC.check_proj_outputs(outs[:3] + (torch.where(LC.block_mask(c.splits, c.r), outs[3], 0.0).to(BF16),), ref,
                                  c.splits, c.r, "model", *starts)
