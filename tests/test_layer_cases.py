"""The strict transformer-layer tests (tests/test_layer_strict_gpu.py, tests/_layer_cases.py) on the CPU: the
cases are what their module says, the fp64 reference agrees with an independent formulation, the fp32 model
and the project's CPU path pass the very checks (at the very bounds) the HIP routes meet, and ten planted
defects fail them."""
import pytest
import torch

from tests import _layer_cases as LY
from tests import _lora_cases as LC
from tests import _parity as P

BF16, F32 = torch.bfloat16, torch.float32
CPU = torch.device("cpu")
LAYERS = (0, 1)


def _ids(v):
    return LY.case_id(v) if isinstance(v, LY.LayerCase) else None


# =========================================================================== the cases
def test_cases_are_the_smallest_shapes_that_reach_the_code():
    from mxllm.ops import gemm

    cfg = LY.config(LY.FULL_256)
    assert (cfg.hidden, cfg.n_heads, cfg.n_kv_heads, cfg.head_dim, cfg.ffn, cfg.n_layers) == (512, 4, 2, 128, 1024, 2)
    assert LY.config(LY.TINY_192).head_dim == 32
    T = LY.FULL_256.B * LY.FULL_256.S
    # two batch rows inside the GEMM's M, two 256-row tiles; every projection in whole gemm8 tiles
    assert LY.FULL_256.B == 2 and T // 256 == 2 and LY.FULL_256.S % 256 == 0
    for name in LY.PROJS:
        assert gemm.g8_shape_ok(True, True, T, sum(LY.proj_splits(cfg, name)), LY.proj_in(cfg, name))
    # T = 384: no gemm8 launch takes it
    assert not gemm.g8_shape_ok(True, True, LY.FULL_192.B * LY.FULL_192.S, 1024, 512) and LY.FULL_192.S % 256
    assert LY.LORA_256.lora == 16 and LY.LORA_256[:3] == LY.FULL_256[:3]


@pytest.mark.parametrize("case", LY.CASES, ids=_ids)
def test_inputs_make_every_op_matter(case):
    """Norm weights spread over (0.5, 1.5); q, k, v and gu of order one; the softmax neither uniform nor one-hot;
    the LoRA adapter terms as large as the base terms; g0 as large as the gradient it is added to."""
    cfg, ws = LY.config(case), LY.layer_weights(case)
    for w in ws[:2]:
        for g in (w["attn_norm"], w["mlp_norm"], ws[2]):
            assert 0.5 <= float(g.min()) < 0.6 and 1.4 < float(g.max()) <= 1.5
    T, D, Hq, Hkv = case.B * case.S, cfg.head_dim, cfg.n_heads, cfg.n_kv_heads
    for i in LAYERS:
        io, w = LY.layer_io(case, i), ws[i]
        h = (io["d"].double() + io["h"].double())
        x = LY._rms(h, w["attn_norm"].double(), cfg.norm_eps)
        qkv = x @ w["wqkv"].double().t()
        if case.lora:
            yw, yl, _, _ = LC.term_rms(x, w["wqkv"], w["wqkv_a"], w["wqkv_b"], torch.zeros(T, qkv.shape[1]), LY.S_LORA)
            assert 0.8 * yw <= yl <= 1.25 * yw, (yw, yl)
            qkv = qkv + LY.S_LORA * (x @ w["wqkv_a"].double().t()) @ w["wqkv_b"].double().t()
        assert 0.7 < LC.rms(qkv) < 2.0
        q = qkv[:, :Hq * D].view(case.B, case.S, Hq, D).transpose(1, 2)
        k = qkv[:, Hq * D:(Hq + Hkv) * D].view(case.B, case.S, Hkv, D).transpose(1, 2)
        s = (q @ k.repeat_interleave(Hq // Hkv, 1).transpose(-1, -2)) / D ** 0.5
        vis = torch.arange(case.S).view(1, -1) <= torch.arange(case.S).view(-1, 1)
        # the largest probability of the rows that see at least S / 2 keys
        pmax = torch.softmax(s.masked_fill(~vis, float("-inf")), -1).amax(-1)[..., case.S // 2:]
        assert float(pmax.median()) > 4.0 / case.S and float(pmax.median()) < 0.7, float(pmax.median())
        ref, g0 = LY.layer_ref64(case, i), LY.start_grads(case, i)
        for key in LY.grad_keys(case):
            assert 0.9 < LC.rms(g0[key]) / LC.rms(ref[key]) < 1.1 and bool((g0[key] != 0).float().mean() > 0.99), key
        assert LC.rms(ref["dd"]) > 0.5 and LC.rms(ref["x2"]) > 0.5


def test_defect_list_is_the_ten_of_the_issue():
    assert len(LY.DEFECTS) == len(set(LY.DEFECTS)) == 10 and set(DEFECT_HITS) == set(LY.DEFECTS)


# =========================================================================== the reference, independently
@pytest.mark.parametrize("i", LAYERS)
@pytest.mark.parametrize("case", LY.CASES, ids=_ids)
def test_reference_agrees_with_the_fp32_cpu_path(case, i, monkeypatch):
    """The project's reference ops (mxllm/ops/reference.py) and its own autograd functions on fp32 parameters
    holding the same values -- another formulation of the same function (torch's softmax attention, the
    hand-written backward of ``_LinearFn`` / ``_LoRAAugFn``): fp32 arithmetic away from ``layer_ref64``."""
    log = LY.apply_route(monkeypatch, "default", case, CPU)
    m = LY.build_model(case, CPU, F32)
    x2, h2, dd = LY.run_layer(m, case, i, CPU)
    (q, k), = [info for name, info in log if name == "attn_in"]
    got = {"x2": x2, "h2": h2, "dd": dd, "q": q.detach(), "k": k.detach()}
    got.update({k: p.grad for k, p in LY.layer_params(m, case, i).items()})
    ref = LY.layer_ref64(case, i)
    for key, r in ref.items():
        if key == "h2" and i == 1:
            continue
        g = got[key].detach().double()
        if case.lora and key.startswith("db_"):
            mask = LC.block_mask(LY.proj_splits(LY.config(case), "w" + key[3:]), case.lora)
            assert not bool(g[~mask].any())
            g, r = g * mask, r * mask
        err = float(((g - r).abs() / r.abs().amax(-1, keepdim=True)).max())
        assert err < 1e-4, (key, err)


# =========================================================================== the model and the CPU path
def _model_outputs(case, i, target, defect=None):
    return LY.round_outputs(case, target, LY.expected(case, i, target, LY.layer_model32, defect))


CASE_TARGETS = [(c, t) for c in LY.CASES for t in (LY.TARGETS if not c.lora else ("autograd",))]


@pytest.mark.parametrize("i", LAYERS)
@pytest.mark.parametrize("case,target", CASE_TARGETS, ids=[f"{LY.case_id(c)}-{t}" for c, t in CASE_TARGETS])
def test_model_meets_its_own_bounds(case, target, i):
    LY.check_outputs(case, i, target, _model_outputs(case, i, target), "model")


@pytest.mark.parametrize("i", LAYERS)
@pytest.mark.parametrize("case,target", CASE_TARGETS, ids=[f"{LY.case_id(c)}-{t}" for c, t in CASE_TARGETS])
def test_cpu_path_meets_the_bounds(case, target, i, monkeypatch):
    """The same ``_layer`` on CPU tensors (reference ops in bf16) through ``check_layer``: bounds, targets,
    gradient-ready notifications, twice the same bits."""
    LY.check_layer(case, "lora-unfused" if case.lora else "default", target, CPU, monkeypatch, i)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("i", LAYERS)
@pytest.mark.parametrize("route", ["rec", "rec-keep-x"])
def test_cpu_recompute_routes_meet_the_bounds(route, i, dtype, monkeypatch):
    """``normed_linear`` / ``swiglu_linear`` on the CPU (x and m rebuilt in the backward), bf16 and fp32 parameters."""
    for target in ("autograd", "attached"):
        LY.check_layer(LY.FULL_192, route, target, CPU, monkeypatch, i, dtype)


# =========================================================================== planted defects
# defect -> (target, layer, the outputs that must fail; every other output must still pass where the defect
# does not reach it)
DEFECT_HITS = {
    "rope-runs-on": ("autograd", 0, {"q", "k"}),
    "mask-off-by-one": ("autograd", 0, {"x2", "h2", "dd", "dw_qkv", "dw_o"}),
    "dw-qkv-from-h": ("autograd", 0, {"dw_qkv"}),
    "no-residual-grad": ("autograd", 0, {"dd"}),
    "dgamma-mlp-short": ("autograd", 0, {"dg_mlp"}),
    "dgu-tile-zero": ("autograd", 0, {"dw_gu", "dd"}),
    "dwd-halves-swapped": ("autograd", 0, {"dw_d"}),
    "next-gamma-missing": ("autograd", 1, {"x2", "dg_next"}),
    "fresh-added": ("fresh", 0, set(LY.FULL_GRADS)),
    "fp32x2-overwritten": ("fp32x2", 0, set(LY.FULL_GRADS)),
}
LOCAL = {"dw-qkv-from-h", "no-residual-grad", "dgamma-mlp-short", "dwd-halves-swapped", "fresh-added",
         "fp32x2-overwritten"}  # defects that touch nothing but the outputs listed


@pytest.mark.parametrize("defect", LY.DEFECTS)
def test_planted_defect_is_rejected(defect):
    """Each defect is applied to the fp32 model -- which passes without it (test_model_meets_its_own_bounds) --
    and the same check at the same inputs must reject every output the defect reaches."""
    case = LY.FULL_256
    target, i, hits = DEFECT_HITS[defect]
    outs = _model_outputs(case, i, target, defect)
    good = _model_outputs(case, i, target)
    with pytest.raises(AssertionError):
        LY.check_outputs(case, i, target, outs, defect)
    for key in hits:  # each one alone: the good outputs with this one replaced
        with pytest.raises(AssertionError, match=key):
            LY.check_outputs(case, i, target, dict(good, **{key: outs[key]}), defect)
    if defect in LOCAL:
        for key in set(good) - hits:
            assert torch.equal(outs[key], good[key]), key
    if defect == "rope-runs-on":
        # RoPE is relative: the same shift of q's and k's positions within a batch row changes no score, so every
        # other output of the layer stays within its bound -- only q and k themselves show the defect
        LY.check_outputs(case, i, target, dict(outs, q=good["q"], k=good["k"]), defect)
        assert torch.equal(outs["q"][0], good["q"][0]) and not torch.equal(outs["q"][1], good["q"][1])


def test_dgu_tile_defect_is_named_by_its_rows():
    """The zero tile is rows 256..511, the second batch row: the first batch row's gradient of d_prev is untouched
    (the attention mixes tokens of one batch row only) and the message's worst element lies in the second."""
    case = LY.FULL_256
    outs, good = _model_outputs(case, 0, "autograd", "dgu-tile-zero"), _model_outputs(case, 0, "autograd")
    with pytest.raises(AssertionError) as e:
        LY.check_outputs(case, 0, "autograd", dict(good, dd=outs["dd"]), "t")
    worst = int(str(e.value).split("worst at (")[1].split(",")[0])
    assert worst >= 256, str(e.value)
    assert torch.equal(outs["dd"][:256], good["dd"][:256])  # the first batch row never sees the second


# =========================================================================== the whole model
@pytest.mark.parametrize("tied", [False, True], ids=["untied", "tied"])
def test_whole_model_inputs_and_model(tied):
    ids, labels, emb, head = LY.model_inputs(tied)
    assert tuple(ids.shape) == (2, 256) and (head is None) == tied
    assert 0.2 < float((ids == LY.REPEATED_ID).float().mean()) < 0.3
    assert 0.05 < float((labels == LY.IGNORE).float().mean()) < 0.15
    ref = LY.model_ref64(tied)
    assert 5.0 < float(ref["loss"]) < 9.0  # near log V = 6.2: logits of order one
    if not tied:  # rows of ids the batch never uses have no gradient, exactly
        unused = torch.ones(emb.shape[0], dtype=torch.bool)
        unused[ids.reshape(-1)] = False
        assert bool(unused.any()) and not bool(ref["demb"][unused].any())
    LY.check_model_outputs(tied, LY.round_model_outputs(LY.model_model32(tied)), "model")


@pytest.mark.parametrize("ckpt", LY.CKPT_SETTINGS, ids=lambda v: f"ckpt-{v}")
@pytest.mark.parametrize("tied", [False, True], ids=["untied", "tied"])
def test_cpu_whole_model_meets_the_bounds(tied, ckpt, monkeypatch):
    LY.check_whole_model(tied, ckpt, CPU, monkeypatch)


@pytest.mark.parametrize("defect,tied,hits", [
    ("tied-embedding-use-dropped", True, {"demb"}),
    ("ignored-labels-counted", False, {"loss", "demb", "dhead", "dg_final"}),
    ("n-valid-plus-two", True, {"loss"}),  # 0.4 % of the loss; the bf16 gradients move by less than an ulp
    ("ckpt-layer-dw-missing", False, {"l0." + k for k in LY.MODEL_LAYER_KEYS}),
    ("ckpt-layer-dw-doubled", False, {"l0." + k for k in LY.MODEL_LAYER_KEYS})])
def test_whole_model_checks_reject(defect, tied, hits):
    outs, good = [LY.round_model_outputs(LY.model_model32(tied, d)) for d in (defect, None)]
    for key in hits:
        with pytest.raises(AssertionError, match=key):
            LY.check_model_outputs(tied, dict(good, **{key: outs[key]}), defect)


# =========================================================================== the constants
def test_measured_constants_are_current():
    acc = dict(LY.measure(), **LY.measure_model())
    want = {"MODEL_LOSS", "MODEL_DEMB", "MODEL_DEMB_TIED", "MODEL_DHEAD", "MODEL_DG_FINAL"}
    want |= {"MODEL_" + k.upper() for k in LY.MODEL_LAYER_KEYS}
    want |= {"LAYER_X2", "LAYER_H2", "LAYER_Q", "LAYER_K", "LAYER_DD"}
    want |= {"LAYER_" + k.upper() + s for k in LY.FULL_GRADS for s in ("", "_F32")}
    want |= {"LAYER_LORA_" + k for k in ("X2", "H2", "Q", "K", "DD") + tuple(g.upper() for g in LY.LORA_GRADS)}
    assert set(acc) == want
    for name, (rel, ab) in acc.items():
        ulp = P.ULP_F32 if name.endswith("_F32") or name in LY.F32_OUTPUTS else P.ULP_BF16
        assert getattr(P, name + "_MEASURED") == (float(f"{rel:.3g}"), float(f"{ab:.3g}")), name
        assert getattr(P, name) == (max(2 * float(f"{rel:.3g}"), ulp), pytest.approx(2 * ab, rel=5e-3)), name
