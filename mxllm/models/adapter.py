"""LoRA adapters as PEFT directories (``adapter_config.json`` + ``adapter_model.safetensors``), so an
adapter trained here moves to any Hugging Face tool and back without the base weights.

Tensor names: ``base_model.model.model.layers.{i}.self_attn.q_proj.lora_A.weight`` [r, in] and
``...lora_B.weight`` [out, r]; projection names and the layer mapping are those of
``mxllm/models/hf.py``.  mxllm stacks the splits' A matrices in ``FusedLinear.lora_a`` and keeps a
block-diagonal ``lora_b``; ``save_adapter`` cuts both per Hugging Face projection.  ``peft`` itself is
never imported.

``load_adapter`` returns ``{"r", "alpha", "scaling", "weights": {(layer, projection): (A, B)}}``,
what ``AdapterTables.put`` (mxllm/ops/lora_serve.py) and ``Engine.load_adapter`` take.
"""
from __future__ import annotations

import json
import math
import os

import torch

from .config import LlamaConfig

CONFIG_NAME = "adapter_config.json"
WEIGHTS_NAME = "adapter_model.safetensors"
# Hugging Face projection -> (module path in the checkpoint, mxllm FusedLinear, split index)
PROJECTIONS = {
    "q_proj": ("self_attn", "wqkv", 0), "k_proj": ("self_attn", "wqkv", 1), "v_proj": ("self_attn", "wqkv", 2),
    "o_proj": ("self_attn", "wo", 0), "gate_proj": ("mlp", "wgu", 0), "up_proj": ("mlp", "wgu", 1),
    "down_proj": ("mlp", "wd", 0),
}


def _key(i: int, proj: str, which: str) -> str:
    return f"base_model.model.model.layers.{i}.{PROJECTIONS[proj][0]}.{proj}.lora_{which}.weight"


def proj_shape(cfg: LlamaConfig, proj: str) -> tuple[int, int]:
    """(out, in) of a Hugging Face projection."""
    return {"q_proj": (cfg.q_dim, cfg.hidden), "k_proj": (cfg.kv_dim, cfg.hidden), "v_proj": (cfg.kv_dim, cfg.hidden),
            "o_proj": (cfg.hidden, cfg.q_dim), "gate_proj": (cfg.ffn, cfg.hidden), "up_proj": (cfg.ffn, cfg.hidden),
            "down_proj": (cfg.hidden, cfg.ffn)}[proj]


@torch.no_grad()
def adapter_state_dict(model) -> tuple[dict, int, float]:
    """(PEFT-named tensors on the host, r, alpha) of a LoRA ``Llama``.  Raises if an
    off-diagonal block of a ``lora_b`` is non-zero: PEFT has no place for it."""
    sd, r, alpha = {}, 0, 0.0
    for i, layer in enumerate(model.layers):
        for proj, (_, lin_name, si) in PROJECTIONS.items():
            lin = getattr(layer, lin_name)
            if getattr(lin, "lora_r", 0) <= 0:
                raise ValueError(f"layers.{i}.{lin_name} has no LoRA adapter")
            r, alpha = lin.lora_r, lin.scaling * lin.lora_r
            off = sum(lin.splits[:si])
            n = lin.splits[si]
            rows = lin.lora_b.detach()[off:off + n]
            if si == 0:  # once per FusedLinear: everything outside the diagonal blocks must be zero
                mask = torch.ones_like(lin.lora_b, dtype=torch.bool)
                o = 0
                for k, nk in enumerate(lin.splits):
                    mask[o:o + nk, k * r:(k + 1) * r] = False
                    o += nk
                if bool((lin.lora_b.detach()[mask] != 0).any()):
                    raise ValueError(f"layers.{i}.{lin_name}.lora_b has a non-zero off-diagonal block: "
                                     "not expressible as per-projection PEFT adapters")
            sd[_key(i, proj, "A")] = lin.lora_a.detach()[si * r:(si + 1) * r].to("cpu").contiguous()
            sd[_key(i, proj, "B")] = rows[:, si * r:(si + 1) * r].to("cpu").contiguous()
    return sd, r, alpha


def save_adapter(model, path: str) -> str:
    """Write the LoRA adapter of ``model`` (an mxllm LoRA ``Llama``, or the dict ``load_adapter``
    returns) as a PEFT directory.  Returns ``path``."""
    from safetensors.torch import save_file

    if isinstance(model, dict):
        r, alpha = int(model["r"]), float(model["alpha"])
        extra = {k: model[k] for k in ("use_rslora",) if k in model}
        sd = {}
        for (i, proj), (A, B) in sorted(model["weights"].items()):
            sd[_key(i, proj, "A")] = A.detach().to("cpu").contiguous()
            sd[_key(i, proj, "B")] = B.detach().to("cpu").contiguous()
        targets = sorted({p for _, p in model["weights"]})
    else:
        sd, r, alpha = adapter_state_dict(model)
        extra, targets = {}, sorted(PROJECTIONS)
    os.makedirs(path, exist_ok=True)
    cfg = {"peft_type": "LORA", "task_type": "CAUSAL_LM", "r": r, "lora_alpha": alpha, "lora_dropout": 0.0,
           "target_modules": targets, "bias": "none", "fan_in_fan_out": False, "use_rslora": False, "use_dora": False,
           "modules_to_save": None, "inference_mode": True, "base_model_name_or_path": None}
    cfg.update(extra)
    with open(os.path.join(path, CONFIG_NAME), "w") as f:
        json.dump(cfg, f, indent=2, sort_keys=True)
    save_file(sd, os.path.join(path, WEIGHTS_NAME), metadata={"format": "pt"})
    return path


def load_adapter(path: str, cfg: LlamaConfig, r_max: int | None = None, dtype=torch.bfloat16) -> dict:
    """Read a PEFT LoRA directory for the model ``cfg``.  Any subset of the seven projections
    (the others stay absent = zero); ``use_rslora`` scales by alpha / sqrt(r).  Raises ``ValueError``
    for DoRA, ``modules_to_save``, a bias other than "none", unknown target modules, tensors of the
    wrong shape and a rank above ``r_max`` (the serving table's)."""
    from safetensors import safe_open

    with open(os.path.join(path, CONFIG_NAME)) as f:
        ac = json.load(f)
    if ac.get("peft_type") != "LORA":
        raise ValueError(f"{path}: peft_type {ac.get('peft_type')!r}, only LORA adapters are supported")
    if ac.get("use_dora"):
        raise ValueError(f"{path}: DoRA adapters (use_dora) are not supported")
    if ac.get("modules_to_save"):
        raise ValueError(f"{path}: modules_to_save {ac['modules_to_save']} is not supported (adapter weights only)")
    if ac.get("bias", "none") != "none":
        raise ValueError(f"{path}: bias {ac['bias']!r} is not supported (bias must be \"none\")")
    if ac.get("fan_in_fan_out"):
        raise ValueError(f"{path}: fan_in_fan_out adapters are not supported")
    targets = ac.get("target_modules") or []
    if isinstance(targets, str):
        raise ValueError(f"{path}: target_modules must be a list of projection names, got {targets!r}")
    unknown = sorted(set(targets) - set(PROJECTIONS))
    if unknown:
        raise ValueError(f"{path}: unknown target modules {unknown}; supported: {sorted(PROJECTIONS)}")
    r, alpha = int(ac["r"]), float(ac["lora_alpha"])
    if r < 1:
        raise ValueError(f"{path}: rank {r}")
    if r_max is not None and r > r_max:
        raise ValueError(f"{path}: adapter rank {r} exceeds the table's rank {r_max}")
    if ac.get("rank_pattern") or ac.get("alpha_pattern"):
        raise ValueError(f"{path}: rank_pattern / alpha_pattern are not supported (one rank per adapter)")
    rs = bool(ac.get("use_rslora"))
    weights, seen = {}, set()
    with safe_open(os.path.join(path, WEIGHTS_NAME), framework="pt", device="cpu") as h:
        keys = set(h.keys())
        for i in range(cfg.n_layers):
            for proj in PROJECTIONS:
                ka, kb = _key(i, proj, "A"), _key(i, proj, "B")
                if ka not in keys and kb not in keys:
                    continue
                if ka not in keys or kb not in keys:
                    raise ValueError(f"{path}: layer {i} {proj} has only one of lora_A / lora_B")
                if proj not in targets:
                    raise ValueError(f"{path}: tensors for {proj}, which target_modules does not list")
                A, B = h.get_tensor(ka), h.get_tensor(kb)
                n_out, n_in = proj_shape(cfg, proj)
                if tuple(A.shape) != (r, n_in) or tuple(B.shape) != (n_out, r):
                    raise ValueError(f"{path}: layer {i} {proj}: lora_A {tuple(A.shape)} / lora_B {tuple(B.shape)}, "
                                     f"expected {(r, n_in)} / {(n_out, r)}")
                weights[(i, proj)] = (A.to(dtype), B.to(dtype))
                seen.update((ka, kb))
        extra = sorted(keys - seen)
        if extra:
            raise ValueError(f"{path}: unexpected tensors {extra[:4]}{' ...' if len(extra) > 4 else ''}")
    out = {"r": r, "alpha": alpha, "scaling": alpha / math.sqrt(r) if rs else alpha / r, "weights": weights}
    if rs:
        out["use_rslora"] = True
    return out


@torch.no_grad()
def apply_adapter_(model, adapter: dict) -> None:
    """Copy ``adapter`` into the LoRA parameters of ``model`` (same rank; absent projections zero)."""
    for i, layer in enumerate(model.layers):
        for proj, (_, lin_name, si) in PROJECTIONS.items():
            lin = getattr(layer, lin_name)
            r = lin.lora_r
            if r != adapter["r"]:
                raise ValueError(f"model rank {r}, adapter rank {adapter['r']}")
            off, n = sum(lin.splits[:si]), lin.splits[si]
            A, B = adapter["weights"].get((i, proj)) or (0.0, 0.0)
            lin.lora_a[si * r:(si + 1) * r] = A
            lin.lora_b[off:off + n, si * r:(si + 1) * r] = B
    model.sync_adapters_()
