"""Per-row LoRA adapters for serving: one copy of the base weights, a table of adapters, and every
row of a batch adds the delta of the adapter it names (csrc/kernels/lora_serve.hip).

Tables of one projection (``ProjTables``; all slots allocated once, ranks below ``r_max`` zero-padded):

  a  bf16 [n_adapters, n_splits * r_max, K]   the splits' A matrices stacked (as ``FusedLinear.lora_a``)
  b  bf16 [n_adapters, N, r_max]              row n: the r_max columns of n's own split (B is block-diagonal)
  s  f32  [n_adapters]                        alpha / r (``scales``: the same numbers on the host)

``lora_delta_rows_(y, x, ids, tables)`` computes, for every row b whose ``ids[b]`` is not -1,

  partial[c][b, j] = sum over the c-th 512 columns k of x[b, k] * A[id, j, k]            (fp32)
  t[b, j]          = partial[0][b, j] + partial[1][b, j] + ...                            (fp32, ascending c)
  y[b, n]          = bf16(f32(y[b, n]) + s[id] * sum_j t[b, i * r_max + j] * B[id, n, j])   (i = n's split, ascending j)

and leaves the other rows alone.  Three paths: the two HIP kernels (GPU decode rows), the library
GEMMs over runs of tokens that share an adapter (GPU prefill, ``segments``) and the PyTorch
expression of the formula above (CPU: the numerics oracle of the kernels, computed row by row so a
row's result does not depend on the batch it is in).
"""
from __future__ import annotations

from dataclasses import dataclass, field

import torch

from ._ext import native, use_native

K_CHUNK = 512  # columns of one shrink partial (kLsChunk in lora_serve.hip)
RANKS = (8, 16, 32, 64)
# mxllm projection -> its Hugging Face projections, in row order (mxllm/models/hf.py)
PROJ_SPLITS = {"wqkv": ("q_proj", "k_proj", "v_proj"), "wo": ("o_proj",), "wgu": ("gate_proj", "up_proj"),
               "wd": ("down_proj",)}


def k_splits(K: int) -> int:
    return (K + K_CHUNK - 1) // K_CHUNK


@dataclass
class ProjTables:
    a: torch.Tensor
    b: torch.Tensor
    s: torch.Tensor
    splits: list
    r_max: int
    ws: torch.Tensor  # f32 partials workspace, shared by every projection of the engine
    scales: list = field(default_factory=list)  # s on the host: the prefill path must not sync

    @property
    def n_adapters(self) -> int:
        return self.a.shape[0]

    @property
    def K(self) -> int:
        return self.a.shape[2]

    def partials(self, M: int) -> torch.Tensor:
        """The [KS, M, R] view of the workspace a call over M rows uses."""
        KS, R = k_splits(self.K), self.a.shape[1]
        if KS * M * R > self.ws.numel():
            raise ValueError(f"lora_delta_rows_: {M} rows need {KS * M * R} workspace floats, {self.ws.numel()} allocated")
        return self.ws[:KS * M * R].view(KS, M, R)


def make_proj_tables(n_adapters: int, K: int, splits, r_max: int, device, max_rows: int,
                     ws: torch.Tensor | None = None, dtype=torch.bfloat16) -> ProjTables:
    if r_max not in RANKS:
        raise ValueError(f"the adapter table rank must be one of {RANKS}, got {r_max}")
    if n_adapters < 1 or K % 8 or any(n % 8 or n <= 0 for n in splits) or not 1 <= len(splits) <= 3:
        raise ValueError(f"adapter tables need K % 8 == 0 and 1..3 splits that are multiples of 8 (K {K}, splits {splits})")
    R = len(splits) * r_max
    if ws is None:
        ws = torch.zeros(k_splits(K) * max_rows * R, dtype=torch.float32, device=device)
    return ProjTables(torch.zeros(n_adapters, R, K, dtype=dtype, device=device),
                      torch.zeros(n_adapters, sum(splits), r_max, dtype=dtype, device=device),
                      torch.zeros(n_adapters, dtype=torch.float32, device=device), list(splits), r_max, ws,
                      [0.0] * n_adapters)


class AdapterTables:
    """The adapter tables of every layer and projection of one engine (``layers[i][proj]`` with proj
    in wqkv / wo / wgu / wd) and the partials workspace they share.  Static buffers: ``put`` and
    ``clear`` write into them, so a captured graph that reads them stays valid."""

    def __init__(self, cfg, n_adapters: int, r_max: int, device, max_rows: int, dtype=torch.bfloat16):
        self.cfg, self.n_adapters, self.r_max = cfg, n_adapters, r_max
        self.shapes = {"wqkv": (cfg.hidden, [cfg.q_dim, cfg.kv_dim, cfg.kv_dim]), "wo": (cfg.q_dim, [cfg.hidden]),
                       "wgu": (cfg.hidden, [cfg.ffn, cfg.ffn]), "wd": (cfg.ffn, [cfg.hidden])}
        need = max(k_splits(K) * max_rows * len(sp) * r_max for K, sp in self.shapes.values())
        self.ws = torch.zeros(need, dtype=torch.float32, device=device)
        self.layers = [{p: make_proj_tables(n_adapters, K, sp, r_max, device, max_rows, self.ws, dtype)
                        for p, (K, sp) in self.shapes.items()} for _ in range(cfg.n_layers)]

    def nbytes(self) -> int:
        return sum(t.a.numel() * 2 + t.b.numel() * 2 for lay in self.layers for t in lay.values())

    @torch.no_grad()
    def put(self, index: int, adapter) -> None:
        """Copy ``adapter`` (mxllm/models/adapter.py ``load_adapter``: r, scaling and
        weights[(layer, hf projection)] = (A [r, in], B [out, r]); absent projections are zero) into
        slot ``index``."""
        if not 0 <= index < self.n_adapters:
            raise ValueError(f"adapter slot {index} outside [0, {self.n_adapters})")
        r = int(adapter["r"])
        if not 1 <= r <= self.r_max:
            raise ValueError(f"adapter rank {r} exceeds the table's rank {self.r_max}")
        self.clear(index)
        for i, lay in enumerate(self.layers):
            for proj, names in PROJ_SPLITS.items():
                t, off = lay[proj], 0
                for si, (hf, n) in enumerate(zip(names, t.splits)):
                    w = adapter["weights"].get((i, hf))
                    if w is not None:
                        A, B = w
                        if tuple(A.shape) != (r, t.K) or tuple(B.shape) != (n, r):
                            raise ValueError(f"layer {i} {hf}: lora_A {tuple(A.shape)} / lora_B {tuple(B.shape)}, "
                                             f"expected {(r, t.K)} / {(n, r)}")
                        t.a[index, si * t.r_max:si * t.r_max + r].copy_(A)
                        t.b[index, off:off + n, :r].copy_(B)
                    off += n
                t.s[index] = float(adapter["scaling"])
                t.scales[index] = float(adapter["scaling"])

    @torch.no_grad()
    def clear(self, index: int) -> None:
        for lay in self.layers:
            for t in lay.values():
                t.a[index].zero_()
                t.b[index].zero_()
                t.s[index] = 0.0
                t.scales[index] = 0.0


def merge_segments(adapters) -> list:
    """Per-token adapter indices (-1 = none) -> [(start, end, adapter)] runs, neighbours merged."""
    out = []
    for i, a in enumerate(adapters):
        if out and out[-1][2] == a:
            out[-1] = (out[-1][0], i + 1, a)
        else:
            out.append((i, i + 1, a))
    return out


def _row_delta_(y: torch.Tensor, x: torch.Tensor, b: int, aid: int, t: ProjTables) -> None:
    """The formula of the module docstring for one row (fp32 PyTorch)."""
    K = t.K
    xr, A = x[b].float(), t.a[aid].float()
    acc = None
    for c in range(0, K, K_CHUNK):
        p = A[:, c:c + K_CHUNK] @ xr[c:c + K_CHUNK]
        acc = p if acc is None else acc + p
    Bm, s = t.b[aid].float(), t.s[aid].float()
    off = 0
    for i, n in enumerate(t.splits):
        d = Bm[off:off + n] @ acc[i * t.r_max:(i + 1) * t.r_max]
        y[b, off:off + n] = (y[b, off:off + n].float() + s * d).to(y.dtype)
        off += n


def lora_gather_shrink(x: torch.Tensor, ids: torch.Tensor, t: ProjTables) -> torch.Tensor:
    part = t.partials(x.shape[0])
    native().lora_gather_shrink(x, ids, t.a, part)
    return part


def lora_gather_expand_add_(y: torch.Tensor, part: torch.Tensor, ids: torch.Tensor, t: ProjTables) -> torch.Tensor:
    native().lora_gather_expand_add_(y, part, ids, t.b, t.s, t.splits, t.K)
    return y


@torch.no_grad()
def lora_delta_rows_(y: torch.Tensor, x: torch.Tensor, ids: torch.Tensor | None, t: ProjTables, *,
                     segments=None) -> torch.Tensor:
    """y [M, N] += each row's adapter delta of x [M, K], in place (module docstring).

    ``ids`` int32 [M] on y's device (-1 = no adapter; values below n_adapters: the caller checks
    them where it builds them).  ``segments``: host list of (start, end, adapter) runs over the
    rows (prefill); ``ids`` is then not needed."""
    if y.dim() != 2 or x.dim() != 2 or x.shape[0] != y.shape[0]:
        raise ValueError(f"lora_delta_rows_: y {tuple(y.shape)} and x {tuple(x.shape)} must be [M, N] and [M, K]")
    if x.shape[1] != t.K or y.shape[1] != sum(t.splits):
        raise ValueError(f"lora_delta_rows_: x / y widths {x.shape[1]} / {y.shape[1]}, the tables hold "
                         f"{t.K} / {sum(t.splits)}")
    if not use_native(y):
        if segments is not None:
            rows = [(b, a) for s, e, a in segments for b in range(s, e) if a >= 0]
        else:
            rows = [(b, a) for b, a in enumerate(ids.tolist()) if a >= 0]
        for b, a in rows:
            if a >= t.n_adapters:
                raise ValueError(f"adapter index {a} outside the table of {t.n_adapters}")
            _row_delta_(y, x, b, a, t)
        return y
    if segments is not None:
        # prefill: runs of tokens on one adapter through the library GEMMs; s from the host copy
        for s, e, a in segments:
            if a < 0:
                continue
            if not (0 <= s < e <= y.shape[0] and a < t.n_adapters):
                raise ValueError(f"lora_delta_rows_: bad segment {(s, e, a)}")
            xs, off = x[s:e], 0
            for i, n in enumerate(t.splits):
                u = xs @ t.a[a, i * t.r_max:(i + 1) * t.r_max].t()
                y[s:e, off:off + n].addmm_(u, t.b[a, off:off + n].t(), alpha=t.scales[a])
                off += n
        return y
    if x.stride(1) != 1 or x.stride(0) % 8:
        x = x.contiguous()
    part = lora_gather_shrink(x, ids, t)
    return lora_gather_expand_add_(y, part, ids, t)
