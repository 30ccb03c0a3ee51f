"""GEMM dispatch between the hand-written 8-phase MFMA kernel (csrc/kernels/gemm8.hip) and
hipBLASLt / rocBLAS (``torch.mm`` with the tuned solution table, mxllm/utils/gemm_tuning.py).

Every training GEMM of a Llama step is one of four operand orders over row-major bf16 storage:

  form  A stored   B stored   computes          used for
  tn    [M][K]     [N][K]     A @ B^T           forward  y = x W^T
  nn    [M][K]     [K][N]     A @ B             input gradient  dX = dY W
  tt    [K][M]     [K][N]     A^T @ B           weight gradient dW = dY^T X (token-major operands)
  nt    [K][M]     [N][K]     A^T @ B^T         (unused; for completeness)

``gemm8`` is selected per (form, M, N, K, output dtype) only where it was measured faster
(entries with ``tail``: the tail-balanced launch, ``mx_gemm8_tail`` -- a last wave of at most half
the CUs runs as twice as many half-K workgroups, e.g. the 16 x 40-tile 70B qkv forward)
(``mxllm/tuning/gemm8_gfx950.json``, written from ``bench/gemm8_probe.py`` runs), or for every
shape it takes in deterministic mode (``MXLLM_DETERMINISTIC=1``: one workgroup per output tile,
a fixed K order, no split-K or atomics — the step is bitwise reproducible; vendor stream-K
solutions are not, archive/profiles/r3aa).  ``MXLLM_GEMM8=0`` disables it, ``=all`` forces it wherever
it takes the shape (A/B runs).
"""
from __future__ import annotations

import json
import os

import torch

from ._ext import native, use_native

_TABLE_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tuning",
                           "gemm8_gfx950.json")
_TABLE: dict | None = None


def deterministic() -> bool:
    return os.environ.get("MXLLM_DETERMINISTIC", "0") == "1"


_TAIL: dict = {}


def _table() -> dict:
    global _TABLE
    if _TABLE is None:
        _TABLE = {}
        try:
            with open(_TABLE_PATH) as f:
                for e in json.load(f).get("wins", []):
                    key = (e["form"], e["M"], e["N"], e["K"], e["out"])
                    _TABLE[key] = int(e.get("ph", 8))
                    if e.get("tail"):
                        _TAIL[key] = int(e["tail"])
        except (OSError, ValueError, KeyError):
            pass
    return _TABLE


CUS = 256  # MI355X compute units: one gemm8 workgroup (256 x 256 tile) per CU at a time


def tail_split(M: int, N: int, K: int) -> int:
    """Split of the tail-balanced launch (mx_gemm8_tail), 0 if it does not apply: the tile grid leaves
    a last wave of at most half the CUs.  > 0: split at that COLUMN (whole waves of tiles in columns
    [0, N1)); < 0: split at ROW -value (when no column split gives whole waves)."""
    if M % 256 or N % 256 or K < 128:
        return 0
    nM, nN = M // 256, N // 256
    r = (nM * nN) % CUS
    if r == 0 or r > CUS // 2:
        return 0
    full = nM * nN - r
    if full % nM == 0 and 0 < full // nM < nN:
        return full // nM * 256
    if full % nN == 0 and 0 < full // nN < nM:
        return -(full // nN * 256)
    return 0


def _multi_rank() -> bool:
    """True in a process group of more than one rank.  The persistent gemm8 (table ``ph`` 5) gives
    each of its one-per-CU workgroups a FIXED share of the tiles; a collective kernel that holds CUs
    for its whole duration (RCCL's channels, the peer collectives) then delays the workgroups that
    cannot start, and with them the whole GEMM -- under ZeRO-3's reduce-scatters overlapped with the
    dW GEMMs that costs far more than the persistence wins (0.7 % of the world-1 config-4 proxy,
    profiles/r5e).  The one-tile-per-workgroup launch lets the hardware rebalance around them."""
    import torch.distributed as dist

    # asked only for ph-5 shapes (a few fp32 dW GEMMs per layer): not cached, so a process that
    # brings a group up or down later is still answered right
    return dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1


def _policy() -> str:
    return os.environ.get("MXLLM_GEMM8", "table")


# (A k-contiguous, B k-contiguous) per form
_KC = {"tn": (True, True), "nn": (True, False), "tt": (False, False), "nt": (False, True)}


def g8_mat(t: torch.Tensor, kc: bool = True) -> tuple:
    """A 2-D row-strided tensor as ``g8_takes`` reads an operand: (base address, row stride in
    elements, k-contiguous).  Works on ``meta`` tensors (address 0)."""
    return (t.data_ptr(), t.stride(0), bool(kc))


def g8_shape_ok(a_kc: bool, b_kc: bool, M: int, N: int, K: int) -> bool:
    """The shape rules of ``g8_takes``: whole 256 x 256 tiles; whole 64-wide K-tiles when an operand
    is k-contiguous."""
    return M > 0 and N > 0 and K > 0 and M % 256 == 0 and N % 256 == 0 and (K % 64 == 0 or not (a_kc or b_kc))


def g8_takes(entry: str, A: tuple, B: tuple, C: tuple, M: int, N: int, K: int, *, out_f32: bool = False,
             beta: float = 0.0, epi: str = "none", ep: dict | None = None, rows: bool = False, at: int = 0,
             ws: int = 0, ph: int = 8, sq: int = 0) -> bool:
    """Whether the gemm8 launcher ``entry`` ("plain", "sq", "epi", "tail", "rope_tail": mx_gemm8,
    mx_gemm8_sq, ...) takes the launch -- the mirror of ``mx::g8_takes`` (csrc/kernels/gemm8_args.h,
    rule for rule, in its order; tests/test_gemm8_args.py runs both over one grid).  ``A`` / ``B`` /
    ``C``: ``g8_mat`` triples; ``epi``: "none", "rope", "swiglu", "swiglu_bwd"; ``ep``: the G8Epi
    fields by name (addresses as ints, absent = 0); ``ws`` / ``sq``: addresses."""
    e = ep or {}
    (pa, lda, a_kc), (pb, ldb, b_kc), (pc, ldc, _) = A, B, C
    tail = entry in ("tail", "rope_tail")
    rope = entry in ("epi", "rope_tail") and epi == "rope"
    swiglu = entry == "epi" and epi == "swiglu"
    swiglu_bwd = entry == "epi" and epi == "swiglu_bwd"
    if entry in ("epi", "rope_tail"):  # fused forward epilogues are TN, SWIGLU_BWD is NN
        if not (rope or swiglu or swiglu_bwd) or not a_kc or b_kc == swiglu_bwd:
            return False
    elif epi != "none":
        return False
    if not g8_shape_ok(a_kc, b_kc, M, N, K):
        return False
    if lda % 8 or ldb % 8 or pa % 16 or pb % 16:
        return False
    if lda < (K if a_kc else M) or ldb < (K if b_kc else N):
        return False
    # spans under 2^31 bytes: 256 rows of a k-contiguous operand, the K-tile-padded rows of an
    # mn-contiguous one; the fused TN epilogues gather weight rows from the whole matrix (N rows)
    kpad = (K + 63) // 64 * 64
    if (256 if a_kc else kpad) * lda >= 2 ** 30:
        return False
    if ((N if rope or swiglu else 256) if b_kc else kpad) * ldb >= 2 ** 30:
        return False
    if beta not in (0.0, 1.0):
        return False
    if not rope and (pc % 16 or ldc % (4 if out_f32 else 8) or ldc < (2 * N if swiglu_bwd else N)):
        return False
    if entry == "sq" and not sq:
        return False
    if entry == "tail" and sq and ph != 4:
        return False
    if tail:
        rest = (M if rows else N) - at
        if K < 128 or at <= 0 or rest <= 0 or at % 256 or rest % 256 or ws % 16:
            return False
    if rope:
        S = e.get("S", 0)
        if N != (e.get("Hq", 0) + 2 * e.get("Hkv", 0)) * 128 or S <= 0 or S % 256 or M % S:
            return False
        if any(not e.get(f, 0) for f in ("q", "k", "v", "cosb", "sinb")) or any(e[f] % 16 for f in ("q", "k", "v")):
            return False
        if entry == "rope_tail" and (e["cosb"] % 16 or e["sinb"] % 16):
            return False
    if swiglu:
        m, ldm = e.get("m", 0), e.get("ldm", 0)
        if (N // 2) % 128 or not pc or not m or ldm < N // 2 or ldm % 8 or m % 16:
            return False
    if swiglu_bwd:
        gu, ldg, m, ldm = e.get("gu", 0), e.get("ldg", 0), e.get("m", 0), e.get("ldm", 0)
        if not pc or not gu or ldg < 2 * N or ldg % 8 or gu % 16:
            return False
        if m and (ldm < N or ldm % 8 or m % 16):
            return False
    return True


_NEW = 16  # stands for a buffer the op allocates itself: non-null, 16-B aligned, contiguous


def _row_major(*ts: torch.Tensor) -> bool:
    """2-D with a unit inner stride: what the bindings require of every gemm8 operand."""
    return all(t.dim() == 2 and t.stride(1) == 1 for t in ts)


def g8_rope_takes(x2: torch.Tensor, w: torch.Tensor, S: int, Hq: int, Hkv: int, at: int = 0) -> bool:
    """``g8_takes`` of the fused qkv projection x2 [B*S, K] @ w [(Hq + 2 Hkv) * 128, K]^T (gemm8_rope;
    with ``at``: gemm8_rope_tail split at that column) into fresh q / k / v and 16-B aligned tables."""
    ep = {"q": _NEW, "k": _NEW, "v": _NEW, "cosb": _NEW, "sinb": _NEW, "S": S, "Hq": Hq, "Hkv": Hkv}
    return _row_major(x2, w) and g8_takes("rope_tail" if at else "epi", g8_mat(x2), g8_mat(w), (0, 0, True),
                                          x2.shape[0], w.shape[0], x2.shape[1], epi="rope", ep=ep, at=at, ws=_NEW)


def g8_swiglu_takes(x2: torch.Tensor, w: torch.Tensor) -> bool:
    """``g8_takes`` of the fused gate-up projection x2 [T, K] @ w [2F, K]^T (gemm8_swiglu) into fresh
    gu [T, 2F] and m [T, F]."""
    N = w.shape[0]
    return _row_major(x2, w) and g8_takes("epi", g8_mat(x2), g8_mat(w), (_NEW, N, True), x2.shape[0], N,
                                          x2.shape[1], epi="swiglu", ep={"m": _NEW, "ldm": N // 2})


def g8_swiglu_bwd_takes(T: int, wd: torch.Tensor) -> bool:
    """``g8_takes`` of the down projection's dX GEMM with the SwiGLU backward fused (gemm8_swiglu_bwd):
    a contiguous dy [T, H] and wd [H, F] into a fresh dgu [T, 2F], from a contiguous gu."""
    if not _row_major(wd):
        return False
    H, F = wd.shape
    return g8_takes("epi", (_NEW, H, True), g8_mat(wd, False), (_NEW, 2 * F, True), T, F, H, epi="swiglu_bwd",
                    ep={"gu": _NEW, "ldg": 2 * F})


def takes(form: str, M: int, N: int, K: int) -> bool:
    """Shape constraints of the kernel: the shape rules of ``g8_takes`` (a dispatch decision sees
    shapes only; strides, alignment and spans are the launcher's to refuse, and ``mm`` then falls
    back)."""
    return g8_shape_ok(*_KC[form], M, N, K)


def tail_at(form: str, M: int, N: int, K: int, out_dtype: torch.dtype) -> int:
    """The tail split this dispatch uses for the shape (the win table's ``tail`` entry; the sign
    convention of ``tail_split``): > 0 a column, < 0 a row, 0 no tail-balanced launch."""
    _table()
    return _TAIL.get((form, M, N, K, "f32" if out_dtype == torch.float32 else "bf16"), 0)


def schedule(form: str, M: int, N: int, K: int, out_dtype: torch.dtype) -> int:
    """0 = not on gemm8; else its phase schedule (8 or 4) for this shape."""
    pol = _policy()
    if pol == "0" or not takes(form, M, N, K):
        return 0
    ph = _table().get((form, M, N, K, "f32" if out_dtype == torch.float32 else "bf16"), 0)
    if ph == 5 and _multi_rank():
        ph = 4  # persistent kernel: world 1 only (see _multi_rank)
    if ph:
        return ph
    return DEFAULT_PH if (pol == "all" or deterministic()) else 0


DEFAULT_PH = int(os.environ.get("MXLLM_GEMM8_DEFAULT_PH", "4"))


def want(form: str, M: int, N: int, K: int, out_dtype: torch.dtype) -> bool:
    return schedule(form, M, N, K, out_dtype) > 0


def _dims(form, a, b):
    if form == "tn":
        return a.shape[0], b.shape[0], a.shape[1]
    if form == "nn":
        return a.shape[0], b.shape[1], a.shape[1]
    if form == "tt":
        return a.shape[1], b.shape[1], a.shape[0]
    return a.shape[1], b.shape[0], a.shape[0]


def mm(form: str, a: torch.Tensor, b: torch.Tensor, out: torch.Tensor | None = None, beta: float = 0.0,
       alpha_t: torch.Tensor | None = None, out_dtype: torch.dtype | None = None) -> torch.Tensor:
    """``out = beta * out + alpha_t * op(a) op(b)`` in operand order ``form`` (module doc).
    ``out`` None: a new [M, N] tensor of ``out_dtype`` (default: a's dtype) and beta is 0.
    ``alpha_t``: optional 1-element f32 device scalar (no host sync)."""
    M, N, K = _dims(form, a, b)
    odt = out.dtype if out is not None else (out_dtype or a.dtype)
    if out is None:
        out = torch.empty(M, N, dtype=odt, device=a.device)
        beta = 0.0
    ph = (schedule(form, M, N, K, odt) if use_native(a) and a.dtype == torch.bfloat16 and b.dtype == torch.bfloat16
          and odt in (torch.bfloat16, torch.float32) else 0)
    if ph:
        a_kc, b_kc = _KC[form]
        t = tail_at(form, M, N, K, odt)
        if (t and beta == 0.0 and alpha_t is None and odt == torch.bfloat16
                and native().gemm8_tail(a, a_kc, b, b_kc, out, abs(t), t < 0, ph)):
            return out
        if native().gemm8(a, a_kc, b, b_kc, out, float(beta), alpha_t, 1.0, ph):
            return out
    A = a if form in ("tn", "nn") else a.t()
    B = b.t() if form in ("tn", "nt") else b
    if alpha_t is not None:
        A = A * alpha_t.to(A.dtype)
    if odt == a.dtype:
        if beta == 0.0:
            return torch.mm(A, B, out=out)
        return out.addmm_(A, B, beta=beta)
    if a.is_cuda:  # bf16 operands, fp32 output (hipBLASLt D = C in fp32)
        return torch.ops.aten.addmm.dtype_out(out, A, B, odt, beta=beta, out=out)
    return out.mul_(beta).add_(A.float() @ B.float()) if beta != 0.0 else out.copy_(A.float() @ B.float())


def mm_sq(form: str, a: torch.Tensor, b: torch.Tensor, out: torch.Tensor, sq: torch.Tensor,
          alpha_t: torch.Tensor | None = None) -> bool:
    """``out = alpha_t * op(a) op(b)`` (bf16, beta 0) on gemm8 that also writes one fp32 sum of squares of
    the stored values per 256 x 256 output tile into ``sq`` (row-major tile order).  Only where the
    dispatch puts this shape on the plain 4-phase gemm8 anyway (same kernel, same bits in ``out``);
    False: nothing launched, the caller takes ``mm``."""
    M, N, K = _dims(form, a, b)
    if not (use_native(a) and a.dtype == b.dtype == out.dtype == torch.bfloat16 and M % 256 == 0 and N % 256 == 0):
        return False
    if schedule(form, M, N, K, torch.bfloat16) != 4:
        return False
    a_kc, b_kc = _KC[form]
    t = tail_at(form, M, N, K, torch.bfloat16)
    if t and alpha_t is None:  # the tail-balanced launch, as ``mm`` takes it (its split part sums per tile)
        return bool(native().gemm8_tail(a, a_kc, b, b_kc, out, abs(t), t < 0, 4, sq))
    return bool(native().gemm8_sq(a, a_kc, b, b_kc, out, sq, alpha_t, 1.0))
