"""CPU reference of the HIP samplers (csrc/kernels/decode.hip sample_kernel /
sample_final_kernel, csrc/kernels/sampling.hip sample_topkp_kernel): numpy / torch, no GPU.

The kernels are deterministic: the noise of token ``i`` at (seed, step) is an integer hash
mapped to a uniform ``u`` in (0, 1), the draw is the argmax of ``x / T - log(-log(u))`` over
the kept set, smallest index on ties.  Here the hash and ``u`` are reproduced bit for bit
(uint32 / float32) and everything after them is fp64, so a single draw of a kernel can be
compared with ``draw()`` whenever the reference margin between the best and the second-best
score is larger than the kernel's f32 score error.

The kept set (``kept``) is written from the documented rule, independently of
``mxllm.ops.decode.filter_probs``: top-k by value with ties kept (``-0.0 == +0.0``), then the
smallest most-likely prefix of that set whose fp64 mass reaches ``top_p`` of the set's mass,
the crossing token and its ties kept.
"""
from __future__ import annotations

import numpy as np
import torch

M32 = 0xFFFFFFFF
ROW_SEED_STRIDE = 7919  # sample(logits, T, seed, step): row r draws with seed + 7919 * r
U_MAX = np.float32(1.0) - np.float32(2.0 ** -24)  # 0x1.fffffep-1: the largest float32 below 1


def _u32(v) -> np.ndarray:
    return (np.asarray(v, dtype=np.int64) & M32).astype(np.uint32)


def hash3(seed, step, idx) -> np.ndarray:
    """The kernels' 32-bit hash of (seed, step, token index), vectorised with broadcasting.
    Every product and sum wraps modulo 2^32 (uint32 arrays)."""
    a, b, c = np.atleast_1d(_u32(seed)), np.atleast_1d(_u32(step)), np.atleast_1d(_u32(idx))
    k = np.uint32
    with np.errstate(over="ignore"):
        h = (a * k(0x9E3779B1)) ^ ((b + k(0x7F4A7C15)) * k(0x85EBCA77)) ^ ((c + k(0x165667B1)) * k(0xC2B2AE3D))
        h ^= h >> k(15)
        h *= k(0x2C1B3C6D)
        h ^= h >> k(12)
        h *= k(0x297A2D39)
        h ^= h >> k(15)
    return h


def uniform(h, clamp: bool = True) -> np.ndarray:
    """The kernels' ``u`` of a hash value, in float32 arithmetic: ((h >> 8) + 0.5) * 2^-24,
    clamped to the largest float32 below 1.  (The f32 sum rounds to even above 2^23, so
    without the clamp h >> 8 == 0xFFFFFF gives exactly 1.0; the multiplication by a power of
    two is exact, so a fused multiply-add gives the same bits.)"""
    m = (np.asarray(h, dtype=np.uint32) >> np.uint32(8)).astype(np.float32)
    u = (m + np.float32(0.5)) * np.float32(1.0 / 16777216.0)
    assert u.dtype == np.float32
    return np.minimum(u, U_MAX) if clamp else u


def row_seed(seed: int, r: int) -> int:
    """Seed of row ``r`` in ``sample(logits, T, seed, step)``."""
    return (int(seed) + ROW_SEED_STRIDE * int(r)) & M32


def as_f64(row) -> np.ndarray:
    """The row exactly as stored (bf16 or f32), widened to fp64."""
    if isinstance(row, torch.Tensor):
        return row.detach().cpu().double().numpy()
    return np.asarray(row).astype(np.float64)


def _temp64(temp) -> float:
    return float(np.float32(temp))  # the f32 value the kernel sees


def _scores_at(x: np.ndarray, idx: np.ndarray, temp, seed, steps: np.ndarray) -> np.ndarray:
    """fp64 scores [len(steps), len(idx)] of the tokens ``idx`` of the fp64 row ``x``."""
    u = uniform(hash3(seed, steps[:, None], idx[None, :])).astype(np.float64)
    with np.errstate(divide="ignore"):
        return x[idx][None, :] / _temp64(temp) - np.log(-np.log(u))


def scores(row, temp, seed, step) -> np.ndarray:
    """float64(row) / temp - log(-log(float64(u))) for every token of the row."""
    x = as_f64(row)
    return _scores_at(x, np.arange(x.size), temp, seed, np.atleast_1d(np.asarray(step, dtype=np.int64)))[0]


def kept(row, temp, top_k: int = 0, top_p: float = 1.0):
    """(mask, gap): the tokens a draw may return, and for top_p < 1 the fp64 distance, as a
    fraction of the set's mass Z, between top_p * Z and the nearest cumulative mass on either
    side (``inf`` without top-p).  A kernel that sums the masses in f32 decides the same set
    when its summation error is below ``gap``."""
    x = as_f64(row)
    V = x.size
    keep = np.ones(V, dtype=bool)
    if 0 < top_k < V:
        kth = np.sort(x)[V - top_k]  # k-th largest value
        keep &= x >= kth             # ties kept; -0.0 >= +0.0 holds
    gap = float("inf")
    p = float(np.float32(top_p))
    if p < 1.0:
        with np.errstate(invalid="ignore"):
            w = np.where(keep, np.exp((x - x.max()) / _temp64(temp)), 0.0)
        z = w.sum()
        target = max(p, 0.0) * z
        # distinct kept values in descending order (np.unique merges -0.0 with +0.0); the mass
        # of a value is the mass of all its ties
        vals, inv = np.unique(x[keep], return_inverse=True)
        mass = np.bincount(inv, weights=w[keep], minlength=vals.size)[::-1]
        vals = vals[::-1]
        incl = np.cumsum(mass)
        j = int(np.argmax(incl >= target)) if (incl >= target).any() else vals.size - 1
        keep &= x >= vals[j]
        excl = incl[j] - mass[j]
        gap = float(min(incl[j] - target, target - excl) / z)
    return keep, gap


def draw(row, temp, seed, step, top_k: int = 0, top_p: float = 1.0):
    """(token, margin) of one draw, or arrays over ``step`` when it is an array: the argmax of
    the scores over the kept set, smallest index on ties, and the fp64 margin between the
    best and the second-best score (``inf`` when nothing else is finite, and for greedy rows,
    whose result does not depend on rounding)."""
    x = as_f64(row)
    steps = np.atleast_1d(np.asarray(step, dtype=np.int64))
    if not (float(temp) > 0.0):
        tok = np.full(steps.size, int(np.argmax(x)), dtype=np.int64)  # first maximum
        margin = np.full(steps.size, np.inf)
    else:
        keep, _ = kept(row, temp, top_k, top_p)
        idx = np.nonzero(keep)[0]
        s = _scores_at(x, idx, temp, seed, steps)
        j = np.argmax(s, axis=1)  # first maximum = smallest token index
        best = s[np.arange(steps.size), j]
        s[np.arange(steps.size), j] = -np.inf
        second = s.max(axis=1) if idx.size > 1 else np.full(steps.size, -np.inf)
        tok = idx[j].astype(np.int64)
        with np.errstate(invalid="ignore"):
            margin = np.where(np.isfinite(second), best - second, np.inf)
    if np.ndim(step) == 0:
        return int(tok[0]), float(margin[0])
    return tok, margin
