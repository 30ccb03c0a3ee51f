"""Inputs of the exact sampler tests, shared by tests/test_sampler_ref.py (CPU: the inputs are
decidable, the head / tail rows are sensitive to a kept set that is off by one) and
tests/test_sampler_exact_gpu.py (GPU: every decidable draw equals the reference).

A case is a small set of logits rows plus one (row, temperature, top_p, top_k, seed, step)
tuple per draw; ``expected`` computes the reference draws once per process.

Constants of the comparison (fixed by the precision of the formats, not by kernel output):

* MARGIN = 1e-3.  A draw is compared only if the fp64 margin between the best and the
  second-best score exceeds it.  Scores here have magnitude at most 64, so one f32 ulp is
  at most 3.8e-6; ``v * (1 / T)`` and the fast logarithms add a few more ulps.
* MAX_OMITTED = 1 %: the largest share of a case's draws that may be left out.  Measured
  on the reference: about 0.2 % at V 1000 / 4099, about 0.05 % at V 128256.
* GAP = 1e-3 of Z on either side of ``top_p * Z``: top_p sits in the middle of a gap of at
  least 2e-3 Z between consecutive cumulative masses.  The worst-case f32 summation error
  of the kernel's mass histogram is V * 2^-24 of Z, 2.4e-4 at V = 4099, so the top-p cases
  use V <= 4099.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np
import torch

from tests import _sampler_ref as R

MARGIN = 1e-3
MAX_OMITTED = 0.01
GAP = 1e-3
TOP_P_MAX_V = 4099
HEAD = 16  # head tokens of a head / tail row
DTYPES = (torch.bfloat16, torch.float32)
U1_V1000 = ((7055, 0, 446), (11614, 0, 596), (68748, 0, 805))  # (seed, step, token) with u == 1.0 unclamped
U1_V128K = (0, 92, 19773)


def _dn(dtype) -> str:
    return "bf16" if dtype == torch.bfloat16 else "f32"


@dataclass
class Case:
    name: str
    family: str
    base: torch.Tensor      # [nb, V] logits as stored (bf16 or f32)
    b: np.ndarray           # per draw: row of `base`
    temps: np.ndarray       # float32
    top_ps: np.ndarray      # float32
    top_ks: np.ndarray      # int32
    seeds: np.ndarray       # int64 (the kernel takes uint32(seed))
    steps: np.ndarray       # int32
    entries: tuple = ("rows",)           # which of sample / temp_rows / rows serve it
    sample_call: tuple | None = None     # (T, seed0, steps): draws are step-major, row = r % nb
    note: dict = field(default_factory=dict)

    @property
    def n(self) -> int:
        return self.b.size


def _case(name, family, base, specs, **kw) -> Case:
    """specs: (row, temp, top_p, top_k, seed, steps) groups; draws are laid out group by group."""
    cols = [[], [], [], [], [], []]
    for (b, t, p, k, seed, steps) in specs:
        steps = np.atleast_1d(np.asarray(steps))
        for c, v in zip(cols, (b, t, p, k, seed, None)):
            c.append(steps if v is None else np.full(steps.size, v))
    b, t, p, k, seed, steps = (np.concatenate(c) for c in cols)
    return Case(name, family, base, b.astype(np.int64), t.astype(np.float32), p.astype(np.float32),
                k.astype(np.int32), seed.astype(np.int64), steps.astype(np.int32), **kw)


def _sample_case(name, family, base, temp, seed0, steps, top_p=1.0, top_k=0, entries=("sample", "temp_rows", "rows"),
                 **kw) -> Case:
    """The draws of ``sample(base, temp, seed0, step)`` for every step, step-major; the per-row
    entry points get the same draws through seeds[r] = seed0 + 7919 * row."""
    nb = base.shape[0]
    specs = [(r, temp, top_p, top_k, R.row_seed(seed0, r), [s]) for s in steps for r in range(nb)]
    return _case(name, family, base, specs, entries=entries, sample_call=(float(temp), int(seed0), list(steps)), **kw)


@functools.lru_cache(maxsize=None)
def expected(case_name: str):
    """(ids, margin, gap) per draw of a case: reference token, fp64 score margin, top-p gap."""
    c = by_name()[case_name]
    ids = np.zeros(c.n, dtype=np.int64)
    margin = np.zeros(c.n)
    gap = np.full(c.n, np.inf)
    keys = np.stack([c.b, c.temps.view(np.int32), c.top_ps.view(np.int32), c.top_ks, c.seeds], axis=1)
    _, first, inv = np.unique(keys, axis=0, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    for g, r0 in enumerate(first):
        sel = np.nonzero(inv == g)[0]
        row = c.base[int(c.b[r0])]
        t, p, k = float(c.temps[r0]), float(c.top_ps[r0]), int(c.top_ks[r0])
        ids[sel], margin[sel] = R.draw(row, t, int(c.seeds[r0]), c.steps[sel], k, p)
        if t > 0 and p < 1.0:
            gap[sel] = R.kept(row, t, k, p)[1]
    return ids, margin, gap


def decidable(case_name: str) -> np.ndarray:
    _, margin, _ = expected(case_name)
    return margin > MARGIN


# ---------------------------------------------------------------- rows
def rand_rows(nb: int, V: int, dtype, gseed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(gseed)
    return (torch.randn(nb, V, generator=g) * 2.0).to(dtype)


def head_tail_row(V: int, dtype, gseed: int, tie_rank: int = 0) -> torch.Tensor:
    """HEAD = 16 distinct head logits 4 + i / 32 (exact in bf16) at random positions, the rest
    N(-4, 1).  The head holds nearly all the mass in nearly equal shares, so one head token
    more or less in the kept set moves 1 / j of the draws.  tie_rank = r: the head tokens of
    rank r and r + 1 (1-based, descending) are equal."""
    g = torch.Generator().manual_seed(gseed)
    x = (torch.randn(V, generator=g) - 4.0).clamp(max=2.0)
    pos = torch.randperm(V, generator=g)[:HEAD]
    vals = 4.0 + torch.randperm(HEAD, generator=g).float() / 32.0
    if tie_rank:
        srt = vals.sort(descending=True).values
        vals[vals == srt[tie_rank]] = srt[tie_rank - 1]
    x[pos] = vals
    return x.to(dtype)


def top_p_after(row: torch.Tensor, temp: float, j: int, top_k: int = 0) -> float:
    """top_p (as f32) in the middle of the cumulative-mass gap that keeps exactly the j most
    likely distinct values of the (top-k restricted) row."""
    x = R.as_f64(row)
    if 0 < top_k < x.size:
        x = x[x >= np.sort(x)[x.size - top_k]]
    vals, cnt = np.unique(x, return_counts=True)
    mass = (np.exp((vals - vals.max()) / float(np.float32(temp))) * cnt)[::-1]
    cum = np.concatenate([[0.0], np.cumsum(mass)])
    return float(np.float32((cum[j - 1] + cum[j]) / 2.0 / cum[-1]))


def zeros_row(V: int, dtype, gseed: int) -> torch.Tensor:
    """3 positive logits, 5 tokens at +0.0, 3 at -0.0, the rest strictly negative."""
    g = torch.Generator().manual_seed(gseed)
    x = (-6.0 - torch.rand(V, generator=g)).float()
    pos = torch.randperm(V, generator=g)[:11]
    x[pos[:3]] = torch.tensor([0.5, 0.375, 0.25])
    x[pos[3:8]] = 0.0
    x[pos[8:11]] = -0.0
    x = x.to(dtype)
    assert int(torch.signbit(x[pos[8:11]]).sum()) == 3 and int(torch.signbit(x[pos[3:8]]).sum()) == 0
    return x


def neg_zero_tokens(row: torch.Tensor) -> np.ndarray:
    return np.nonzero(((row == 0) & torch.signbit(row)).numpy())[0]


def flat_rows(V: int, gseed: int) -> torch.Tensor:
    """f32 [2, V]: 1 + perm(j) * 2^-23 and its negation: keys that differ only in their low 10
    bits (the last radix digit); the negative row's keys are the complemented bits."""
    g = torch.Generator().manual_seed(gseed)
    x = 1.0 + torch.randperm(V, generator=g).double() * 2.0 ** -23
    x = x.float()
    assert x.unique().numel() == V
    return torch.stack([x, -x])


def poisoned_row(V: int, dtype, gseed: int, token: int, finite: int = 0) -> torch.Tensor:
    """`token` holds the lowest finite logit, the maximum is 20 above it.  finite = m > 0: only
    m tokens are finite, the rest -inf."""
    g = torch.Generator().manual_seed(gseed)
    x = (torch.randn(V, generator=g) * 2.0).clamp(-6.0, 6.0)
    others = [i for i in torch.randperm(V, generator=g).tolist() if i != token]
    if finite:
        x[others[finite - 1:]] = float("-inf")
    x[token] = -10.0
    x[others[0]] = 10.0
    return x.to(dtype)


def find_u1(V: int, n_seeds: int, want: int, step: int = 0):
    """The first `want` (seed, step, token) with h >> 8 == 0xFFFFFF among seeds < n_seeds."""
    found = []
    tok = np.arange(V)
    for s0 in range(0, n_seeds, 2000):
        h = R.hash3(np.arange(s0, min(n_seeds, s0 + 2000))[:, None], step, tok[None, :])
        si, ti = np.nonzero((h >> np.uint32(8)) == np.uint32(0xFFFFFF))
        found += [(s0 + int(a), step, int(b)) for a, b in zip(si, ti)]
        if len(found) >= want:
            break
    return tuple(sorted(found)[:want])


# ---------------------------------------------------------------- case lists
N_STEPS = 512  # rows of one launch in the kept-set cases
SENSITIVITY = 0.05


def off_by_one_shares(row, temp, seed, j, top_k=0, by_mass=False) -> list:
    """Shares of the N_STEPS reference draws that change when the kept set holds j - 1 or j + 1
    instead of j head tokens (by top-k, or by a top_p placed by mass inside the top-k set).
    The j + 1 side is left out where the next token is not a head token or top-k excludes it."""
    steps = np.arange(N_STEPS)

    def draws(jj):
        if by_mass:
            return R.draw(row, temp, seed, steps, top_k, top_p_after(row, temp, jj, top_k))[0]
        return R.draw(row, temp, seed, steps, jj, 1.0)[0]

    ids = draws(j)
    sides = [j - 1] + ([j + 1] if j < HEAD and (not by_mass or not 0 < top_k < j + 1) else [])
    return [float((draws(jj) != ids).mean()) for jj in sides]


def sensitive_seed(row, temp, seed0, j, top_k=0, by_mass=False) -> int:
    """The first noise seed >= seed0 whose N_STEPS draws show a kept set off by one token in at
    least SENSITIVITY of the draws.  The expected share is the token's mass, 1 / j down to
    about 1 / 22 for the lightest of the 16 head tokens at T = 0.7, so at j = 16 not every
    seed's 512 draws reach 5 %; the choice depends on the reference alone."""
    for seed in range(seed0, seed0 + 64):
        if min(off_by_one_shares(row, temp, seed, j, top_k, by_mass)) >= SENSITIVITY:
            return seed
    raise AssertionError("no sensitive seed")


def _entry_cases():
    out = []
    for dtype in DTYPES:
        for V in (7, 1000, 1003, 2049, 4099):
            for ti, T in enumerate((0.3, 1.0, 1.7)):
                out.append(_sample_case(f"entry-{_dn(dtype)}-V{V}-T{T}", "entry points",
                                        rand_rows(3, V, dtype, 11 * V + ti), T, 1000 + V + ti, range(64)))
        for V in (128256, 200003):
            out.append(_sample_case(f"entry-{_dn(dtype)}-V{V}", "entry points, large V", rand_rows(4, V, dtype, V), 0.8,
                                    77 + V, range(8)))
        out.append(_sample_case(f"entry-{_dn(dtype)}-B1030", "entry points, 1030 rows",
                                rand_rows(1030, 1000, dtype, 1030), 1.0, 4242, [3], entries=("sample",)))
    return out


def _topk_cases():
    out = []
    steps = range(N_STEPS)
    for dtype in DTYPES:
        for V in (1000, 4099):
            for j in (5, 11, 16):
                row = head_tail_row(V, dtype, 100 * V + j)
                out.append(_case(f"topk-{_dn(dtype)}-V{V}-k{j}", "top-k sets", row[None],
                                 [(0, 1.0, 1.0, j, sensitive_seed(row, 1.0, 900, j), steps)], note={"j": j}))
            row = head_tail_row(V, dtype, 100 * V + 7, tie_rank=7)
            out.append(_case(f"topk-{_dn(dtype)}-V{V}-tie7", "top-k sets", row[None], [(0, 1.0, 1.0, 7, 907, steps)],
                             note={"tie": 7}))
    return out


def _radix_cases():
    base = flat_rows(1000, 5)
    specs = [(b, 1.0, 1.0, k, 3000 + 10 * i + b, range(64))
             for b in (0, 1) for i, k in enumerate((1, 8, 500, 999, 1000, 5000, 0, -3))]
    return [_case("radix-f32-flat", "radix depth", base, specs)]


def _topp_cases():
    out = []
    steps = range(N_STEPS)
    for dtype in DTYPES:
        for V in (1003, 4099):
            for T in (0.7, 1.0):
                for j in (5, 11, 16):
                    row = head_tail_row(V, dtype, 200 * V + j)
                    p = top_p_after(row, T, j)
                    out.append(_case(f"topp-{_dn(dtype)}-V{V}-T{T}-j{j}", "top-p sets", row[None],
                                     [(0, T, p, 0, sensitive_seed(row, T, 1900, j, by_mass=True), steps)],
                                     note={"j": j}))
            # nucleus inside the top-k set: 5 of the 8 kept (top_p of the whole row's mass would keep 9)
            row = head_tail_row(V, dtype, 200 * V + 8)
            p = top_p_after(row, 1.0, 5, top_k=8)
            out.append(_case(f"topkp-{_dn(dtype)}-V{V}-k8-j5", "top-k + top-p sets", row[None],
                             [(0, 1.0, p, 8, sensitive_seed(row, 1.0, 1908, 5, 8, by_mass=True), steps)],
                             note={"j": 5}))
    return out


def _zeros_cases():
    out = []
    for dtype in DTYPES:
        row = zeros_row(1000, dtype, 31)
        # rank 5 is a +0.0: top-k keeps 3 positives and all 8 zeros of either sign
        out.append(_case(f"zeros-{_dn(dtype)}-topk", "zeros", row[None], [(0, 1.0, 1.0, 5, 61, range(N_STEPS))]))
        # the mass of rank 4 (the zeros, 8 tokens) crosses top_p: 4 of its 8 units in, i.e. inside
        # the five +0.0 tokens when the two signs are told apart
        out.append(_case(f"zeros-{_dn(dtype)}-topp", "zeros", row[None],
                         [(0, 1.0, top_p_after(row, 1.0, 4), 0, 62, range(N_STEPS))]))
    return out


def _inf_cases():
    out = []
    for dtype in DTYPES:
        a = torch.full((1000,), float("-inf"))
        a[[17, 500, 999]] = torch.tensor([1.0, 0.5, 0.0])
        b = torch.full((1000,), float("-inf"))
        b[123] = -2.0
        base = torch.stack([a, b]).to(dtype)
        out.append(_case(f"inf-{_dn(dtype)}-k8-p0.9", "-inf entries", base,
                         [(0, 1.0, 0.9, 8, 71, range(64)), (1, 1.0, 0.9, 8, 72, range(64))]))
        out.append(_sample_case(f"inf-{_dn(dtype)}-plain", "-inf entries", base, 1.0, 73, range(64)))
    return out


MIXED_KINDS = ("greedy", "temperature", "top-k", "top-p", "both")


def _mixed_cases():
    out = []
    for dtype in DTYPES:
        V = 4099
        base = torch.stack([head_tail_row(V, dtype, 300 + i) for i in range(5)])
        specs = [(0, 0.0, 1.0, 0, 81, range(16)), (1, 0.9, 1.0, 0, 82, range(16)), (2, 1.0, 1.0, 11, 83, range(16)),
                 (3, 1.0, top_p_after(base[3], 1.0, 5), 0, 84, range(16)),
                 (4, 1.0, top_p_after(base[4], 1.0, 5, top_k=8), 8, 85, range(16))]
        out.append(_case(f"mixed-{_dn(dtype)}", "mixed batch", base, specs))
    return out


def _greedy_cases():
    out = []
    for dtype in DTYPES:
        for V in (8200, 8201):  # 8201: rows 1 and 2 are not 16-byte aligned (scalar reader)
            base = rand_rows(3, V, torch.float32, V).clamp(max=2.5)
            ties = ((5, 5 + 8 * 1024), (V - 1, 3), (10, 10 + 512 * 3))  # same thread; last / early; two waves
            for r, (i, j) in enumerate(ties):
                base[r, i] = base[r, j] = 3.0
            out.append(_sample_case(f"greedy-{_dn(dtype)}-V{V}", "greedy ties", base.to(dtype), 0.0, 5, [0],
                                    entries=("sample", "rows"), note={"ties": ties}))
    return out


def _u1_cases():
    out = []
    for dtype in DTYPES:
        for V, triples in ((1000, U1_V1000), (128256, (U1_V128K,))):
            for (seed, step, tok) in triples:
                plain = rand_rows(1, V, dtype, seed + 1)[0]
                # row 1 of a two-row sample() call: seed0 + 7919 = seed
                base = torch.stack([plain, poisoned_row(V, dtype, seed + 2, tok)])
                out.append(_sample_case(f"u1-{_dn(dtype)}-V{V}-s{seed}", "u == 1.0", base, 1.0, (seed - 7919) & R.M32,
                                        [step], note={"row": 1, "token": tok}))
                base = poisoned_row(V, dtype, seed + 3, tok, finite=50)[None]
                out.append(_case(f"u1-{_dn(dtype)}-V{V}-s{seed}-k50", "u == 1.0", base,
                                 [(0, 1.0, 1.0, 50, seed, [step])], note={"row": 0, "token": tok}))
    return out


@functools.lru_cache(maxsize=None)
def all_cases() -> tuple:
    out = (_entry_cases() + _topk_cases() + _radix_cases() + _topp_cases() + _zeros_cases() + _inf_cases()
           + _mixed_cases() + _greedy_cases() + _u1_cases())
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def by_name() -> dict:
    return {c.name: c for c in all_cases()}


def names(family: str | None = None) -> list:
    return [c.name for c in all_cases() if family is None or c.family.startswith(family)]
