"""CPU tests of the sampler reference (tests/_sampler_ref.py) and of the inputs of the exact GPU
sampler tests (tests/_sampler_cases.py): the hash and the uniform are what the kernels compute,
the kept set agrees with ``filter_probs``, every case is decidable within the caps, and the
head / tail rows show a kept set that is off by one token.

Shares left out (reference margin <= 1e-3), measured over the case lists of
tests/_sampler_cases.py: about 0.2 % of the draws at V 1000 ... 4099, none of the 32 draws of a
large-V case (about 0.05 % expected at V 128256); the cap is MAX_OMITTED = 1 % per case.
"""
import numpy as np
import pytest
import torch

from mxllm.ops import decode as dops
from tests import _sampler_cases as C
from tests import _sampler_ref as R


def _hash3_int(a, b, c):
    m = 0xFFFFFFFF
    h = (a * 0x9E3779B1 & m) ^ ((b + 0x7F4A7C15 & m) * 0x85EBCA77 & m) ^ ((c + 0x165667B1 & m) * 0xC2B2AE3D & m)
    h ^= h >> 15
    h = h * 0x2C1B3C6D & m
    h ^= h >> 12
    h = h * 0x297A2D39 & m
    h ^= h >> 15
    return h


def test_hash3_wraps_like_uint32():
    rng = np.random.default_rng(0)
    a, b, c = (rng.integers(0, 2 ** 32, 500) for _ in range(3))
    got = R.hash3(a, b, c)
    assert got.dtype == np.uint32
    assert got.tolist() == [_hash3_int(int(x), int(y), int(z)) for x, y, z in zip(a, b, c)]
    # broadcasting: [steps, 1] x [1, tokens]
    g2 = R.hash3(7, np.arange(3)[:, None], np.arange(5)[None, :])
    assert g2.shape == (3, 5) and int(g2[2, 4]) == _hash3_int(7, 2, 4)
    # seeds are taken modulo 2^32 (the kernel's uint32(seed))
    assert int(R.hash3(2 ** 32 + 5, 1, 2)[0]) == _hash3_int(5, 1, 2)
    assert int(R.hash3(-1, 1, 2)[0]) == _hash3_int(0xFFFFFFFF, 1, 2)


def test_recorded_u1_triples():
    for (seed, step, tok) in C.U1_V1000 + (C.U1_V128K,):
        h = R.hash3(seed, step, tok)
        assert int(h[0]) >> 8 == 0xFFFFFF
        assert float(R.uniform(h, clamp=False)[0]) == 1.0 and float(R.uniform(h)[0]) < 1.0
    assert C.find_u1(1000, 200000, 3) == C.U1_V1000
    # default seed 0 at V = 128256: the first steps with such a token
    steps = np.arange(0, 322)
    hits = []
    for s0 in range(0, steps.size, 46):
        h = R.hash3(0, steps[s0:s0 + 46, None], np.arange(128256)[None, :])
        si, ti = np.nonzero((h >> np.uint32(8)) == np.uint32(0xFFFFFF))
        hits += [(int(steps[s0 + a]), int(b)) for a, b in zip(si, ti)]
    assert sorted(hits) == [(92, 19773), (139, 103693), (321, 81931)]


def test_uniform_is_inside_the_unit_interval_exhaustively():
    h = np.arange(1 << 24, dtype=np.uint32) << np.uint32(8)
    raw, u = R.uniform(h, clamp=False), R.uniform(h)
    assert u.dtype == np.float32
    assert float(u.min()) == 2.0 ** -25 and float(u.max()) == float(R.U_MAX) < 1.0
    assert np.nonzero(raw == np.float32(1.0))[0].tolist() == [0xFFFFFF]  # the one value the clamp changes
    assert np.array_equal(raw[:-1], u[:-1])
    assert np.all(np.diff(u.astype(np.float64)) >= 0)
    g = -np.log(-np.log(u.astype(np.float64)))
    assert np.isfinite(g).all() and g.max() < 16.7


def test_seed_rule_and_scores():
    assert R.row_seed(0, 3) == 3 * 7919 and R.row_seed(2 ** 32 - 1, 1) == 7918
    row = torch.tensor([0.5, -1.0, 2.0, float("-inf")]).bfloat16()
    s = R.scores(row, 0.7, 9, 4)
    u = R.uniform(R.hash3(9, 4, np.arange(4))).astype(np.float64)
    want = row.double().numpy() / float(np.float32(0.7)) - np.log(-np.log(u))
    assert np.array_equal(s, want) and s[3] == -np.inf
    tok, margin = R.draw(row, 0.7, 9, 4)
    assert tok == int(np.argmax(s)) and margin == pytest.approx(np.sort(s)[-1] - np.sort(s)[-2])
    toks, margins = R.draw(row, 0.7, 9, np.arange(6))
    assert toks.shape == (6,) and toks[4] == tok and margins[4] == margin
    # greedy and exact ties: the smallest index
    assert R.draw(torch.tensor([1.0, 3.0, 3.0, 0.0]), 0.0, 1, 0) == (1, float("inf"))


def test_kept_rules():
    x = torch.tensor([2.0, 1.0, 1.0, 0.0, -0.0, -1.0, float("-inf")])
    assert R.kept(x, 1.0, 2)[0].tolist() == [True, True, True, False, False, False, False]  # tie at rank 2
    assert R.kept(x, 1.0, 4)[0].tolist() == [True, True, True, True, True, False, False]   # -0.0 == +0.0
    assert R.kept(x, 1.0, 0)[0].all() and R.kept(x, 1.0, 7)[0].all() and R.kept(x, 1.0, -2)[0].all()
    w = np.exp(np.array([0.0, -1.0, -1.0, -2.0, -2.0, -3.0]))
    z, c1, c2 = w.sum(), w[0], w[:3].sum()
    keep, gap = R.kept(x, 1.0, 0, (c1 + c2) / 2 / z)  # crossing inside the tied pair: both kept
    assert keep.tolist() == [True, True, True, False, False, False, False]
    assert gap == pytest.approx((c2 - c1) / 2 / z, rel=1e-5)
    keep, _ = R.kept(x, 1.0, 0, (c2 + w[:5].sum()) / 2 / z)    # crossing inside the zeros: both signs kept
    assert keep.tolist() == [True, True, True, True, True, False, False]
    keep, _ = R.kept(x, 1.0, 3, 0.999)  # the nucleus is taken inside the top-k set
    assert keep.tolist() == [True, True, True, False, False, False, False]
    assert R.kept(x, 0.25, 0, 0.9)[0].sum() == 1 and R.kept(x, 4.0, 0, 0.9)[0].sum() >= 5  # temperature first


def test_kept_agrees_with_filter_probs():
    g = torch.Generator().manual_seed(3)
    compared = 0
    for i in range(60):
        V = [64, 257, 1000][i % 3]
        row = (torch.randn(V, generator=g) * 2.0).to([torch.bfloat16, torch.float32][i % 2])
        T = [0.5, 1.0, 1.6][i % 3]
        k = [0, 5, 40, V + 3][i % 4]
        p = [1.0, 0.9, 0.5, 0.3][(i // 4) % 4]
        keep, gap = R.kept(row, T, k, p)
        if gap < 1e-5:  # fp32 filter_probs may put the crossing on the neighbouring token
            continue
        compared += 1
        assert np.array_equal(keep, (dops.filter_probs(row, T, k, p) > 0).numpy()), (i, V, T, k, p)
    assert compared >= 55


def test_every_case_is_decidable_within_the_caps():
    """At most MAX_OMITTED of a case's draws have a margin <= MARGIN; every top-p draw has
    top_p * Z at least GAP * Z away from the cumulative masses around it, at V <= 4099."""
    fam: dict = {}
    for c in C.all_cases():
        ids, margin, gap = C.expected(c.name)
        dec = margin > C.MARGIN
        left = int((~dec).sum())
        assert left <= C.MAX_OMITTED * c.n, (c.name, left, c.n)
        topp = (c.temps > 0) & (c.top_ps < 1)
        if topp.any():
            assert c.base.shape[1] <= C.TOP_P_MAX_V, c.name
            assert gap[topp].min() >= C.GAP, (c.name, gap[topp].min())
        x = R.as_f64(c.base)
        t_min = float(c.temps[c.temps > 0].min(initial=1.0))
        assert np.abs(x[np.isfinite(x)]).max() / t_min + 17 < 64, c.name  # the score magnitude the margin is sized for
        t = fam.setdefault(c.family, [0, 0])
        t[0] += c.n * len(c.entries)
        t[1] += left * len(c.entries)
    for k, (n, left) in fam.items():  # shown with pytest -s
        print(f"[sampler cases] {k}: {n - left} draws compared, {left} left out")


def test_head_tail_cases_show_a_kept_set_off_by_one():
    """A kept set one head token too small or too large changes at least 5 % of the 512 reference
    draws (expected: that token's mass, 1 / j ... 1 / (j + 1)).  Past the 16th head token the next
    token is a tail token of mass ~1e-4, so there only 'too small' is visible."""
    seen = 0
    for c in C.all_cases():
        j = c.note.get("j")
        if j is None:
            continue
        row, T, k, p = c.base[0], float(c.temps[0]), int(c.top_ks[0]), float(c.top_ps[0])
        assert c.n == C.N_STEPS == 512 and c.steps.tolist() == list(range(512)), c.name
        assert int(R.kept(row, T, k, p)[0].sum()) == j, c.name
        shares = C.off_by_one_shares(row, T, int(c.seeds[0]), j, top_k=0 if p >= 1 else k, by_mass=p < 1)
        assert len(shares) == (1 if j == C.HEAD else 2), c.name
        assert min(shares) >= 0.05, (c.name, shares)
        seen += len(shares)
    assert seen >= 60


def test_special_rows_are_what_the_cases_say():
    for c in C.all_cases():
        ids, _, _ = C.expected(c.name)
        if c.family == "zeros":  # the -0.0 tokens are in the kept set and are drawn
            nz = C.neg_zero_tokens(c.base[0])
            keep = R.kept(c.base[0], 1.0, int(c.top_ks[0]), float(c.top_ps[0]))[0]
            assert nz.size == 3 and keep[nz].all() and keep.sum() == 11, c.name
            assert np.isin(ids, nz).mean() > 0.1, c.name
        if c.family == "u == 1.0":
            tok = c.note["token"]
            sel = c.b == c.note["row"]
            x = R.as_f64(c.base[c.note["row"]])
            fin = x[np.isfinite(x)]
            assert x[tok] == fin.min() and fin.max() - x[tok] == 20.0, c.name
            assert int(R.hash3(c.seeds[sel][0], c.steps[sel][0], tok)[0]) >> 8 == 0xFFFFFF, c.name
            assert R.kept(c.base[c.note["row"]], 1.0, int(c.top_ks[sel][0]), 1.0)[0][tok], c.name
            assert (ids[sel] != tok).all(), c.name
        if c.family == "-inf entries":
            assert np.isfinite(R.as_f64(c.base)[c.b, ids]).all(), c.name
        if c.family == "top-k sets" and "tie" in c.note:
            assert int(R.kept(c.base[0], 1.0, c.note["tie"])[0].sum()) == c.note["tie"] + 1, c.name
        if c.family == "greedy ties":
            assert ids.tolist() == [min(t) for t in c.note["ties"]], c.name
